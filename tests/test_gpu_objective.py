"""GPU tier of v- / x0-prediction and min-SNR loss weighting: dm3d_pred_to_eps and dm3d_objective_loss_grad bitwise against numpy
float32 restatements, the chains of a v- and an x0-model against the float64 chains of tests/chain_reference.py on the CPU oracle's
output read as v or as x0 and converted to eps (where the chain is guided, before the guidance), the single-call predict_eps, and training against torch.autograd with the loss written out here in float64.

The network is the oracle's (oracle.ref_torch.unet_forward on synthetic weights): what its output "means" is up to the chain, so the
same weights serve as an eps-, a v- and an x0-model."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chain_reference as cr

pytestmark = pytest.mark.gpu
CHAIN_BAR = 2e-3        # the project's chain bar (tests/test_gpu_ddim.py)
SIZES = [4, 1004, 131084]      # per_sample: one float4; a partial block; two grid-stride trips of 64 blocks and a tail of 3 float4
T_ROWS = (0, 517, 999)


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32) if t.dtype == torch.float32 else t.detach().cpu().contiguous().view(torch.int64)


# ---- dm3d_pred_to_eps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per", SIZES)
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_pred_to_eps_is_bitwise_the_float32_restatement(dev, kind, per):
    import dm3d_amd
    from dm3d_amd import _lib
    from dm3d_amd.diffusion import prediction_table
    T, B = 1000, 3
    table = prediction_table(dm3d_amd.Betas(T).alpha_bar, kind)
    rng = np.random.default_rng(per)
    pred, x = (rng.standard_normal((B, per)).astype(np.float32) for _ in range(2))
    want = np.stack([table[t, 0] * pred[b] + table[t, 1] * x[b] for b, t in enumerate(T_ROWS)])     # float32: mul, mul, add
    assert want.dtype == np.float32
    tab_d = torch.from_numpy(table).to(dev)
    x_d = torch.from_numpy(x).to(dev)
    guard = float(np.float32(-7.5))

    def run(t_rows, in_place):
        # pred sits inside a larger buffer with a guard float4 on either side: nothing outside [B, per] may be written
        buf = torch.full((B * per + 8,), guard, dtype=torch.float32, device=dev)
        p_d = buf[4:4 + B * per].view(B, per)
        p_d.copy_(torch.from_numpy(pred))
        obuf = torch.full((B * per + 8,), guard, dtype=torch.float32, device=dev)
        d = _lib.PredDesc()
        d.pred, d.x, d.table = p_d.data_ptr(), x_d.data_ptr(), tab_d.data_ptr()
        t_d = torch.tensor(t_rows, dtype=torch.int32, device=dev)
        d.t_idx, d.batch, d.per_sample, d.timesteps = t_d.data_ptr(), B, per, T
        if not in_place:
            d.out = obuf[4:].data_ptr()
        _lib.check(_lib.lib().dm3d_pred_to_eps(C.byref(d), _st()), "pred_to_eps")
        torch.cuda.synchronize()
        res, other = (buf, obuf) if in_place else (obuf, buf)
        assert torch.all(res[:4] == guard) and torch.all(res[-4:] == guard)
        if in_place:
            assert torch.all(other == guard)
        else:
            assert np.array_equal(other[4:-4].cpu().numpy().view(np.int32), pred.reshape(-1).view(np.int32))     # pred is left alone
        return res[4:-4].cpu().numpy().reshape(B, per)

    for in_place in (True, False):
        got = run(T_ROWS, in_place)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (kind, per, in_place)
    assert np.array_equal(x_d.cpu().numpy().view(np.int32), x.view(np.int32))
    # t is clamped into [0, timesteps)
    assert np.array_equal(run((-3, 517, 2000), True).view(np.int32), want.view(np.int32))


# ---- dm3d_objective_loss_grad -------------------------------------------------------------------------------------------------------
def _loss_call(dev, pred, noise, x0, rows, inv, with_dpred=True):
    from dm3d_amd import _lib
    B, per = pred.shape
    coef = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).to(dev)
    dpred = torch.full_like(pred, float("nan")) if with_dpred else None
    partials = torch.full((B * _lib.LOSS_PARTIAL_BLOCKS,), float("nan"), dtype=torch.float64, device=dev)
    loss_rows = torch.full((B,), float("nan"), dtype=torch.float64, device=dev)
    loss = torch.full((1,), float("nan"), dtype=torch.float64, device=dev)      # written, not accumulated into
    d = _lib.LossDesc()
    d.pred, d.noise, d.x0, d.coef = pred.data_ptr(), noise.data_ptr(), x0.data_ptr(), coef.data_ptr()
    d.dpred = None if dpred is None else dpred.data_ptr()
    d.partials, d.loss_rows, d.loss = partials.data_ptr(), loss_rows.data_ptr(), loss.data_ptr()
    d.batch, d.per_sample, d.inv_divisor = B, per, inv
    _lib.check(_lib.lib().dm3d_objective_loss_grad(C.byref(d), _st()), "objective_loss_grad")
    torch.cuda.synchronize()
    return dpred, loss_rows, loss


@pytest.mark.parametrize("per", SIZES)
def test_objective_loss_grad_against_restatements(dev, per):
    """Rows for eps, v and x0 with distinct (min-SNR) weights.  dpred bitwise; the losses within 1e-10 relative of a float64 sum of the
    float32 d squared in float64 (only the order of the sum differs: n 2^-53 = 4e-11 at n = 393 252); two runs give the same bits; rows
    (1, 0, 1) give dm3d_mse_loss_grad's dpred bitwise."""
    import dm3d_amd
    from dm3d_amd import _lib
    from dm3d_amd.diffusion import objective_rows
    B, T, inv = 3, 1000, 1.0 / (4 * 2 * 4 ** 4)
    ab = dm3d_amd.Betas(T).alpha_bar
    rows = np.concatenate([objective_rows(ab, [t], kind, "min_snr", 5.0) for t, kind in zip(T_ROWS, ("eps", "v", "x0"))])
    assert len(set(rows[:, 2].tolist())) == 3 and rows[1, 0] != 0 and rows[1, 1] != 0
    rng = np.random.default_rng(per + 1)
    pred, noise, x0 = (rng.standard_normal((B, per)).astype(np.float32) for _ in range(3))
    d32 = np.stack([pred[b] - (rows[b, 0] * noise[b] + rows[b, 1] * x0[b]) for b in range(B)])       # float32: mul, mul, add, sub
    scale = [np.float32(2.0 * inv * float(rows[b, 2])) for b in range(B)]
    want_g = np.stack([d32[b] * scale[b] for b in range(B)])
    assert d32.dtype == np.float32 and want_g.dtype == np.float32
    want_rows = np.array([float(rows[b, 2]) * inv * float(np.sum(d32[b].astype(np.float64) ** 2)) for b in range(B)])
    p_d, z_d, c_d = (torch.from_numpy(a).to(dev) for a in (pred, noise, x0))
    g1, r1, l1 = _loss_call(dev, p_d, z_d, c_d, rows, inv)
    g2, r2, l2 = _loss_call(dev, p_d, z_d, c_d, rows, inv)
    assert np.array_equal(g1.cpu().numpy().view(np.int32), want_g.view(np.int32))
    rel = np.abs(r1.cpu().numpy() - want_rows) / want_rows
    rel_total = abs(float(l1.item()) - float(want_rows.sum())) / float(want_rows.sum())
    print(f"per_sample {per}: loss_rows rel err {rel.max():.2e}, loss rel err {rel_total:.2e}")
    assert rel.max() < 1e-10 and rel_total < 1e-10
    assert float(l1.item()) == float(r1[0].item()) + float(r1[1].item()) + float(r1[2].item())         # in index order
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(r1), _bits(r2)) and torch.equal(_bits(l1), _bits(l2))
    # without dpred the losses are the same bits
    _, r3, l3 = _loss_call(dev, p_d, z_d, c_d, rows, inv, with_dpred=False)
    assert torch.equal(_bits(r1), _bits(r3)) and torch.equal(_bits(l1), _bits(l3))
    # the plain objective: dm3d_mse_loss_grad on the same buffers
    plain = np.tile(np.array([1, 0, 1, 0], np.float32), (B, 1))
    g4, r4, l4 = _loss_call(dev, p_d, z_d, c_d, plain, inv)
    g5, l5 = torch.empty_like(p_d), torch.zeros(1, dtype=torch.float64, device=dev)
    _lib.check(_lib.lib().dm3d_mse_loss_grad(p_d.data_ptr(), z_d.data_ptr(), p_d.numel(), inv, l5.data_ptr(), g5.data_ptr(), _st()), "mse")
    torch.cuda.synchronize()
    assert torch.equal(_bits(g4), _bits(g5))
    assert abs(float(l4.item()) - float(l5.item())) / float(l5.item()) < 1e-10


# ---- chains -------------------------------------------------------------------------------------------------------------------------
def _as_eps(kind, f, ab, ctx):
    """The oracle network's output under ``ctx`` read as ``kind`` and converted to eps, as the converting chain does."""
    return lambda x, t: cr.eps64(kind, x, f(x, t, ctx), float(ab[t]))


IDS = torch.tensor([[[1]], [[0]]])
SHAPE = (2, 8, 8, 8, 4)


@pytest.mark.parametrize("sampler", ["ddim", "dpmpp", "ddpm"])
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_chain_matches_float64(dev, kind, sampler):
    """8^3 x 4ch, T = 20, S = 5, B = 2 with one context id per volume (the DDPM chain: all 20 steps, injected noise).  At T = 20
    alpha_bar stays above 0.8: the x0 estimate divides by no small sqrt(alpha_bar)."""
    T, S = 20, 5
    m, W = cr.cond_model(T, 2, prediction=kind)
    g = torch.Generator().manual_seed(21)
    x_T = torch.randn(SHAPE, generator=g)
    b = cr.oracle_betas(T)
    ab = b.alpha_bar.double()
    net = _as_eps(kind, cr.oracle(W), ab, IDS)
    assert float(b.alpha_bar.min()) > 0.8
    if sampler == "ddpm":
        noise = torch.randn((T,) + SHAPE, generator=g)
        got = m.generate(SHAPE, context_value=IDS, x_T=x_T, noise=noise).cpu()
        ref = cr.chain64(net, ab, list(range(T)), x_T, "ddpm", noise=noise, betas=b)
    else:
        got = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler=sampler, num_steps=S).cpu()
        ref = cr.chain64(net, ab, cr.schedule(T, S), x_T, sampler)
    err = float((got.double() - ref).abs().max())
    print(f"{kind} model, {sampler} chain: max abs difference {err:.2e} (max |x| {float(ref.abs().max()):.3f})")
    assert torch.isfinite(got).all() and err < CHAIN_BAR


def test_guided_v_chain_matches_float64(dev):
    """Guidance (w = 3, phi = 0.7) acts on the converted eps of both halves of the plan."""
    T, S = 20, 5
    m, W = cr.cond_model(T, 2, prediction="v")
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(22))
    neg = torch.tensor([[[0]], [[1]]])
    got = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="ddim", num_steps=S, guidance_scale=3.0, guidance_rescale=0.7,
                     negative_context=neg).cpu()
    f, ab = cr.oracle(W), cr.oracle_alpha_bar(T).double()
    pos, neg_eps = _as_eps("v", f, ab, IDS), _as_eps("v", f, ab, neg)
    ref = cr.chain64(lambda x, t: cr.guide64(pos(x, t), neg_eps(x, t), 3.0, 0.7), ab, cr.schedule(T, S), x_T, "ddim")
    err = float((got.double() - ref).abs().max())
    print(f"guided v model, ddim chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR
    eager = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="ddim", num_steps=S, guidance_scale=3.0, guidance_rescale=0.7,
                       negative_context=neg, use_graph=False).cpu()
    assert torch.equal(eager, got)


def test_graph_equals_eager_and_kinds_do_not_leak(dev):
    """A seeded v chain is bitwise the same through the graph and eagerly; an eps model and a v model on the same weights, run
    alternately, each equal their own fresh model's result bitwise; the converting step's graph has a kind of its own and the eps
    model's kinds are what they were."""
    T = 20
    v, W = cr.cond_model(T, 2, prediction="v")
    e, _ = cr.cond_model(T, 2, W=W)
    calls = [dict(sampler="ddim", num_steps=5, eta=0.5), dict(sampler="dpmpp", num_steps=5), dict()]
    for kw in calls:
        a = v.generate(SHAPE, context_value=IDS, seed=5, use_graph=True, **kw)
        b = v.generate(SHAPE, context_value=IDS, seed=5, use_graph=False, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.isfinite(a).all(), kw
    fresh = {}
    for name, kind in (("v", "v"), ("eps", "eps")):
        fm, _ = cr.cond_model(T, 2, W=W, prediction=kind)
        fresh[name] = [fm.generate(SHAPE, context_value=IDS, seed=5, **kw).clone() for kw in calls]
    for _ in range(2):
        for i, kw in enumerate(calls):
            assert torch.equal(e.generate(SHAPE, context_value=IDS, seed=5, **kw), fresh["eps"][i]), kw
            assert torch.equal(v.generate(SHAPE, context_value=IDS, seed=5, **kw), fresh["v"][i]), kw
            assert not torch.equal(fresh["v"][i], fresh["eps"][i])
    assert {k[1] for k in v._graphs} == {"ddim+pred", "dpmpp+pred", "ddpm+pred"}
    assert {k[1] for k in e._graphs} == {"ddim", "dpmpp", "ddpm"}
    # inversion goes through the same hook
    x0 = torch.rand(SHAPE, generator=torch.Generator().manual_seed(5)) * 2 - 1
    assert torch.equal(v.invert(x0, 1, num_steps=5), v.invert(x0, 1, num_steps=5, use_graph=False))
    assert not torch.equal(v.invert(x0, 1, num_steps=5), e.invert(x0, 1, num_steps=5))


def test_predict_eps_then_ddim_step_is_one_step_of_the_chain(dev):
    T, S = 20, 5
    m, W = cr.cond_model(T, 2, prediction="v")
    sched = cr.schedule(T, S)
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(23))
    want = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="ddim", num_steps=S, steps=1)
    t = torch.tensor([sched[-1]] * 2)
    pred = m.network([x_T.to(dev), t, IDS])
    eps = m.predict_eps(x_T, pred, sched[-1])
    got = m.ddim_step(x_T, eps, sched[-1], sched[-2])
    assert float((got - want).abs().max()) < CHAIN_BAR
    ab = cr.oracle_alpha_bar(T).double()
    ref = cr.chain64(_as_eps("v", cr.oracle(W), ab, IDS), ab, sched, x_T, "ddim", steps=1)
    assert float((got.cpu().double() - ref).abs().max()) < CHAIN_BAR
    # out of place: the inputs are left alone; per-volume t; an eps model's table is the identity
    assert torch.equal(m.predict_eps(x_T, pred, [sched[-1], sched[-1]]), eps)
    plain, _ = cr.cond_model(T, 2, W=W)
    assert torch.equal(plain.predict_eps(x_T, pred, 7), pred)


# ---- training -----------------------------------------------------------------------------------------------------------------------
def _ref_loss_and_grads(W64, ocfg, ob, lat, t, noise, ctx, gbs, lc, kind, weighting, gamma=5.0, stats=None):
    """torch.autograd over the oracle's training forward with the loss written out in float64: per sample
    w * mean_c sum_dhw (pred - target)^2 / (gbs lc^4), target and w from alpha_bar[t]."""
    from oracle import ref_torch as rt, ref_train as ot
    Wg = {k: (v.clone().requires_grad_(True) if ot.is_trainable(k) else v) for k, v in W64.items()}
    noisy = rt.q_sample(ob, lat, t, noise).to(lat.dtype)
    pred = ot.unet_forward_train(Wg, ocfg, noisy, t, ctx, stats=stats)
    ab = ob.alpha_bar.double()[t].reshape(-1, 1, 1, 1, 1)
    a, s = ab.sqrt(), (1 - ab).sqrt()
    target = {"eps": noise, "v": a * noise - s * lat, "x0": lat}[kind]
    snr = (ab / (1 - ab)).reshape(-1)
    w = torch.ones_like(snr)
    if weighting == "min_snr":
        clipped = snr.clamp(max=gamma)
        w = {"eps": clipped / snr, "v": clipped / (snr + 1), "x0": clipped}[kind]
    per = w * ((pred - target) ** 2).mean(-1).sum((1, 2, 3)) / (gbs * lc ** 4 * 1.0)
    loss = per.sum()
    names = [k for k in Wg if Wg[k].requires_grad]
    grads = torch.autograd.grad(loss, [Wg[k] for k in names], allow_unused=True)
    return loss.detach(), {k: (g if g is not None else torch.zeros_like(Wg[k])) for k, g in zip(names, grads)}, per.detach(), w


def _compare_grads(got, ref, tol, label=""):
    """tests/test_gpu_train.py's rule: per tensor, max |g - ref| <= tol * max(|ref| of that tensor, 1e-3 * the largest gradient entry)."""
    gmax = max(float(v.abs().max()) for v in ref.values())
    worst = ("", 0.0)
    for name, r in ref.items():
        scale = max(float(r.abs().max()), 1e-3 * gmax)
        e = float((torch.as_tensor(got[name]).double() - r.double()).abs().max()) / scale
        if e > worst[1]:
            worst = (name, e)
    print(f"{label} worst gradient error {worst[1]:.3e} at {worst[0]} (largest gradient entry {gmax:.3e})")
    assert worst[1] < tol, worst


def test_v_min_snr_loss_and_all_gradients(dev):
    """8^3 x 4ch, B = 2, T = 50, t = (3, 40): gamma = 5 clips at t = 3 and not at t = 40.  Loss within 1e-5 relative, every gradient
    within 1e-4 (tests/test_gpu_train.py's bars); the per-sample losses sum to the loss."""
    import dm3d_amd
    from dm3d_amd.betas import BETAS_FIELDS
    from dm3d_amd.diffusion import objective_rows
    from dm3d_amd.train import Trainer
    from oracle import ref_torch as rt
    cfg = dm3d_amd.UNetConfig(img_size=8, img_channels=4)
    W = dm3d_amd.synthetic_weights(cfg, seed=0)
    g = torch.Generator().manual_seed(0)
    lat, noise = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    t, T, gbs, lc = torch.tensor([3, 40]), 50, 2, 4
    ocfg, ob = rt.UNetConfig(img_size=8, img_channels=4), rt.Betas(T)
    W64 = {k: torch.from_numpy(v).double() for k, v in W.items()}
    loss_ref, grads_ref, per_ref, w_ref = _ref_loss_and_grads(W64, ocfg, ob, lat.double(), t, noise.double(), IDS, gbs, lc, "v", "min_snr")
    snr = ob.alpha_bar.double()[t] / (1 - ob.alpha_bar.double()[t])
    assert float(snr[0]) > 5.0 > float(snr[1])
    b = dm3d_amd.Betas(T)
    rows = objective_rows(b.alpha_bar, t, "v", "min_snr", 5.0)
    assert np.allclose(rows[:, 2], w_ref.numpy(), rtol=1e-6)
    tr = Trainer(cfg, W, dev)
    tab = b.device_tables(dev)
    betas = (tab[BETAS_FIELDS.index("sqrt_alpha_bar")], tab[BETAS_FIELDS.index("sqrt_one_minus_alpha_bar")])
    loss, _ = tr.loss_and_grad(lat.to(dev), t, noise.to(dev), IDS.reshape(-1).numpy(), betas, T, gbs, lc, objective=rows)
    torch.cuda.synchronize()
    lerr = abs(float(loss.item()) - float(loss_ref)) / float(loss_ref)
    per = tr.sample_loss.cpu()
    perr = float(((per - per_ref).abs() / per_ref).max())
    print(f"loss {float(loss.item()):.8f} vs autograd {float(loss_ref):.8f} (rel {lerr:.2e}); per-sample rel {perr:.2e}")
    assert lerr < 1e-5 and perr < 1e-5
    assert per.dtype == torch.float64 and tuple(per.shape) == (2,) and float(per[0]) + float(per[1]) == float(loss.item())
    got = {k: torch.from_numpy(v) for k, v in tr.grads().items()}
    assert set(got) == set(grads_ref)
    _compare_grads(got, grads_ref, 1e-4, "v + min-SNR, all gradients:")
    # without an objective the step is the plain MSE launch it was, and keeps no per-sample loss
    tr.loss_and_grad(lat.to(dev), t, noise.to(dev), IDS.reshape(-1).numpy(), betas, T, gbs, lc)
    assert tr.sample_loss is None


@pytest.mark.parametrize("kind,weighting", [("x0", None), ("eps", "min_snr")])
def test_train_step_public_api(dev, kind, weighting):
    """One public train_step: the loss, and the weights after Adam against oracle.ref_train.adam_step on the autograd gradients,
    compared as tests/test_gpu_train.py::test_train_step_public_api compares them.  That test allows 3e-5 after three steps of 2e-4
    (5 % of the distance moved); one step of 2e-4 is held to the same share, 1e-5."""
    import dm3d_amd
    from oracle import ref_torch as rt, ref_train as ot
    T, B, lc, lr = 50, 2, 4, 2e-4
    m, W = cr.cond_model(T, B, W=cr.weights(seed=1), prediction=kind)
    m.compile(loss="mse_sum", optimizer=SimpleNamespace(learning_rate=lr), loss_weighting=weighting)
    g = torch.Generator().manual_seed(5)
    lat, noise = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    t = torch.tensor([3, 40])
    ocfg, ob = rt.UNetConfig(img_size=8, img_channels=4), rt.Betas(T)
    Wd = {k: torch.from_numpy(v).double() for k, v in W.items()}
    lref, gref, per_ref, _ = _ref_loss_and_grads(Wd, ocfg, ob, lat.double(), t, noise.double(), IDS, B, lc, kind, weighting)
    zeros = {k: torch.zeros_like(v) for k, v in gref.items()}
    Wn, mom, _ = ot.adam_step(Wd, gref, zeros, zeros, 1, lr)
    out = m.train_step((None, None, IDS), latents=lat, t=t, noise=noise)
    assert set(out) == {"loss"}
    print(f"{kind} / {weighting}: loss {out['loss']:.8f} vs autograd {float(lref):.8f}")
    assert np.allclose(out["loss"], float(lref), rtol=2e-5)
    per = m.trainer.sample_loss.cpu()
    assert float(((per - per_ref).abs() / per_ref).max()) < 2e-5
    st = m.network.state_dict()
    worst = 0.0
    for k in mom:
        sel = mom[k].abs() > 1e-3 * mom[k].abs().max().clamp_min(1e-30)
        if sel.any():
            worst = max(worst, float((torch.from_numpy(st[k]).double() - Wn[k]).abs()[sel].max()))
    print(f"after one step: max |w - w_ref| = {worst:.3e} (one step of {lr})")
    assert worst < 1e-5
