"""GPU tier of the DPM-Solver++(2M) sampler (dm3d_dpm_update, DiffusionModel.dpm_step, generate / edit / sampler with "dpmpp").

The float64 reference is this file's own restatement of the update (Lu et al. 2022, Algorithm 2, in the data-prediction form) with eps
from the CPU oracle (oracle.ref_torch.unet_forward) and alpha_bar from the oracle's float32 Betas table, the table the kernels read.
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
CHAIN_BAR = 2e-3        # the existing chain tests' bar (values in [-1, 1] + noise)
KERNEL_BAR = 2e-6       # the DDIM kernel test's bar, scaled below by the coefficient mass of the row


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return torch.device("cuda:0")


def _args(T, bs=1):
    return SimpleNamespace(timesteps=T, num_gpus=1, kernel_resize=False, bs=bs)


def _schedule(T, S):
    return [T - 1] if S == 1 else [int(math.floor(i * (T - 1) / (S - 1) + 0.5)) for i in range(S)]


def _cond_model(T, B, size=8, C=4, W=None, **kw):
    import dm3d_amd
    from dm3d_amd.networks import conditional_dm3d as cdm
    cfg = dm3d_amd.UNetConfig(img_size=size, img_channels=C)
    W = dm3d_amd.synthetic_weights(cfg, seed=0) if W is None else W
    return cdm.DiffusionModel(size, 1024, C, None, _args(T, B), weights=W, **kw), W


def _oracle(W, size, C, conditional=True):
    from oracle import ref_torch as rt
    ocfg = rt.UNetConfig(img_size=size, img_channels=C, conditional=conditional)
    Wt = {k: torch.from_numpy(v) for k, v in W.items()}
    return lambda x, t, ctx=None: rt.unet_forward(Wt, ocfg, x.float(), torch.full((x.shape[0],), int(t), dtype=torch.int64), ctx)


def _row64(ab, s, t, p):
    """(c_x, c_0, c_1) of the step from timestep s to t (t < 0: clean) in float64; p: the timestep of the step before (p < 0: first order).
    alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma), h = lambda_t - lambda_s, r = (lambda_s - lambda_p) / h."""
    if t < 0:
        return 0.0, 1.0, 0.0
    al = lambda i: math.sqrt(float(ab[i]))
    sg = lambda i: math.sqrt(1.0 - float(ab[i]))
    lam = lambda i: math.log(al(i) / sg(i))
    h = lam(t) - lam(s)
    A = al(t) * (1.0 - math.exp(-h))
    if p < 0:
        return sg(t) / sg(s), A, 0.0
    r = (lam(s) - lam(p)) / h
    return sg(t) / sg(s), A * (1.0 + 1.0 / (2.0 * r)), -A / (2.0 * r)


def _dpm64(x, eps, ab, s, t, p=-1, hist=None, clip=True):
    """One step in float64: (x at t, the x0 estimate)."""
    x, eps, a = x.double(), eps.double(), float(ab[s])
    x0 = (x - math.sqrt(1 - a) * eps) / math.sqrt(a)
    if clip:
        x0 = x0.clamp(-1, 1)
    c_x, c_0, c_1 = _row64(ab, s, t, p)
    out = c_x * x + c_0 * x0
    return (out + c_1 * hist.double() if c_1 != 0 else out), x0


def _prev(sched, order=2, lower_order_final=True):
    """The order rule: p of the step from sched[i] (the first step, the step to clean and, with lower_order_final, the step into
    sched[0] are first order)."""
    n = len(sched)
    prev = list(sched[1:]) + [-1]
    if order == 1:
        prev = [-1] * n
    if lower_order_final and n > 1:
        prev[1] = -1
    return prev


def _chain64(eps_fn, ab, sched, x_start, order=2, lower_order_final=True, clip=True, blend=None, steps=None):
    """The whole chain with float64 bookkeeping: steps from sched[-1] down to sched[0], then clean; ``blend(i, x)`` (edit chains) follows
    the step from sched[i].  The history is the model's own x0 estimate, before any blend."""
    x, hist, prev = x_start.double(), None, _prev(sched, order, lower_order_final)
    for k, i in enumerate(range(len(sched) - 1, -1, -1)):
        if steps is not None and k == steps:
            break
        x, hist = _dpm64(x, eps_fn(x, sched[i]), ab, sched[i], sched[i - 1] if i > 0 else -1, prev[i], hist, clip)
        if blend is not None:
            x = blend(i, x)
    return x


def _known64(x0, ab, level, z):
    if level < 0:
        return x0.double()
    a = float(ab[level])
    return math.sqrt(a) * x0.double() + math.sqrt(1 - a) * z.double()


CASES = [  # (t, t_prev, t_before or None), one entry per sample
    ([400, 300, 20], [380, 150, -1], None),                      # first order; sample 2 steps to clean
    ([400, 300, 20], [380, 150, -1], [420, 999, 25]),            # second order; sample 2 to clean (first order whatever the history)
    ([200, 50, 5], [100, 49, 0], [300, 51, 900]),                # second order: a wide, a unit and a tiny step after a far history
    ([5, 1, 0], [-1, 0, -1], None),
]


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("clip", [True, False])
def test_kernel_matches_float64_restatement(dev, clip, B):
    """dpm_step (mode 0) on random x / eps / x0_prev with per-sample t: first-order, second-order and to-clean rows.  The bar of x_next
    is the DDIM kernel test's 2e-6 times the row's coefficient mass max(1, |c_x| + |c_0| + |c_1|); the x0 estimate is the linear map
    (x - sigma eps) / alpha of the inputs, so its bar takes that map's mass max(1, (1 + sigma) / alpha).  Values stay below 20."""
    from oracle import ref_torch as rt
    T = 1000
    m, _ = _cond_model(T, B)
    ab = rt.Betas(T).alpha_bar.double()
    g = torch.Generator().manual_seed(29 + B)
    shape = (B, 8, 8, 8, 4)
    x, e, h = (torch.randn(shape, generator=g) for _ in range(3))
    cases = CASES + ([([999, 998, 700], [950, 997, 650], None), ([990, 800, 700], [900, 600, 100], [999, 900, 999])] if clip else [])
    for t, tp, tb in cases:
        t, tp = t[:B], tp[:B]
        tb = None if tb is None else tb[:B]
        second = tb is not None
        if second:
            got, x0 = m.dpm_step(x, e, torch.tensor(t), torch.tensor(tp), h, torch.tensor(tb), clip_x0=clip)
        else:
            got, x0 = m.dpm_step(x, e, torch.tensor(t), torch.tensor(tp), clip_x0=clip)
        got, x0 = got.cpu(), x0.cpu()
        for b in range(B):
            p = tb[b] if second else -1
            ref, ref0 = _dpm64(x[b], e[b], ab, t[b], tp[b], p, h[b], clip)
            assert float(ref.abs().max()) < 20 and float(ref0.abs().max()) < 20             # O(1) values: the bars are absolute
            a = float(ab[t[b]])
            bar = KERNEL_BAR * max(1.0, sum(abs(c) for c in _row64(ab, t[b], tp[b], p)))
            bar0 = KERNEL_BAR * max(1.0, (1 + math.sqrt(1 - a)) / math.sqrt(a))
            err, err0 = float((got[b].double() - ref).abs().max()), float((x0[b].double() - ref0).abs().max())
            print(f"B={B} clip={clip} t={t[b]} -> {tp[b]} (before {p}): x_next err {err:.2e} (bar {bar:.2e}), x0 err {err0:.2e} (bar {bar0:.2e})")
            assert err < bar and err0 < bar0, (t, tp, tb, b)
            if tp[b] < 0:
                assert torch.equal(got[b], x0[b])                                           # the clean row hands on x0 bitwise


def test_order_one_step_is_ddim_eta0_and_inputs_stay(dev):
    """A first-order row is the DDIM step at eta = 0 wherever the x0 estimate is not clipped (where it is, DDIM carries the model's eps
    on and this solver the eps the clipped estimate implies: x enters the update, eps does not)."""
    from oracle import ref_torch as rt
    T, B = 1000, 3
    m, _ = _cond_model(T, B)
    ab = rt.Betas(T).alpha_bar.double()
    g = torch.Generator().manual_seed(7)
    shape = (B, 8, 8, 8, 4)
    x, e, h = (torch.randn(shape, generator=g).cuda() for _ in range(3))
    keep = [v.clone() for v in (x, e, h)]
    for clip in (False, True):
        for t, tp in (([400, 300, 20], [380, 150, -1]), ([350, 100, 1], [349, 0, 0])):
            got, x0 = m.dpm_step(x, e, torch.tensor(t), torch.tensor(tp), clip_x0=clip)
            ddim = m.ddim_step(x, e, torch.tensor(t), torch.tensor(tp), 0.0, clip_x0=clip)
            inside = x0.abs() < 1 if clip else torch.ones_like(x0, dtype=torch.bool)
            assert 0.2 < float(inside.float().mean()) and float(got.abs().max()) < 20
            for b in range(B):
                bar = KERNEL_BAR * max(1.0, sum(abs(c) for c in _row64(ab, t[b], tp[b], -1)))
                err = float((got[b] - ddim[b])[inside[b]].abs().max())
                print(f"clip={clip} t={t[b]} -> {tp[b]}: |dpm_step - ddim_step| {err:.2e} (bar {bar:.2e})")
                assert err < bar, (clip, t[b], tp[b])
    m.dpm_step(x, e, 300, 150, h, 400)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((x, e, h), keep))                          # mode 0 leaves x, eps and the history alone


def test_nan_reaches_its_element_only(dev):
    m, _ = _cond_model(1000, 2)
    g = torch.Generator().manual_seed(8)
    shape = (2, 8, 8, 8, 4)
    x, e, h = (torch.randn(shape, generator=g) for _ in range(3))
    e_nan = e.clone()
    e_nan[0, 1, 2, 3, 1] = float("nan")
    for clip in (True, False):
        for hist in ((), (h, 520)):
            out, x0 = m.dpm_step(x, e_nan, 500, 480, *hist, clip_x0=clip)
            for v in (out.cpu(), x0.cpu()):
                assert torch.isnan(v[0, 1, 2, 3, 1]) and int(torch.isnan(v).sum()) == 1
    # a NaN in the history reaches a second-order row only
    h_nan = h.clone()
    h_nan[1, 0, 0, 0, 0] = float("nan")
    out, x0 = m.dpm_step(x, e, 500, 480, h_nan, 520)
    assert torch.isnan(out[1, 0, 0, 0, 0]) and int(torch.isnan(out).sum()) == 1 and not torch.isnan(x0).any()
    out, x0 = m.dpm_step(x, e, 500, -1, h_nan, 520)                                         # to clean: first order, the history unread
    assert not torch.isnan(out).any() and torch.equal(out, x0)


def test_stale_history_never_reaches_a_chain(dev):
    """The first row of a chain has c_1 = 0 and does not read plan.dpm_hist: a buffer full of NaN before reset() changes no bit."""
    T, B = 20, 2
    m, _ = _cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    for use_graph in (True, False):
        for kw in (dict(num_steps=5), dict(num_steps=2), dict(num_steps=1), dict(num_steps=6, lower_order_final=False)):
            want = m.generate(shape, context_value=1, seed=3, sampler="dpmpp", use_graph=use_graph, **kw)
            smp = m.sampler(shape, 1, seed=3, kind="dpmpp", use_graph=use_graph, **kw)
            smp.plan.dpm_hist.fill_(float("nan"))
            smp.reset()
            for _ in range(smp.n_steps):
                smp.step()
            torch.cuda.synchronize()
            assert torch.isfinite(smp.x).all() and torch.equal(smp.x, want), (use_graph, kw)
            with pytest.raises(RuntimeError):
                smp.step()


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("conditional", [True, False])
def test_chain_matches_float64(dev, conditional, clip, order):
    """8^3 x 4ch, T = 20, S = 5, B = 2 (conditional: one context id per volume)."""
    import dm3d_amd
    from dm3d_amd.networks import dm3d
    from oracle import ref_torch as rt
    T, S, B = 20, 5, 2
    shape = (B, 8, 8, 8, 4)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(21))
    kw = dict(x_T=x_T, sampler="dpmpp", num_steps=S, clip_x0=clip, solver_order=order)
    if conditional:
        m, W = _cond_model(T, B)
        ids = torch.tensor([[[1]], [[0]]])
        got = m.generate(shape, context_value=ids, **kw).cpu()
        f = _oracle(W, 8, 4)
        eps_fn = lambda x, t: f(x, t, ids)
    else:
        cfg = dm3d_amd.UNetConfig(img_size=8, img_channels=4, conditional=False)
        W = dm3d_amd.synthetic_weights(cfg, seed=0)
        m = dm3d.DiffusionModel(8, 1024, 4, None, _args(T, B), weights=W)
        got = m.generate(shape, **kw).cpu()
        eps_fn = _oracle(W, 8, 4, conditional=False)
    ab = rt.Betas(T).alpha_bar.double()
    ref = _chain64(eps_fn, ab, _schedule(T, S), x_T, order, True, clip)
    err = float((got.double() - ref).abs().max())
    print(f"dpmpp chain conditional={conditional} clip={clip} order={order}: max abs difference {err:.2e}, max |x| {float(ref.abs().max()):.3f}")
    assert err < CHAIN_BAR
    if order == 2:                                      # the second-order rows do something: the order-1 chain differs
        assert not torch.equal(got, m.generate(shape, **dict(kw, solver_order=1), **(dict(context_value=ids) if conditional else {})).cpu())
    elif not clip:                                      # order 1 without the clip is the DDIM chain at eta = 0, in another arithmetic order
        ddim = m.generate(shape, x_T=x_T, sampler="ddim", num_steps=S, clip_x0=False, **(dict(context_value=ids) if conditional else {})).cpu()
        assert float((got - ddim).abs().max()) < 2 * CHAIN_BAR           # each lies within the bar of the one float64 chain


def test_graph_equals_eager_repeats_and_serves_every_schedule(dev):
    """Graph replay equals eager bitwise, two calls under one seed are bitwise equal, and a second schedule, order or lower_order_final
    on the same plan reuses the captured graph (the count does not grow) and still matches its float64 chain."""
    from oracle import ref_torch as rt
    T, B = 20, 2
    m, W = _cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    ids = torch.tensor([[[1]], [[0]]])
    f = _oracle(W, 8, 4)
    ab = rt.Betas(T).alpha_bar.double()
    counts = []
    runs = [dict(num_steps=5), dict(num_steps=8), dict(timesteps=[0, 3, 11, 19], clip_x0=False), dict(num_steps=20),
            dict(num_steps=7, lower_order_final=False), dict(num_steps=6, solver_order=1)]
    for kw in runs:
        a = m.generate(shape, context_value=ids, seed=5, sampler="dpmpp", use_graph=True, **kw)
        counts.append(len(m._graphs))
        b = m.generate(shape, context_value=ids, seed=5, sampler="dpmpp", use_graph=False, **kw)
        c = m.generate(shape, context_value=ids, seed=5, sampler="dpmpp", use_graph=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.isfinite(a).all(), kw
        # the chain draws only its x_T: take it from a zero-step chain under the seed
        x_T = m.generate(shape, context_value=ids, seed=5, sampler="dpmpp", steps=0, **kw).cpu()
        sched = kw.get("timesteps") or _schedule(T, kw["num_steps"])
        ref = _chain64(lambda x, t: f(x, t, ids), ab, sched, x_T, kw.get("solver_order", 2), kw.get("lower_order_final", True),
                       kw.get("clip_x0", True))
        err = float((a.cpu().double() - ref).abs().max())
        print(f"dpmpp {kw}: max abs difference {err:.2e}")
        assert err < CHAIN_BAR, kw
    assert counts == [counts[0]] * len(runs) and ("dpmpp" in {k[1] for k in m._graphs})
    assert not torch.equal(m.generate(shape, context_value=ids, seed=6, sampler="dpmpp", num_steps=5),
                           m.generate(shape, context_value=ids, seed=5, sampler="dpmpp", num_steps=5))


def test_kinds_do_not_leak(dev):
    """A "dpmpp" call after a "ddim" call on the same plan, and the reverse, leaves each bitwise as it is alone (on a fresh model); so
    for the DDPM chain."""
    T, B = 20, 2
    shape = (B, 8, 8, 8, 4)
    calls = {"dpmpp": dict(sampler="dpmpp", num_steps=5), "ddim": dict(sampler="ddim", num_steps=5, eta=0.5), "ddpm": {}}
    alone = {}
    for k, kw in calls.items():
        fresh, _ = _cond_model(T, B)
        alone[k] = fresh.generate(shape, context_value=0, seed=5, **kw)
    m, _ = _cond_model(T, B)
    for k in ("ddim", "dpmpp", "ddim", "ddpm", "dpmpp", "ddpm", "ddim"):
        got = m.generate(shape, context_value=0, seed=5, **calls[k])
        torch.cuda.synchronize()
        assert torch.equal(got, alone[k]), k
    assert {"dpmpp", "ddim", "ddpm"} <= {k[1] for k in m._graphs}


def _half_mask(B):
    """Regenerate the lower half of D, keep the upper half, with a fractional slab at the boundary (a 16^3 mask over 8^3 latents)."""
    m = torch.zeros((B, 16, 16, 16))
    m[:, :8] = 1.0
    m[:, 8:10] = 0.3
    m[:, 8:10, :, :4] = 0.8
    return m


@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_edit_chain_matches_float64(dev, strength):
    """edit(sampler="dpmpp"), 8^3 x 4ch, T = 20, S = 5, B = 2, a half mask with a fractional slab, injected known_noise: the blend
    follows every update, the history stays unblended, kept voxels are x0 bitwise; strength 0.6 keeps 3 steps and starts first order
    from q_sample(x0, sched[2])."""
    from dm3d_amd.diffusion import edit_steps, latent_mask
    from oracle import ref_torch as rt
    T, S, B = 20, 5, 2
    m, W = _cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    g = torch.Generator().manual_seed(41)
    x0 = torch.rand(shape, generator=g) * 2 - 1
    n = edit_steps(strength, S)
    sched = _schedule(T, S)[:n]
    assert n == (5 if strength == 1.0 else 3)
    known_noise = torch.randn((n + 1,) + shape, generator=g)
    ids = torch.tensor([[[1]], [[0]]])
    mask = _half_mask(B)
    ab = rt.Betas(T).alpha_bar.double()
    kw = dict(mask=mask, strength=strength, seed=13, sampler="dpmpp", num_steps=S)
    if n == S:
        x_start = m.edit(x0, ids, steps=0, **kw).cpu()                    # generate()'s x_T under the seed
    else:
        x_start = _known64(x0, ab, sched[-1], known_noise[n])
    got = m.edit(x0, ids, known_noise=known_noise, **kw).cpu()
    f = _oracle(W, 8, 4)
    w = (1 - latent_mask(mask, shape)).double().unsqueeze(-1)
    blend = lambda i, x: w * _known64(x0, ab, sched[i - 1] if i > 0 else -1, known_noise[i]) + (1 - w) * x
    ref = _chain64(lambda x, t: f(x, t, ids), ab, sched, x_start, blend=blend)
    err = float((got.double() - ref).abs().max())
    print(f"dpmpp edit chain strength={strength}: max abs difference {err:.2e}")
    assert err < CHAIN_BAR
    kept = (w == 1).expand(shape)
    regen = (w == 0).expand(shape)
    assert torch.equal(got[kept], x0[kept])                               # the kept region is x0 bitwise
    assert float((got[regen] - x0[regen]).abs().mean()) > 1e-2            # the regenerated one is new
    # seeded runs repeat, through the graph and eagerly, and all-regenerate at strength 1 is generate()
    a, b = m.edit(x0, ids, **kw), m.edit(x0, ids, use_graph=False, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a.cpu()[kept], x0[kept])
    if n == S:
        want = m.generate(shape, context_value=ids, seed=13, sampler="dpmpp", num_steps=S)
        assert torch.equal(m.edit(x0, ids, seed=13, sampler="dpmpp", num_steps=S), want)
    assert "dpmpp-edit" in {k[1] for k in m._graphs}


def _guide64(ep, en, w, phi):
    ep, en = ep.double(), en.double()
    out = []
    for b in range(ep.shape[0]):
        g = en[b] + w * (ep[b] - en[b])
        if phi != 0:
            sg = float(g.std(unbiased=False))
            g = (phi * float(ep[b].std(unbiased=False)) / sg + (1 - phi) if sg > 0 else 1.0) * g
        out.append(g)
    return torch.stack(out)


def test_guided_chain_is_the_plain_2b_chain_at_w_one(dev):
    T, B = 20, 2
    m, _ = _cond_model(T, 2 * B)
    shape, shape2 = (B, 8, 8, 8, 4), (2 * B, 8, 8, 8, 4)
    c, n = [1, 0], [0, 1]
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    kw = dict(sampler="dpmpp", num_steps=5)
    got = m.generate(shape, context_value=c, x_T=x_T, guidance_scale=1.0, negative_context=n, **kw)
    plain = m.generate(shape2, context_value=c + n, x_T=torch.cat([x_T, x_T]), **kw)
    torch.cuda.synchronize()
    assert got.shape == shape and torch.isfinite(got).all()
    assert torch.equal(got, plain[:B]) and not torch.equal(plain[:B], plain[B:])
    assert torch.equal(m.generate(shape, context_value=c, x_T=x_T, guidance_scale=0.0, negative_context=n, **kw), plain[B:])
    assert {"dpmpp", "dpmpp-cfg"} <= {k[1] for k in m._graphs}


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_chain_matches_float64(dev, phi):
    """8^3 x 4ch, T = 20, S = 5, B = 2, per-volume contexts, w = 3.  Bar: the guidance tests' (the chain bar times |w| + |1 - w| = 5)."""
    from oracle import ref_torch as rt
    T, S, B, w = 20, 5, 2, 3.0
    m, W = _cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(23))
    c, n = torch.tensor([[[1]], [[0]]]), torch.tensor([[[0]], [[1]]])
    f, ab = _oracle(W, 8, 4), rt.Betas(T).alpha_bar.double()
    kw = dict(context_value=c, x_T=x_T, sampler="dpmpp", num_steps=S)
    got = m.generate(shape, guidance_scale=w, negative_context=n, guidance_rescale=phi, **kw)
    ref = _chain64(lambda x, t: _guide64(f(x, t, c), f(x, t, n), w, phi), ab, _schedule(T, S), x_T)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"guided dpmpp phi={phi} chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR * (abs(w) + abs(1 - w))
    assert not torch.equal(got, m.generate(shape, **kw))                  # guidance does something
    eager = m.generate(shape, guidance_scale=w, negative_context=n, guidance_rescale=phi, use_graph=False, **kw)
    assert torch.equal(eager, got)
    # a guided edit: kept voxels are x0 bitwise, graph and eager agree
    x0 = torch.rand(shape, generator=torch.Generator().manual_seed(24)) * 2 - 1
    ekw = dict(mask=_half_mask(B), strength=0.6, seed=3, sampler="dpmpp", num_steps=S, guidance_scale=w, negative_context=n, guidance_rescale=phi)
    a, b = m.edit(x0, c, **ekw), m.edit(x0, c, use_graph=False, **ekw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a.cpu()[:, 5:], x0[:, 5:]) and not torch.equal(a.cpu()[:, :4], x0[:, :4])
    assert "dpmpp-edit-cfg" in {k[1] for k in m._graphs}


def test_full_size_chain(dev):
    """32^3 x 8ch (h3), B = 2, S = 8 of T = 1000, plain and guided: finite, the range guard quiet (generate() raises if it is flagged).
    The output conv is scaled by 0.1 as in the DDIM tests: untrained weights amplify eps along a deterministic chain."""
    import dm3d_amd
    T, S, B, C = 1000, 8, 2, 8
    cfg = dm3d_amd.UNetConfig(img_size=32, img_channels=C)
    W = dm3d_amd.synthetic_weights(cfg, seed=0)
    Wb = dict(W, **{k: W[k] * np.float32(0.1) for k in ("out.conv.kernel", "out.conv.bias")})
    m, _ = _cond_model(T, B, size=32, C=C, W=Wb, precision="h3")
    shape = (B, 32, 32, 32, C)
    out = m.generate(shape, context_value=[1, 0], seed=7, sampler="dpmpp", num_steps=S)
    guided = m.generate(shape, context_value=[1, 0], seed=7, sampler="dpmpp", num_steps=S, guidance_scale=3.0, negative_context=[0, 1],
                        guidance_rescale=0.7)
    torch.cuda.synchronize()
    for v in (out, guided):
        assert torch.isfinite(v).all() and float(v.abs().max()) <= 1.0 + 1e-6
    assert not torch.equal(out, guided)
