"""GPU tier of the DPM-Solver++(2M) sampler (dm3d_dpm_update, DiffusionModel.dpm_step, generate / edit / sampler with "dpmpp").

The float64 reference is tests/chain_reference.py's restatement of the update (Lu et al. 2022, Algorithm 2, in the data-prediction form)
with eps from the CPU oracle (oracle.ref_torch.unet_forward) and alpha_bar from the oracle's float32 Betas table, the table the kernels
read.
"""
import math
import os

import pytest
import torch

import chain_reference as cr

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
    T = 1000
    m, _ = cr.cond_model(T, B)
    ab = cr.oracle_alpha_bar(T).double()
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
            ref, ref0 = cr.dpm64(x[b], e[b], ab, t[b], tp[b], p, h[b], clip)
            assert float(ref.abs().max()) < 20 and float(ref0.abs().max()) < 20             # O(1) values: the bars are absolute
            a = float(ab[t[b]])
            bar = KERNEL_BAR * max(1.0, sum(abs(c) for c in cr.dpm_row64(ab, t[b], tp[b], p)))
            bar0 = KERNEL_BAR * max(1.0, (1 + math.sqrt(1 - a)) / math.sqrt(a))
            err, err0 = float((got[b].double() - ref).abs().max()), float((x0[b].double() - ref0).abs().max())
            print(f"B={B} clip={clip} t={t[b]} -> {tp[b]} (before {p}): x_next err {err:.2e} (bar {bar:.2e}), x0 err {err0:.2e} (bar {bar0:.2e})")
            assert err < bar and err0 < bar0, (t, tp, tb, b)
            if tp[b] < 0:
                assert torch.equal(got[b], x0[b])                                           # the clean row hands on x0 bitwise


def test_order_one_step_is_ddim_eta0_and_inputs_stay(dev):
    """A first-order row is the DDIM step at eta = 0 wherever the x0 estimate is not clipped (where it is, DDIM carries the model's eps
    on and this solver the eps the clipped estimate implies: x enters the update, eps does not)."""
    T, B = 1000, 3
    m, _ = cr.cond_model(T, B)
    ab = cr.oracle_alpha_bar(T).double()
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
                bar = KERNEL_BAR * max(1.0, sum(abs(c) for c in cr.dpm_row64(ab, t[b], tp[b], -1)))
                err = float((got[b] - ddim[b])[inside[b]].abs().max())
                print(f"clip={clip} t={t[b]} -> {tp[b]}: |dpm_step - ddim_step| {err:.2e} (bar {bar:.2e})")
                assert err < bar, (clip, t[b], tp[b])
    m.dpm_step(x, e, 300, 150, h, 400)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((x, e, h), keep))                          # mode 0 leaves x, eps and the history alone


def test_nan_reaches_its_element_only(dev):
    m, _ = cr.cond_model(1000, 2)
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
    m, _ = cr.cond_model(T, B)
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
    T, S, B = 20, 5, 2
    shape = (B, 8, 8, 8, 4)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(21))
    kw = dict(x_T=x_T, sampler="dpmpp", num_steps=S, clip_x0=clip, solver_order=order)
    if conditional:
        m, W = cr.cond_model(T, B)
        ids = torch.tensor([[[1]], [[0]]])
        got = m.generate(shape, context_value=ids, **kw).cpu()
        f = cr.oracle(W)
        eps_fn = lambda x, t: f(x, t, ids)
    else:
        m, W = cr.uncond_model(T, B)
        got = m.generate(shape, **kw).cpu()
        eps_fn = cr.oracle(W, conditional=False)
    ab = cr.oracle_alpha_bar(T).double()
    ref = cr.chain64(eps_fn, ab, cr.schedule(T, S), x_T, order=order, clip=clip)
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
    T, B = 20, 2
    m, W = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    ids = torch.tensor([[[1]], [[0]]])
    f = cr.oracle(W)
    ab = cr.oracle_alpha_bar(T).double()
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
        sched = kw.get("timesteps") or cr.schedule(T, kw["num_steps"])
        ref = cr.chain64(lambda x, t: f(x, t, ids), ab, sched, x_T, order=kw.get("solver_order", 2),
                         lower_order_final=kw.get("lower_order_final", True), clip=kw.get("clip_x0", True))
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
        fresh, _ = cr.cond_model(T, B)
        alone[k] = fresh.generate(shape, context_value=0, seed=5, **kw)
    m, _ = cr.cond_model(T, B)
    for k in ("ddim", "dpmpp", "ddim", "ddpm", "dpmpp", "ddpm", "ddim"):
        got = m.generate(shape, context_value=0, seed=5, **calls[k])
        torch.cuda.synchronize()
        assert torch.equal(got, alone[k]), k
    assert {"dpmpp", "ddim", "ddpm"} <= {k[1] for k in m._graphs}


@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_edit_chain_matches_float64(dev, strength):
    """edit(sampler="dpmpp"), 8^3 x 4ch, T = 20, S = 5, B = 2, a half mask with a fractional slab, injected known_noise: the blend
    follows every update, the history stays unblended, kept voxels are x0 bitwise; strength 0.6 keeps 3 steps and starts first order
    from q_sample(x0, sched[2])."""
    from dm3d_amd.diffusion import edit_steps, latent_mask
    T, S, B = 20, 5, 2
    m, W = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    g = torch.Generator().manual_seed(41)
    x0 = torch.rand(shape, generator=g) * 2 - 1
    n = edit_steps(strength, S)
    sched = cr.schedule(T, S)[:n]
    assert n == (5 if strength == 1.0 else 3)
    known_noise = torch.randn((n + 1,) + shape, generator=g)
    ids = torch.tensor([[[1]], [[0]]])
    mask = cr.half_mask(B, 16, slab=True)
    ab = cr.oracle_alpha_bar(T).double()
    kw = dict(mask=mask, strength=strength, seed=13, sampler="dpmpp", num_steps=S)
    if n == S:
        x_start = m.edit(x0, ids, steps=0, **kw).cpu()                    # generate()'s x_T under the seed
    else:
        x_start = cr.known64(x0, ab, sched[-1], known_noise[n])
    got = m.edit(x0, ids, known_noise=known_noise, **kw).cpu()
    f = cr.oracle(W)
    keep = 1 - latent_mask(mask, shape)
    w = keep.double().unsqueeze(-1)
    blend = cr.edit_blend64(x0, ab, sched, keep, known_noise)
    ref = cr.chain64(lambda x, t: f(x, t, ids), ab, sched, x_start, blend=blend)
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


def test_guided_chain_is_the_plain_2b_chain_at_w_one(dev):
    T, B = 20, 2
    m, _ = cr.cond_model(T, 2 * B)
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
    T, S, B, w = 20, 5, 2, 3.0
    m, W = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(23))
    c, n = torch.tensor([[[1]], [[0]]]), torch.tensor([[[0]], [[1]]])
    f, ab = cr.oracle(W), cr.oracle_alpha_bar(T).double()
    kw = dict(context_value=c, x_T=x_T, sampler="dpmpp", num_steps=S)
    got = m.generate(shape, guidance_scale=w, negative_context=n, guidance_rescale=phi, **kw)
    ref = cr.chain64(lambda x, t: cr.guide64(f(x, t, c), f(x, t, n), w, phi), ab, cr.schedule(T, S), x_T)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"guided dpmpp phi={phi} chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR * (abs(w) + abs(1 - w))
    assert not torch.equal(got, m.generate(shape, **kw))                  # guidance does something
    eager = m.generate(shape, guidance_scale=w, negative_context=n, guidance_rescale=phi, use_graph=False, **kw)
    assert torch.equal(eager, got)
    # a guided edit: kept voxels are x0 bitwise, graph and eager agree
    x0 = torch.rand(shape, generator=torch.Generator().manual_seed(24)) * 2 - 1
    ekw = dict(mask=cr.half_mask(B, 16, slab=True), strength=0.6, seed=3, sampler="dpmpp", num_steps=S, guidance_scale=w, negative_context=n, guidance_rescale=phi)
    a, b = m.edit(x0, c, **ekw), m.edit(x0, c, use_graph=False, **ekw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a.cpu()[:, 5:], x0[:, 5:]) and not torch.equal(a.cpu()[:, :4], x0[:, :4])
    assert "dpmpp-edit-cfg" in {k[1] for k in m._graphs}


def test_full_size_chain(dev):
    """32^3 x 8ch (h3), B = 2, S = 8 of T = 1000, plain and guided: finite, the range guard quiet (generate() raises if it is flagged).
    The output conv is scaled by 0.1 as in the DDIM tests: untrained weights amplify eps along a deterministic chain."""
    T, S, B, C = 1000, 8, 2, 8
    m, _ = cr.cond_model(T, B, size=32, C=C, W=cr.weights(32, C, scale=0.1), precision="h3")
    shape = (B, 32, 32, 32, C)
    out = m.generate(shape, context_value=[1, 0], seed=7, sampler="dpmpp", num_steps=S)
    guided = m.generate(shape, context_value=[1, 0], seed=7, sampler="dpmpp", num_steps=S, guidance_scale=3.0, negative_context=[0, 1],
                        guidance_rescale=0.7)
    torch.cuda.synchronize()
    for v in (out, guided):
        assert torch.isfinite(v).all() and float(v.abs().max()) <= 1.0 + 1e-6
    assert not torch.equal(out, guided)
