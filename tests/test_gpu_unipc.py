"""GPU tier of the UniPC sampler (dm3d_unipc_update, DiffusionModel.unipc_step, generate / sampler with "unipc").

The float64 reference is tests/unipc_reference.py, a restatement from the paper's formulas that never sees the library's tables, with
eps from the CPU oracle (oracle.ref_torch.unet_forward) and alpha_bar from the oracle's float32 Betas table, the table the kernels read;
models, oracle and schedules are tests/chain_reference.py's.

Kernel bar.  Measured on the CPU over this file's own kernel inputs (KERNEL_CASES x clip on / off x B = 1, 3 and the two sizes): the worst
|f32-order restatement - float64 restatement| is 4.14e-6 (x_next), 3.9e-7 (x_corr) and 2.5e-6 (x0), on values up to some tens; test_kernel_bar_is_four_times_the_
measured_error recomputes it.  The kernel gets four times the worst of them: KERNEL_BAR = 1.7e-5.  The largest is far below 1e-4, so no
case is ill-conditioned (no tiny r_k).  The chains keep the DPM-Solver++ chain tests' bar, which is the U-Net's error against the
float64 oracle carried through five steps, not the update's."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import chain_reference as cr
import unipc_reference as ur
from guarded_buffers import IN, OUT, Guarded

CHAIN_BAR = 2e-3        # the DPM-Solver++ chain tests' bar (values in [-1, 1] + noise)
MEASURED = 4.2e-6       # worst |f32-order - float64| of the restatement over this file's kernel inputs (CPU)
KERNEL_BAR = 1.7e-5     # four times that (rounded up)
T_K = 1000

# (t, t_prev, t_hist (newest first), predictor order, corrector order), one entry per sample
KERNEL_CASES = [
    ([400, 300, 20], [380, 150, -1], [], 1, 0),                                                         # order 1, no corrector; sample 2 to clean
    ([400, 300, 20], [380, 150, -1], [[420, 330, 25]], 1, 1),                                           # order-1 corrector
    ([400, 300, 20], [380, 150, 10], [[420, 330, 25], [450, 400, 40]], 2, 2),                           # order 2 both
    ([400, 300, 60], [380, 150, 40], [[420, 330, 80], [450, 400, 100], [500, 480, 130]], 3, 3),         # order 3 both: every slot read
    ([600, 500, 200], [550, 450, 100], [[650, 520, 300], [700, 600, 420]], 3, 1),                       # order-3 predictor after an order-1 corrector
]


def _ab(T=T_K):
    return cr.oracle_alpha_bar(T).double().numpy()


def _inputs(B, per, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, per)).astype(np.float32) for _ in range(6)]              # x, eps, xc, h0, h1, h2


def _tables(ab, case, B, clip):
    """The two float32 tables of a launch with one row per sample, from the restatement's own collapse."""
    t, tp, th, p, c = case
    coef, corr = np.zeros((B, 8)), np.zeros((B, 8))
    for b in range(B):
        before = [lv[b] for lv in th]
        coef[b, 0], coef[b, 1] = math.sqrt(ab[t[b]]), math.sqrt(1 - ab[t[b]])
        row = ur.predictor_row(ab, t[b], tp[b], before[:p - 1])
        coef[b, 2:5], coef[b, 5], coef[b, 6] = row[:3], float(clip), row[3]
        if c:
            corr[b, :5] = ur.corrector_row(ab, before[0], t[b], before[1:c])
    return coef.astype(np.float32), corr.astype(np.float32)


def _reference(ab, case, bufs, B, clip, float_order, bound=None):
    t, tp, th, p, c = case
    x, e, xc, *h = bufs
    out = []
    for b in range(B):
        before = [lv[b] for lv in th]
        out.append(ur.kernel(ab, x[b], e[b], xc[b], [v[b] for v in h[:len(th)]], t[b], tp[b], before, p, c, clip=clip,
                             bound=None if bound is None else float(bound[b]), float_order=float_order))
    return [np.stack([o[k] for o in out]) for k in range(3)]


def _sizes():
    return [(1, 4), (3, 4 * 256 + 4)]


def test_kernel_bar_is_four_times_the_measured_error():
    """Needs no GPU: the figure in the docstring, recomputed over the very inputs the kernel tests below use."""
    ab = _ab()
    worst = [0.0, 0.0, 0.0]
    for B, per in _sizes():
        for i, case in enumerate(KERNEL_CASES):
            for clip in (True, False):
                bufs = _inputs(B, per, 100 + i)
                f32, f64 = (_reference(ab, case, bufs, B, clip, o) for o in ("f32", "f64"))
                assert max(float(np.abs(v).max()) for v in f64) < 100            # O(10) values at most: the bar is absolute
                worst = [max(w, float(np.abs(a.astype(np.float64) - b).max())) for w, a, b in zip(worst, f32, f64)]
    print("worst |f32 - f64| (x_next, x_corr, x0):", " ".join(f"{w:.2e}" for w in worst))
    assert max(worst) <= MEASURED < 1e-4 and KERNEL_BAR >= 4 * MEASURED > KERNEL_BAR / 1.1


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return torch.device("cuda:0")


def _launch(dev, bufs, coef, corr, mode, slots=(2, 1, 0), bound=None, rot=0):
    """One guarded launch with one row per sample.  ``slots``: the descriptor slot of h0, h1, h2.  Returns (x_next, x_corr, x0)."""
    from dm3d_amd import _lib
    x, e, xc, h0, h1, h2 = bufs
    B, per = x.shape
    role = OUT if mode == 1 else IN
    coef = coef.copy()
    coef[:, 7] = rot
    g = dict(x=Guarded(x, dev, role), eps=Guarded(e, dev, IN), xc=Guarded(xc, dev, role), coef=Guarded(coef, dev, IN),
             corr=Guarded(corr, dev, IN), pos=Guarded(np.arange(B, dtype=np.int32), dev, IN))
    hs = [Guarded(h, dev, role) for h in (h0, h1, h2)]
    d = _lib.UniPcDesc()
    d.x, d.eps, d.xc, d.coef, d.corr, d.pos = (g[k].ptr for k in ("x", "eps", "xc", "coef", "corr", "pos"))
    for h, s in zip(hs, slots):
        d.hist[s] = h.ptr
    d.batch, d.per_sample, d.rows, d.mode = B, per, B, mode
    outs = []
    if mode == 0:
        outs = [Guarded(np.zeros((B, per), np.float32), dev, OUT) for _ in range(3)]
        d.out, d.xc_out, d.x0_out = (o.ptr for o in outs)
    if bound is not None:
        g["bound"] = Guarded(np.asarray(bound, np.float32), dev, IN)
        d.x0_bound = g["bound"].ptr
    _lib.check(_lib.lib().dm3d_unipc_update(C.byref(d), None), "unipc_update")
    torch.cuda.synchronize()
    for k in ("eps", "coef", "corr", "pos", "bound"):
        if k in g:
            g[k].unchanged()
    if mode == 0:
        for v in [g["x"], g["xc"]] + hs:
            v.unchanged()                                               # mode 0 leaves x, the corrected state and every slot alone
        return [o.get() for o in outs]
    written = hs[slots.index(rot)]                                      # the slot h2 sits in takes the estimate ...
    for h in hs:
        if h is not written:
            h.get()
            assert np.array_equal(h._words(), h.host)                   # ... and the other two stay as they are
    return [g["x"].get(), g["xc"].get(), written.get()]


@pytest.mark.gpu
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("B,per", _sizes())
def test_kernel_matches_float64_restatement(dev, B, per, clip):
    """B = 1 with a single float4, and B = 3 with per_sample = 4 * 256 + 4 (a grid-stride tail) and three distinct rows per launch;
    orders 1, 2 and 3; mode 0 (inputs untouched) and mode 1 (in place, under a rotated slot assignment) give the same bits."""
    ab = _ab()
    for i, case in enumerate(KERNEL_CASES):
        bufs = _inputs(B, per, 100 + i)
        coef, corr = _tables(ab, case, B, clip)
        ref = _reference(ab, case, bufs, B, clip, "f64")
        got = _launch(dev, bufs, coef, corr, 0)
        for name, a, b in zip(("x_next", "x_corr", "x0"), got, ref):
            err = float(np.abs(a.astype(np.float64) - b).max())
            print(f"B={B} per={per} clip={clip} case {i} {name}: err {err:.2e} (bar {KERNEL_BAR:.1e})")
            assert err < KERNEL_BAR, (i, name)
        for b in range(B):
            if case[1][b] < 0:
                assert np.array_equal(got[0][b], got[2][b])             # the clean row hands on x0 bitwise
        if case[4] == 0:
            assert np.array_equal(got[1], bufs[0])                      # no corrector: the corrected state is x bitwise
        for rot, slots in ((0, (2, 1, 0)), (1, (0, 2, 1)), (2, (1, 0, 2))):
            inplace = _launch(dev, bufs, coef, corr, 1, slots=slots, rot=rot)
            assert all(np.array_equal(a, b) for a, b in zip(inplace, got)), (i, rot)


@pytest.mark.gpu
def test_dynamic_bound_is_honoured(dev):
    ab, B, per = _ab(), 3, 4 * 256 + 4
    case, bound = KERNEL_CASES[2], np.array([1.0, 1.7, 3.0], np.float32)
    bufs = _inputs(B, per, 7)
    coef, corr = _tables(ab, case, B, True)
    got = _launch(dev, bufs, coef, corr, 0, bound=bound)
    ref = _reference(ab, case, bufs, B, True, "f64", bound)
    assert all(float(np.abs(a.astype(np.float64) - b).max()) < KERNEL_BAR for a, b in zip(got, ref))
    assert float(np.abs(got[2]).max()) <= 1.0 and np.array_equal(got[2][0], _launch(dev, bufs, coef, corr, 0)[2][0])     # s = 1: the static clamp


@pytest.mark.gpu
def test_nan_reaches_its_element_only_and_zero_coefficients_read_nothing(dev):
    ab, B, per = _ab(), 3, 4 * 256 + 4
    case = KERNEL_CASES[3]                                               # order 3: every buffer is read
    coef, corr = _tables(ab, case, B, True)
    clean = _launch(dev, _inputs(B, per, 9), coef, corr, 0)
    for which in range(6):
        bufs = _inputs(B, per, 9)
        bufs[which][1, 517] = float("nan")
        got = _launch(dev, bufs, coef, corr, 0)
        for k, v in enumerate(got):
            nan = np.isnan(v)
            assert int(nan.sum()) <= 1 and (not nan.any() or nan[1, 517]), (which, k)
            v, c = v.copy(), clean[k].copy()
            v[1, 517] = c[1, 517] = 0
            assert np.array_equal(v, c), (which, k)                     # every other element keeps its bits
        assert np.isnan(got[0][1, 517])                                 # at order 3 each input reaches x_next
    # rows whose coefficients are zero never read the buffer: NaN-filled corrected state and slots under an order-1 row without corrector
    first = KERNEL_CASES[0]
    coef, corr = _tables(ab, first, B, True)
    bufs = _inputs(B, per, 9)
    want = _launch(dev, bufs, coef, corr, 0)
    for k in range(2, 6):
        bufs[k][:] = float("nan")
    got = _launch(dev, bufs, coef, corr, 0)
    assert all(np.array_equal(a, b) for a, b in zip(got, want)) and not any(np.isnan(v).any() for v in got)


# ---- chains ---------------------------------------------------------------------------------------------------------------------
def _numpy(net):
    """A torch net(x, t) as ur.chain calls it: numpy in, numpy out."""
    return lambda x, t: net(torch.from_numpy(np.asarray(x)), t).numpy()


T, S, B = 20, 5, 2
SHAPE = (B, 8, 8, 8, 4)
IDS = torch.tensor([[[1]], [[0]]])


@pytest.fixture(scope="module")
def cond(dev):
    """The conditional 8^3 x 4ch model of tests/test_gpu_dpm.py, its oracle and alpha_bar, built once for the chain tests."""
    m, W = cr.cond_model(T, B)
    return m, cr.oracle(W), _ab(T)


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2, 3])
def test_conditional_chain_matches_float64(dev, cond, order):
    m, f, ab = cond
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(21))
    for clip, variant in ((True, "bh2"), (False, "bh1")):
        got = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="unipc", num_steps=S, clip_x0=clip, solver_order=order,
                         unipc_variant=variant).cpu()
        ref = ur.chain(_numpy(lambda x, t: f(x, t, IDS)), ab, cr.schedule(T, S), x_T.numpy(), order, True, variant, clip)
        err = float(np.abs(got.double().numpy() - ref).max())
        print(f"unipc chain order={order} clip={clip} {variant}: max abs difference {err:.2e}, max |x| {float(np.abs(ref).max()):.3f}")
        assert err < CHAIN_BAR
    if order > 1:                                       # the higher-order rows do something
        kw = dict(context_value=IDS, x_T=x_T, sampler="unipc", num_steps=S, lower_order_final=False)
        assert not torch.equal(m.generate(SHAPE, solver_order=order, **kw), m.generate(SHAPE, solver_order=order - 1, **kw))


@pytest.mark.gpu
@pytest.mark.parametrize("order", [1, 2, 3])
def test_unconditional_chain_matches_float64(dev, order):
    m, W = cr.uncond_model(T, B)
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(22))
    got = m.generate(SHAPE, x_T=x_T, sampler="unipc", num_steps=S, solver_order=order, lower_order_final=False).cpu()
    ref = ur.chain(_numpy(cr.oracle(W, conditional=False)), _ab(T), cr.schedule(T, S), x_T.numpy(), order, False)
    err = float(np.abs(got.double().numpy() - ref).max())
    print(f"unconditional unipc chain order={order}: max abs difference {err:.2e}")
    assert err < CHAIN_BAR


@pytest.mark.gpu
def test_guided_chains(dev, cond):
    """w = 1 is the plain 2B chain bitwise; w = 3 against float64 (bar: the chain bar times |w| + |1 - w| = 5, as the guidance tests)."""
    m, f, ab = cond
    m4, _ = cr.cond_model(T, 2 * B)
    c, n = [1, 0], [0, 1]
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(5))
    kw = dict(sampler="unipc", num_steps=S, solver_order=3)
    got = m4.generate(SHAPE, context_value=c, x_T=x_T, guidance_scale=1.0, negative_context=n, **kw)
    plain = m4.generate((2 * B,) + SHAPE[1:], context_value=c + n, x_T=torch.cat([x_T, x_T]), **kw)
    torch.cuda.synchronize()
    assert torch.isfinite(got).all() and torch.equal(got, plain[:B]) and not torch.equal(plain[:B], plain[B:])
    assert {"unipc", "unipc-cfg"} <= {k[1] for k in m4._graphs}
    w = 3.0
    neg = torch.tensor([[[0]], [[1]]])
    got = m.generate(SHAPE, context_value=IDS, x_T=x_T, guidance_scale=w, negative_context=neg, **kw)
    ref = ur.chain(_numpy(lambda x, t: cr.guide64(f(x, t, IDS), f(x, t, neg), w)), ab, cr.schedule(T, S), x_T.numpy(), 3)
    err = float(np.abs(got.cpu().double().numpy() - ref).max())
    print(f"guided unipc chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR * (abs(w) + abs(1 - w))
    assert torch.equal(got, m.generate(SHAPE, context_value=IDS, x_T=x_T, guidance_scale=w, negative_context=neg, use_graph=False, **kw))


@pytest.mark.gpu
def test_thresholded_chain(dev, cond):
    m, f, ab = cond
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(31)) * 1.5
    kw = dict(context_value=IDS, x_T=x_T, sampler="unipc", num_steps=S, dynamic_threshold=0.9, threshold_max=4.0)
    got = m.generate(SHAPE, **kw)
    ref = ur.chain(_numpy(lambda x, t: f(x, t, IDS)), ab, cr.schedule(T, S), x_T.numpy(), 2, threshold=(0.9, 4.0))
    err = float(np.abs(got.cpu().double().numpy() - ref).max())
    print(f"thresholded unipc chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR and float(got.abs().max()) <= 1.0
    assert torch.equal(got, m.generate(SHAPE, use_graph=False, **kw)) and not torch.equal(got, m.generate(SHAPE, **dict(kw, dynamic_threshold=None, threshold_max=None)))
    assert "unipc+thr" in {k[1] for k in m._graphs}


@pytest.mark.gpu
def test_graph_equals_eager_repeats_and_serves_every_schedule_and_order(dev, cond):
    m, f, ab = cond
    counts = []
    runs = [dict(num_steps=5), dict(num_steps=8, solver_order=3), dict(timesteps=[0, 3, 11, 19], clip_x0=False, solver_order=1),
            dict(num_steps=20, solver_order=3, unipc_variant="bh1"), dict(num_steps=7, lower_order_final=False, solver_order=3), dict(num_steps=1),
            dict(num_steps=2)]
    for kw in runs:
        a = m.generate(SHAPE, context_value=IDS, seed=5, sampler="unipc", use_graph=True, **kw)
        counts.append(len([k for k in m._graphs if k[1] == "unipc"]))
        b = m.generate(SHAPE, context_value=IDS, seed=5, sampler="unipc", use_graph=False, **kw)
        c = m.generate(SHAPE, context_value=IDS, seed=5, sampler="unipc", use_graph=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.isfinite(a).all(), kw
        x_T = m.generate(SHAPE, context_value=IDS, seed=5, sampler="unipc", steps=0, **kw).cpu()
        sched = kw.get("timesteps") or cr.schedule(T, kw["num_steps"])
        ref = ur.chain(_numpy(lambda x, t: f(x, t, IDS)), ab, sched, x_T.numpy(), kw.get("solver_order", 2), kw.get("lower_order_final", True),
                       kw.get("unipc_variant", "bh2"), kw.get("clip_x0", True))
        err = float(np.abs(a.cpu().double().numpy() - ref).max())
        print(f"unipc {kw}: max abs difference {err:.2e}")
        assert err < CHAIN_BAR, kw
    assert counts == [1] * len(runs)


@pytest.mark.gpu
def test_stale_buffers_never_reach_a_chain(dev, cond):
    """A chain's first row has no corrector and reads no history, and later rows read only what the chain wrote: NaN in every UniPC
    buffer of the plan before reset() changes no bit."""
    m, _, _ = cond
    for use_graph in (True, False):
        for kw in (dict(num_steps=5, solver_order=3), dict(num_steps=2), dict(num_steps=1), dict(num_steps=6, lower_order_final=False, solver_order=3)):
            want = m.generate(SHAPE, context_value=1, seed=3, sampler="unipc", use_graph=use_graph, **kw)
            smp = m.sampler(SHAPE, 1, seed=3, kind="unipc", use_graph=use_graph, **kw)
            smp.plan.unipc_hist.fill_(float("nan"))
            smp.plan.unipc_xc.fill_(float("nan"))
            smp.reset()
            for _ in range(smp.n_steps):
                smp.step()
            torch.cuda.synchronize()
            assert torch.isfinite(smp.x).all() and torch.equal(smp.x, want), (use_graph, kw)
            with pytest.raises(RuntimeError):
                smp.step()


@pytest.mark.gpu
def test_kinds_do_not_leak(dev):
    """"unipc" after "dpmpp" on one model, and the reverse, leaves each bitwise as it is alone: neither reuses the other's graph or tables."""
    calls = {"unipc": dict(sampler="unipc", num_steps=5, solver_order=3), "dpmpp": dict(sampler="dpmpp", num_steps=5),
             "ddim": dict(sampler="ddim", num_steps=5, eta=0.5)}
    alone = {}
    for k, kw in calls.items():
        fresh, _ = cr.cond_model(T, B)
        alone[k] = fresh.generate(SHAPE, context_value=0, seed=5, **kw)
    m, _ = cr.cond_model(T, B)
    for k in ("dpmpp", "unipc", "dpmpp", "ddim", "unipc", "ddim"):
        got = m.generate(SHAPE, context_value=0, seed=5, **calls[k])
        torch.cuda.synchronize()
        assert torch.equal(got, alone[k]), k
    assert {"dpmpp", "unipc", "ddim"} <= {k[1] for k in m._graphs}
    assert m._graphs[[k for k in m._graphs if k[1] == "unipc"][0]][0] is not m._graphs[[k for k in m._graphs if k[1] == "dpmpp"][0]][0]
    assert not torch.equal(alone["unipc"], alone["dpmpp"])


@pytest.mark.gpu
def test_unipc_step_is_the_chains_step(dev, cond):
    """A chain rebuilt from unipc_step calls, with the network's eps taken from the model itself, is generate()'s chain."""
    m, _, _ = cond
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(8))
    want = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="unipc", num_steps=S, solver_order=3)
    taus = cr.schedule(T, S)
    p = ur.orders(S, 3, True)
    x, xc, hist, levels = x_T.cuda(), None, [], []
    for r in range(S - 1, -1, -1):
        eps = m.network([x, torch.full((B,), taus[r]), IDS])
        c = p[r + 1] if r < S - 1 else 0
        c = 0 if r == 0 else c
        x, xc, x0 = m.unipc_step(x, eps, taus[r], taus[r - 1] if r > 0 else -1, hist[:max(p[r] - 1, c)], levels[:max(p[r] - 1, c)], xc,
                                 solver_order=p[r], corrector_order=c)
        hist, levels = [x0] + hist, [taus[r]] + levels
    torch.cuda.synchronize()
    err = float((x - want).abs().max())
    print(f"chain from unipc_step calls against generate(): max abs difference {err:.2e}")
    assert err < CHAIN_BAR                               # (the U-Net runs through another plan here: each lies within the bar of one float64 chain)
