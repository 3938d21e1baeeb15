"""GPU tier of dynamic thresholding (dm3d_x0_threshold; DiffusionModel.x0_threshold, ddim_step / dpm_step / generate / edit / sampler
with dynamic_threshold / threshold_max).

The bound s is exact, so it is compared bitwise with the np.float32 restatement of the rule (include/dm3d.h, dm3d_thresh_desc) in
tests/chain_reference.py: x0 by the same three float32 operations, the order statistics from np.sort.  Chains are compared with that
module's float64 chains driven by the CPU oracle (oracle.ref_torch.unet_forward), whose quantile is numpy's "linear" one in float64.
"""
import math
import os

import numpy as np
import pytest
import torch

import chain_reference as cr

pytestmark = pytest.mark.gpu
CHAIN_BAR = 2e-3        # the DDIM / DPM-Solver++ chain tests' bar
KERNEL_BAR = 2e-6       # their kernel tests' bar
ROUND = 6e-8            # one float32 rounding of a value <= 1: the thresholded estimate the float64 formulas start from


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return torch.device("cuda:0")


# ---- the rule, restated in np.float32 (cr.x0_32, cr.bound32) ------------------------------------------------------------------------
def _apply32(x0, s):
    with np.errstate(all="ignore"):
        return np.where(np.isnan(x0), x0, np.minimum(np.maximum(x0, -s), s) / s).astype(np.float32)


def _bounds32(x, e, ab32, t, p, smax=None):
    B = x.shape[0]
    t, p = np.broadcast_to(np.asarray(t), (B,)), np.broadcast_to(np.asarray(p, dtype=np.float64), (B,))
    smax = np.broadcast_to(np.asarray(cr.F32_MAX if smax is None else smax, dtype=np.float64), (B,))
    out = [cr.bound32(cr.x0_32(x[b], e[b], ab32, t[b]), p[b], smax[b]) for b in range(B)]
    return np.array([o[0] for o in out], dtype=np.float32), np.array([o[1] for o in out], dtype=np.float32)


def _same(got, want):
    """Bitwise, a NaN matching any NaN."""
    got, want = np.asarray(got.detach().cpu() if torch.is_tensor(got) else got, dtype=np.float32), np.asarray(want, dtype=np.float32)
    nan = np.isnan(want)
    return got.shape == want.shape and np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


# ---- 1. the bound is bitwise ---------------------------------------------------------------------------------------------------------
SHAPES = [(2, 4), (2, 500), (2, 1028), (2, 2048), (3, 8, 8, 8, 4), (2, 10240)]       # 10240: two blocks, the second one partial


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bound_is_bitwise(dev, shape):
    T, B = 1000, shape[0]
    m, _ = cr.cond_model(T, B)
    ab = cr.oracle_alpha_bar(T)
    g = torch.Generator().manual_seed(int(np.prod(shape)))
    x, e = (torch.randn(shape, generator=g) for _ in range(2))
    t = [400, 30, 900][:B] if len(shape) == 5 else 300                # a different row per volume at 8^3 x 4
    regimes = set()
    for scale in (0.02, 1.0, 40.0):                                    # s_raw < 1, 1 < s_raw < smax, s_raw > smax
        for p in (0.5, 0.995, 1.0, [0.5, 1.0, 0.9][:B]):
            for smax in (3.0, None, [1.0, 2.5, 100.0][:B]):
                xs, es = x * scale, e * scale
                want, raw = _bounds32(xs.numpy(), es.numpy(), ab, t, p, smax)
                got = m.x0_threshold(xs, es, torch.as_tensor(t), p, smax)
                assert got.shape == (B,) and got.dtype == torch.float32
                assert _same(got, want), (scale, p, smax, got.cpu().numpy(), want)
                if smax == 3.0:
                    regimes |= {"below" if r < 1 else "above" if r > 3 else "between" for r in raw}
                    assert all((w == 1) if r < 1 else (w == 3) if r > 3 else (w == r) for w, r in zip(want, raw))
    assert regimes == {"below", "between", "above"}
    # a row that does not clip: s = 1 whatever the values
    assert _same(m.x0_threshold(x * 40, e * 40, torch.as_tensor(t), 0.5, clip_x0=False), np.ones(B, np.float32))
    # the call repeats bitwise and leaves its inputs alone
    xd, ed = (x * 3).to(dev), (e * 3).to(dev)
    keep = xd.clone(), ed.clone()
    a, b = m.x0_threshold(xd, ed, torch.as_tensor(t), 0.995), m.x0_threshold(xd, ed, torch.as_tensor(t), 0.995)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(xd, keep[0]) and torch.equal(ed, keep[1])


# ---- 2. ties and specials ------------------------------------------------------------------------------------------------------------
def _x0_inputs(x0, ab32, t):
    """x / eps whose float32 x0 estimate at timestep t is exactly ``x0``: eps = 0 and x = x0 * sqrt(a), checked."""
    a = np.float64(np.asarray(ab32)[t])
    with np.errstate(all="ignore"):
        x = (np.asarray(x0, dtype=np.float32) * np.float32(np.sqrt(a))).astype(np.float32)
    return x, np.zeros_like(x)


def test_ties_and_specials(dev):
    T, N, t = 1000, 2048, 300
    m, _ = cr.cond_model(T, 2)
    ab = cr.oracle_alpha_bar(T)
    rng = np.random.default_rng(5)

    def check(x, e, p, smax=None, t=t):
        want, raw = _bounds32(x, e, ab, t, p, smax)
        got = m.x0_threshold(torch.from_numpy(x), torch.from_numpy(e), t, p, smax)
        assert _same(got, want), (p, smax, got.cpu().numpy(), want)
        return want, raw

    # one repeated value (above and below 1), every rank inside the one run
    for value in (2.75, 0.3):
        x = np.full((2, N), value, np.float32)
        x[1] = -x[1]
        for p in (0.5, 0.995, 1.0):
            want, raw = check(x, np.zeros_like(x), p)
            assert raw[0] == raw[1] and (want[0] > 1) == (value > 1)
    # values quantised to 8 levels: v_i == v_{i+1} inside a long run, and ranks that straddle two runs
    levels = np.linspace(0.25, 4.0, 8).astype(np.float32)
    x = (levels[rng.integers(0, 8, (2, N))] * rng.choice([-1.0, 1.0], (2, N))).astype(np.float32)
    e = np.zeros_like(x)
    for p in (0.5, 0.9, 0.995, 1.0):
        check(x, e, p)
    counts = np.cumsum(np.bincount(np.searchsorted(levels, np.sort(np.abs(cr.x0_32(x[0], e[0], ab, t)))), minlength=8))
    edge = int(counts[3]) - 1                                          # the last element of a run: v_i and v_{i+1} differ
    v = np.sort(np.abs(cr.x0_32(x[0], e[0], ab, t)))
    assert v[edge] != v[edge + 1]
    check(x, e, (edge + 0.5) / (N - 1))
    # +-0, +-inf and magnitudes that differ in the lowest mantissa bit only (the last digit of the select)
    base = np.float32(1.5)
    ulps = np.array([base.view(np.uint32) + k for k in range(8)], dtype=np.uint32).view(np.float32)
    x0 = np.empty((2, N), np.float32)
    x0[0] = ulps[rng.integers(0, 8, N)] * rng.choice([-1.0, 1.0], N)
    x0[1] = rng.standard_normal(N)
    x0[1, :6] = [0.0, -0.0, np.inf, -np.inf, 0.0, -0.0]
    x, e = _x0_inputs(x0, ab, t)
    got_x0 = np.stack([cr.x0_32(x[b], e[b], ab, t) for b in range(2)])
    assert len(np.unique(np.abs(got_x0[0]))) >= 4 and np.ptp(np.abs(got_x0[0]).view(np.uint32).astype(np.int64)) <= 16
    assert np.isinf(got_x0[1]).sum() == 2 and (got_x0[1] == 0).sum() == 4
    for p in (0.25, 0.5, 0.75, 0.995, (N - 3.5) / (N - 1), 1.0, 1e-4):
        check(x, e, p)
    want, raw = check(x, e, (N - 3.5) / (N - 1))
    assert np.isfinite(raw[1])                                         # below the two infinities
    want, raw = check(x, e, 1.0)
    assert np.isnan(want[1]) and np.isfinite(want[0])
    # one NaN at p = 0.995 leaves s finite; N-1-i+1 NaNs reach v_i: s is NaN
    xr = rng.standard_normal((2, N)).astype(np.float32) * 2
    er = rng.standard_normal((2, N)).astype(np.float32)
    i = int(math.floor(0.995 * (N - 1)))
    one = xr.copy()
    one[0, 77] = np.nan
    want, _ = check(one, er, 0.995)
    assert np.all(np.isfinite(want))
    many = xr.copy()
    many[0, rng.choice(N, N - 1 - i + 1, replace=False)] = np.nan
    want, _ = check(many, er, 0.995)
    assert np.isnan(want[0]) and np.isfinite(want[1])
    fewer = xr.copy()
    fewer[0, rng.choice(N, N - 1 - i - 1, replace=False)] = np.nan    # fewer than N-1-i: v_{i+1} is still a number
    want, _ = check(fewer, er, 0.995)
    assert np.all(np.isfinite(want))


# ---- 3. the update -------------------------------------------------------------------------------------------------------------------
def test_update_matches_restatement(dev):
    """ddim_step / dpm_step with the keywords: the restatement's float32 clamp(x0, -s, s) / s, then the float64 step formulas.  Bars: the
    DDIM / DPM-Solver++ kernel tests' for the same outputs plus one float32 rounding of the thresholded estimate."""
    T, B = 1000, 3
    m, _ = cr.cond_model(T, B)
    ab32 = cr.oracle_alpha_bar(T)
    ab = ab32.double()
    g = torch.Generator().manual_seed(31)
    shape = (B, 8, 8, 8, 4)
    x, e, z, h = (torch.randn(shape, generator=g) for _ in range(4))
    x = x * 2
    xd, ed, hd = x.to(dev), e.to(dev), h.to(dev)
    keep = [v.clone() for v in (xd, ed, hd)]
    p, smax = [0.9, 0.995, 0.6], [100.0, 100.0, 1.5]
    for t, tp, tb in (([400, 300, 20], [380, 150, -1], [420, 999, 25]), ([500, 999, 5], [480, 979, -1], [520, -1, 9])):
        s, _ = _bounds32(x.numpy(), e.numpy(), ab32, t, p, smax)
        assert np.any(s > 1) and np.all(np.isfinite(s))
        x0 = [torch.from_numpy(_apply32(cr.x0_32(x[b], e[b], ab32, t[b]), s[b])).reshape(shape[1:]).double() for b in range(B)]
        for eta in (0.0, 0.5):
            got = m.ddim_step(xd, ed, torch.tensor(t), torch.tensor(tp), eta, noise=z, dynamic_threshold=p, threshold_max=smax).cpu()
            for b in range(B):
                ref = cr.ddim_update64(x0[b], e[b].double(), float(ab[t[b]]), float(ab[tp[b]]) if tp[b] >= 0 else 1.0, eta, z[b])
                err = float((got[b].double() - ref).abs().max())
                print(f"ddim_step eta={eta} t={t[b]} -> {tp[b]} s={s[b]:.4f}: err {err:.2e}")
                assert float(ref.abs().max()) < 20 and err < KERNEL_BAR + ROUND
        second = all(v > 0 for v in tb)
        hist = (hd, torch.tensor(tb)) if second else ()
        got, got0 = m.dpm_step(xd, ed, torch.tensor(t), torch.tensor(tp), *hist, dynamic_threshold=p, threshold_max=smax)
        got, got0 = got.cpu(), got0.cpu()
        for b in range(B):
            pb = tb[b] if second else -1
            ref = cr.dpm_update64(x[b].double(), x0[b], ab, t[b], tp[b], pb, h[b])
            bar = KERNEL_BAR * max(1.0, sum(abs(c) for c in cr.dpm_row64(ab, t[b], tp[b], pb))) + ROUND
            err = float((got[b].double() - ref).abs().max())
            print(f"dpm_step t={t[b]} -> {tp[b]} (before {pb}) s={s[b]:.4f}: err {err:.2e} (bar {bar:.2e})")
            assert err < bar
            assert torch.equal(got0[b], x0[b].float())                  # the estimate handed on is the restatement's, bitwise
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip((xd, ed, hd), keep))     # mode 0 leaves x, eps and the history alone
    # inputs whose bound is 1: bitwise the call without the keywords
    xs, es = xd * 0.05, ed * 0.05
    t, tp = torch.tensor([400, 300, 20]), torch.tensor([380, 150, -1])
    s, raw = _bounds32(xs.cpu().numpy(), es.cpu().numpy(), ab32, t.numpy(), 0.995)
    assert np.all(s == 1) and np.all(raw < 1)
    s, raw = _bounds32(xd.cpu().numpy(), ed.cpu().numpy(), ab32, t.numpy(), 0.995, 1.0)
    assert np.all(s == 1) and np.all(raw > 1)                              # capped at 1: the static clamp, with elements to clamp
    for xi, ei, cap in ((xs, es, None), (xd, ed, 1.0)):
        kw = dict(dynamic_threshold=0.995, threshold_max=cap)
        assert torch.equal(m.ddim_step(xi, ei, t, tp, 0.5, noise=z, **kw), m.ddim_step(xi, ei, t, tp, 0.5, noise=z))
        a, b = m.dpm_step(xi, ei, t, tp, hd, torch.tensor([420, 999, 25]), **kw), m.dpm_step(xi, ei, t, tp, hd, torch.tensor([420, 999, 25]))
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- 4. chains -----------------------------------------------------------------------------------------------------------------------
P_CHAIN, CAP_CHAIN = 0.9, 6.0
SOLVERS = [("ddim", dict(eta=0.0)), ("ddim", dict(eta=0.5)), ("dpmpp", dict(solver_order=1)), ("dpmpp", dict(solver_order=2))]
X_SCALE = 1.5           # of x_T and of the edited latent
OUT_SCALE = 3.0         # of the output conv.  A DDIM chain at eta = 0 carries eps on, so once its estimate is thresholded the next one
                        # exceeds 1 only by what eps changed between the steps: with the synthetic weights as they are that chain
                        # has s > 1 at its first step alone; at 3x two of five steps (and two of an edit's three) have it, and every
                        # step of the DPM-Solver++ chains (asserted below)


@pytest.fixture(scope="module")
def chain_model(dev):
    T, B = 20, 2
    m, W = cr.cond_model(T, B, W=cr.weights(scale=OUT_SCALE))
    return m, cr.oracle(W), cr.oracle_alpha_bar(T).double(), T, B


@pytest.mark.parametrize("solver,opts", SOLVERS, ids=lambda v: v if isinstance(v, str) else "-".join(f"{k}{x}" for k, x in v.items()))
@pytest.mark.parametrize("mode", ["plain", "guided", "guided-rescaled", "edit", "guided-edit"])
def test_chain_matches_float64(chain_model, solver, opts, mode):
    """8^3 x 4ch, T = 20, S = 5, B = 2, per-volume contexts: plain, guided (w = 3, phi 0 and 0.7), edit (half mask, strength 0.6, 3
    steps) and guided edit, against the float64 chain.  Bar: the chain tests' (guided: times |w| + |1 - w|, as theirs)."""
    from dm3d_amd.diffusion import edit_steps, latent_mask
    m, f, ab, T, B = chain_model
    S, w = 5, 3.0
    shape = (B, 8, 8, 8, 4)
    g = torch.Generator().manual_seed(61)
    x_T = torch.randn(shape, generator=g) * X_SCALE
    c, n = torch.tensor([[[1]], [[0]]]), torch.tensor([[[0]], [[1]]])
    guided, edit = mode.startswith("guided"), mode.endswith("edit")
    phi = 0.7 if mode == "guided-rescaled" else 0.0
    eta = opts.get("eta", 0.0)
    order = opts.get("solver_order", 2)
    eps_fn = (lambda x, t: cr.guide64(f(x, t, c), f(x, t, n), w, phi)) if guided else (lambda x, t: f(x, t, c))
    kw = dict(sampler=solver, num_steps=S, dynamic_threshold=P_CHAIN, threshold_max=CAP_CHAIN, **opts)
    if guided:
        kw.update(guidance_scale=w, negative_context=n, guidance_rescale=phi)
    bounds = []
    if not edit:
        sched = cr.schedule(T, S)
        noise = torch.randn((S,) + shape, generator=g) if eta else None
        got = m.generate(shape, context_value=c, x_T=x_T, noise=noise, **kw)
        ref = cr.chain64(eps_fn, ab, sched, x_T, solver, eta=eta, noise=noise, order=order, thr=(P_CHAIN, CAP_CHAIN, bounds))
        plain = m.generate(shape, context_value=c, x_T=x_T, noise=noise, **{k: v for k, v in kw.items() if "threshold" not in k})
    else:
        x0 = (torch.rand(shape, generator=g) * 2 - 1) * X_SCALE
        k = edit_steps(0.6, S)
        sched = cr.schedule(T, S)[:k]
        assert k == 3
        known_noise = torch.randn((k + 1,) + shape, generator=g)
        noise = torch.randn((k,) + shape, generator=g) if eta else None
        mask = cr.half_mask(B, 16)
        blend = cr.edit_blend64(x0, ab, sched, 1 - latent_mask(mask, shape), known_noise)
        ekw = dict(mask=mask, strength=0.6, known_noise=known_noise, noise=noise, **kw)
        got = m.edit(x0, c, **ekw)
        ref = cr.chain64(eps_fn, ab, sched, cr.known64(x0, ab, sched[-1], known_noise[k]), solver, eta=eta, noise=noise, order=order,
                         thr=(P_CHAIN, CAP_CHAIN, bounds), blend=blend)
        plain = m.edit(x0, c, **{k_: v for k_, v in ekw.items() if "threshold" not in k_})
        assert torch.equal(got.cpu()[:, 4:], x0[:, 4:])                 # the kept half is x0 bitwise
    steps = len(bounds) // B
    active = sum(any(s > 1 for s in bounds[i * B:(i + 1) * B]) for i in range(steps))
    err = float((got.cpu().double() - ref).abs().max())
    print(f"{solver} {opts} {mode}: max abs difference {err:.2e}; s per step {[round(s, 3) for s in bounds]}")
    assert steps == len(sched) and 3 * active >= steps                  # the feature is at work in the float64 chain
    assert err < CHAIN_BAR * ((abs(w) + abs(1 - w)) if guided else 1.0)
    assert not torch.equal(got, plain)                                  # ... and in the kernel's


# ---- 5. graphs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("solver", ["ddim", "dpmpp"])
def test_graph_replay_tables_and_interleaving(dev, solver):
    T, B = 20, 2
    shape = (B, 8, 8, 8, 4)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(3)) * X_SCALE
    ids = [1, 0]
    base = dict(context_value=ids, x_T=x_T, sampler=solver)
    thr_a = dict(num_steps=5, dynamic_threshold=0.9, threshold_max=6.0)
    thr_b = dict(num_steps=8, dynamic_threshold=[0.995, 0.5], threshold_max=[2.0, 50.0])
    plain_a = dict(num_steps=5)
    # a model that never touches the feature: the parent's path, and each chain's solo result
    m0, W = cr.cond_model(T, B, W=cr.weights(scale=OUT_SCALE))
    solo_plain = m0.generate(shape, **base, **plain_a).clone()
    solo_none = m0.generate(shape, **base, **plain_a, dynamic_threshold=None, threshold_max=None).clone()
    assert torch.equal(solo_plain, solo_none)
    assert {k[1] for k in m0._graphs} == {solver}                          # None: the same graph key as ever
    m1, _ = cr.cond_model(T, B, W=W)
    solo_a = m1.generate(shape, **base, **thr_a).clone()
    solo_b = m1.generate(shape, **base, **thr_b).clone()
    kinds = [k[1] for k in m1._graphs]
    assert len(kinds) == 1 and kinds[0] != solver                          # one graph served both ratios, caps and schedules
    assert not torch.equal(solo_a, solo_plain) and not torch.equal(solo_a, solo_b)
    # graph replay equals eager bitwise and repeats bitwise
    for kw, want in ((thr_a, solo_a), (thr_b, solo_b)):
        assert torch.equal(m1.generate(shape, **base, **kw, use_graph=False), want)
        assert torch.equal(m1.generate(shape, **base, **kw), want)
    # a thresholded and a plain chain on one plan, interleaved in either order
    for order in ((thr_a, plain_a, thr_b, plain_a, thr_a), (plain_a, thr_b, plain_a, thr_a)):
        m2, _ = cr.cond_model(T, B, W=W)
        for kw in order:
            want = solo_plain if kw is plain_a else solo_a if kw is thr_a else solo_b
            assert torch.equal(m2.generate(shape, **base, **kw), want)
        assert sorted(k[1] for k in m2._graphs) == sorted([solver, kinds[0]])   # one graph each, neither replays the other's
        assert len({k[0] for k in m2._graphs}) == 1                         # ... on the same plan
    # the sampler() interface: a thresholded chain stepped by hand is generate()'s
    smp = m1.sampler(shape, ids, kind=solver, **thr_a)
    smp.reset(x_T)
    for _ in range(smp.n_steps):
        smp.step()
    torch.cuda.synchronize()
    assert torch.equal(smp.x, solo_a)


# ---- 6. full size --------------------------------------------------------------------------------------------------------------------
def test_full_size_bounds_are_bitwise(dev):
    """32^3 x 8ch (h3), B = 2, three steps of a thresholded DPM-Solver++ chain (S = 8 of T = 1000): each step's s, read from the chain
    and recomputed by x0_threshold on the chain's own x / eps, is the restatement's bitwise.  262 144 values a volume: 32 blocks."""
    T, S, B, C, p = 1000, 8, 2, 8, 0.995
    m, _ = cr.cond_model(T, B, size=32, C=C, W=cr.weights(32, C, scale=0.1), precision="h3")      # as the solvers' full-size tests
    ab = cr.oracle_alpha_bar(T)
    shape = (B, 32, 32, 32, C)
    sched = cr.schedule(T, S)
    smp = m.sampler(shape, [1, 0], seed=7, kind="dpmpp", num_steps=S, dynamic_threshold=[p, 0.9], threshold_max=[cr.F32_MAX, 4.0])
    smp.reset()
    seen = []
    for k in range(3):
        t = sched[S - 1 - k]
        x_before = smp.x.clone()
        smp.step()
        torch.cuda.synchronize()
        eps, got = smp.plan.eps.clone(), smp.plan.thr_bound.clone()
        want, raw = _bounds32(x_before.cpu().numpy(), eps.cpu().numpy(), ab, t, [p, 0.9], [cr.F32_MAX, 4.0])
        again = m.x0_threshold(x_before, eps, t, [p, 0.9], [cr.F32_MAX, 4.0])
        print(f"step from t={t}: s = {got.cpu().numpy()}, s_raw = {raw}")
        assert _same(got, want) and _same(again, want)
        seen += list(raw)
    assert any(r > 1 for r in seen) and torch.isfinite(smp.x).all()
