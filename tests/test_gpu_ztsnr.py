"""GPU tier of the zero-terminal-SNR schedule: dm3d_ddim_update_frame, dm3d_dpm_update_frame and dm3d_x0_threshold with ``frame`` set, bitwise against
numpy float32 restatements inside guarded buffers; the chains of a zero-terminal-SNR v- and x0-model against the float64 chains of
tests/chain_reference.py, written from the formulas of DESIGN.md section 4.13 (the network is the CPU oracle's, its output read as v or
as x0; guidance combines and rescales the raw predictions); graph against eager; a
zero-terminal-SNR model beside a plain v-model; and one train_step whose timesteps include T-1 against torch.autograd in float64."""
import ctypes as C
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import chain_reference as cr
from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu
CHAIN_BAR = 2e-3        # the project's chain bar (tests/test_gpu_ddim.py, tests/test_gpu_objective.py)
GUIDED_BAR = 5 * CHAIN_BAR   # guided chains at w = 3: the bar times |w| + |1 - w| = 5 (tests/test_gpu_guidance.py)
SIZES = [4, 1004, 131084]      # per_sample: one float4; a partial block; grid-stride trips and a tail (tests/test_gpu_objective.py)
F = np.float32
T_K = 1000
ROWS_T = (T_K - 1, 517, 0)     # the rows' timesteps: alpha_bar = 0, mid-schedule, t = 0


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return torch.device("cuda:0")


def _st():
    return torch.cuda.current_stream().cuda_stream


def _bits(a):
    return np.ascontiguousarray(a, dtype=F).view(np.uint32)


# ---- float32 restatements --------------------------------------------------------------------------------------------------------------
def _lin(k_a, a, k_b, b):
    """k_a*a + k_b*b in float32: mul, mul, add, each rounded."""
    out = F(k_a) * a + F(k_b) * b
    assert out.dtype == F
    return out


def _bounded(x0, clip, s):
    """dm3d_x0_bounded: off; the static clamp (s None); clamp(x0, -s, s) / s."""
    if not clip:
        return x0
    if s is None:
        return np.minimum(np.maximum(x0, F(-1)), F(1))
    return np.minimum(np.maximum(x0, -F(s)), F(s)) / F(s)


def _tables(kind):
    """The zero-terminal-SNR alpha_bar (float32), the frame rows at ROWS_T, and DDIM / DPM coefficient rows [3, 8] for the steps
    999 -> 900 (from alpha_bar = 0; DPM: first order), 517 -> 400 (DPM: second order, the step before started from 640) and 0 -> clean;
    DDIM at eta = 0.5 (sigma != 0 in rows 0 and 1, 0 in the row to clean)."""
    import dm3d_amd
    from dm3d_amd.diffusion import ddim_coefficients, dpm_coefficients, frame_table
    ab = dm3d_amd.Betas(T_K, zero_terminal_snr=True).alpha_bar
    assert ab[T_K - 1] == 0.0
    src, dst, prev = np.array(ROWS_T), np.array([900, 400, -1]), np.array([-1, 640, 3])
    frame = np.ascontiguousarray(frame_table(ab, kind)[src])
    ddim = np.zeros((3, 8))
    ddim[:, :5] = ddim_coefficients(ab, src, dst, 0.5)
    dpm = np.zeros((3, 8))
    dpm[:, :2] = ddim[:, :2]
    dpm[:, 2:5] = dpm_coefficients(ab, src, dst, prev)
    assert ddim[0, 4] != 0 and ddim[1, 4] != 0 and ddim[2, 4] == 0
    assert dpm[0, 4] == 0 and dpm[1, 4] != 0 and dpm[2, 4] == 0 and np.all(np.isfinite(dpm)) and np.all(np.isfinite(ddim))
    return frame, ddim.astype(F), dpm.astype(F)


POS = (2, 0, 1)                 # sample b runs row POS[b]: every sample another row, none its own index
S_DYN = (1.0, 1.75, 2.5)        # the dynamic bounds of the three samples
CLIPS = ("off", "static", "dynamic")


def _inputs(per, seed):
    rng = np.random.default_rng(seed)
    x, p, z, h = (rng.standard_normal((3, per)).astype(F) * F(1.5) for _ in range(4))
    return x, p, z, h


@pytest.mark.parametrize("per", SIZES)
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_ddim_update_with_frame_is_bitwise_the_restatement(dev, kind, per):
    from dm3d_amd import _lib
    frame, coef, _ = _tables(kind)
    x, p, z, _ = _inputs(per, per)
    for clip in CLIPS:
        c = coef.copy()
        c[:, 5] = 0.0 if clip == "off" else 1.0
        # columns 0 and 1 are not read with a frame: poison them
        c[:, 0:2] = np.nan
        want = np.empty_like(x)
        for b, r in enumerate(POS):
            k0x, k0p, kex, kep = frame[r]
            x0 = _bounded(_lin(k0x, x[b], k0p, p[b]), clip != "off", S_DYN[b] if clip == "dynamic" else None)
            e = _lin(kex, x[b], kep, p[b])
            zb = z[b] if c[r, 4] != 0 else np.zeros_like(z[b])
            want[b] = (c[r, 2] * x0 + c[r, 3] * e) + c[r, 4] * zb
        assert want.dtype == F and np.all(np.isfinite(want))
        for mode in (0, 1):
            runs = []
            for _ in range(2):
                gx = Guarded(x, dev, OUT if mode == 1 else IN)
                gp, gz, gc, gf = (Guarded(a, dev, IN) for a in (p, z, c, frame))
                gout = Guarded(np.zeros_like(x), dev, OUT)
                gtau = Guarded(np.array(ROWS_T, np.int32), dev, IN)
                gnext = Guarded(np.array([900, 400, 0], np.int32), dev, IN)
                gpos = Guarded(np.array(POS, np.int32), dev, IN)
                gtidx = Guarded(np.full(3, -7, np.int32), dev, OUT)
                gs = Guarded(np.array(S_DYN, F), dev, IN)
                d = _lib.DdimDesc()
                d.x, d.eps, d.noise, d.coef, d.tau, d.pos = gx.ptr, gp.ptr, gz.ptr, gc.ptr, gtau.ptr, gpos.ptr
                d.t_next, d.t_idx = gnext.ptr, gtidx.ptr
                d.out = gout.ptr if mode == 0 else None
                d.x0_bound = gs.ptr if clip == "dynamic" else None
                d.batch, d.per_sample, d.rows, d.mode = 3, per, 3, mode
                _lib.check(_lib.lib().dm3d_ddim_update_frame(C.byref(d), gf.ptr, _st()), "ddim_update_frame")
                torch.cuda.synchronize()
                got = (gout if mode == 0 else gx).get()
                for g in (gp, gz, gc, gf, gtau, gnext, gpos, gs) + ((gx,) if mode == 0 else ()):
                    g.unchanged()
                if mode == 1:
                    assert np.all(_bits(gout.get()) == _bits(np.zeros_like(x)))          # out is not written in mode 1
                assert gtidx.get().tolist() == [[900, 400, 0][r] for r in POS]
                runs.append(got)
            assert np.array_equal(_bits(runs[0]), _bits(want)), (kind, per, clip, mode)
            assert np.array_equal(_bits(runs[0]), _bits(runs[1]))


@pytest.mark.parametrize("per", SIZES)
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_dpm_update_with_frame_is_bitwise_the_restatement(dev, kind, per):
    from dm3d_amd import _lib
    frame, _, coef = _tables(kind)
    x, p, _, h = _inputs(per, per + 1)
    for clip in CLIPS:
        c = coef.copy()
        c[:, 5] = 0.0 if clip == "off" else 1.0
        c[:, 0:2] = np.nan
        want, want0 = np.empty_like(x), np.empty_like(x)
        for b, r in enumerate(POS):
            v = _bounded(_lin(frame[r, 0], x[b], frame[r, 1], p[b]), clip != "off", S_DYN[b] if clip == "dynamic" else None)
            first = c[r, 2] * x[b] + c[r, 3] * v
            want[b] = first + c[r, 4] * h[b] if c[r, 4] != 0 else first
            want0[b] = v
        assert want.dtype == F and np.all(np.isfinite(want))
        for mode in (0, 1):
            runs = []
            for _ in range(2):
                gx, gh = (Guarded(a, dev, OUT if mode == 1 else IN) for a in (x, h))
                gp, gc, gf = (Guarded(a, dev, IN) for a in (p, c, frame))
                gout, gx0 = (Guarded(np.zeros_like(x), dev, OUT) for _ in range(2))
                gnext = Guarded(np.array([900, 400, 0], np.int32), dev, IN)
                gpos = Guarded(np.array(POS, np.int32), dev, IN)
                gtidx = Guarded(np.full(3, -7, np.int32), dev, OUT)
                gs = Guarded(np.array(S_DYN, F), dev, IN)
                d = _lib.DpmDesc()
                d.x, d.eps, d.hist, d.coef, d.pos = gx.ptr, gp.ptr, gh.ptr, gc.ptr, gpos.ptr
                d.t_next, d.t_idx = gnext.ptr, gtidx.ptr
                if mode == 0:
                    d.out, d.x0_out = gout.ptr, gx0.ptr
                d.x0_bound = gs.ptr if clip == "dynamic" else None
                d.batch, d.per_sample, d.rows, d.mode = 3, per, 3, mode
                _lib.check(_lib.lib().dm3d_dpm_update_frame(C.byref(d), gf.ptr, _st()), "dpm_update_frame")
                torch.cuda.synchronize()
                got, got0 = ((gout, gx0) if mode == 0 else (gx, gh))
                got, got0 = got.get(), got0.get()
                for g in (gp, gc, gf, gnext, gpos, gs) + ((gx, gh) if mode == 0 else ()):
                    g.unchanged()
                if mode == 1:
                    assert np.all(_bits(gout.get()) == 0) and np.all(_bits(gx0.get()) == 0)
                assert gtidx.get().tolist() == [[900, 400, 0][r] for r in POS]
                runs.append((got, got0))
            assert np.array_equal(_bits(runs[0][0]), _bits(want)), (kind, per, clip, mode)
            assert np.array_equal(_bits(runs[0][1]), _bits(want0)), (kind, per, clip, mode)
            assert np.array_equal(_bits(runs[0][0]), _bits(runs[1][0])) and np.array_equal(_bits(runs[0][1]), _bits(runs[1][1]))


@pytest.mark.parametrize("per", SIZES)
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_x0_threshold_with_frame_is_bitwise_the_restatement(dev, kind, per):
    from dm3d_amd import _lib
    from dm3d_amd.diffusion import threshold_tables
    frame, coef, _ = _tables(kind)
    x, p, _, _ = _inputs(per, per + 2)
    rank, frac, smax = threshold_tables(3, per, [0.9, 0.995, 1.0], [100.0, 1.5, 100.0])
    nbytes = int(_lib.lib().dm3d_x0_threshold_scratch_bytes(3, per))
    for clip in ("off", "on"):
        c = coef.copy()
        c[:, 5] = 0.0 if clip == "off" else 1.0
        c[:, 0:2] = np.nan
        want = np.ones(3, F)
        if clip == "on":
            want = np.array([cr.bound32_at(_lin(frame[r, 0], x[b], frame[r, 1], p[b]), rank[b], frac[b], smax[b]) for b, r in enumerate(POS)], F)
            if per > 4:
                assert want[0] > 1 and want[1] == F(1.5) and want[2] > 1      # a quantile, the cap, the maximum
        runs = []
        for _ in range(2):
            gx, gp, gc, gf = (Guarded(a, dev, IN) for a in (x, p, c, frame))
            gpos = Guarded(np.array(POS, np.int32), dev, IN)
            grank, gfrac, gsmax = (Guarded(a, dev, IN) for a in (rank, frac, smax))
            gbound = Guarded(np.zeros(3, F), dev, OUT)
            gscr = Guarded(np.zeros((nbytes + 15) // 16 * 4, np.int32), dev, OUT)
            d = _lib.ThreshDesc()
            d.x, d.eps, d.coef, d.frame, d.pos = gx.ptr, gp.ptr, gc.ptr, gf.ptr, gpos.ptr
            d.rank, d.frac, d.smax, d.bound, d.scratch = grank.ptr, gfrac.ptr, gsmax.ptr, gbound.ptr, gscr.ptr
            d.batch, d.per_sample, d.rows = 3, per, 3
            _lib.check(_lib.lib().dm3d_x0_threshold(C.byref(d), _st()), "x0_threshold")
            torch.cuda.synchronize()
            for g in (gx, gp, gc, gf, gpos, grank, gfrac, gsmax):
                g.unchanged()
            gscr.get()
            runs.append(gbound.get())
        assert np.array_equal(_bits(runs[0]), _bits(want)), (kind, per, clip, runs[0], want)
        assert np.array_equal(_bits(runs[0]), _bits(runs[1]))


# ---- chains ----------------------------------------------------------------------------------------------------------------------------
T_C, S_C = 20, 5
SHAPE = (2, 8, 8, 8, 4)
IDS = torch.tensor([[[1]], [[0]]])
NEG = torch.tensor([[[0]], [[1]]])
THR_P, THR_CAP = 0.9, 4.0


def _intermediates(m, steps_of, **kw):
    """The latents after every step of a chain driven through the public sampler: all finite, the first step included."""
    smp = m.sampler(SHAPE, IDS, **kw)
    smp.reset(steps_of)
    out = []
    for _ in range(smp.n_steps):
        smp.step()
        out.append(smp.x.clone())
    torch.cuda.synchronize()
    return out


CHAINS = [("ddim", dict(eta=0.0)), ("ddim", dict(eta=0.5)), ("dpmpp", dict())]


@pytest.mark.parametrize("solver,opts", CHAINS, ids=["ddim-eta0", "ddim-eta0.5", "dpmpp"])
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_chain_matches_float64(dev, kind, solver, opts):
    """8^3 x 4ch, T = 20, S = 5, B = 2: the first step starts from alpha_bar = 0."""
    m, W = cr.cond_model(T_C, 2, prediction=kind, zero_terminal_snr=True)
    g = torch.Generator().manual_seed(31)
    x_T = torch.randn(SHAPE, generator=g)
    eta = opts.get("eta", 0.0)
    noise = torch.randn((S_C,) + SHAPE, generator=g) if eta else None
    sched, ab = cr.schedule(T_C, S_C), cr.alpha_bar64(T_C, True)
    assert ab[sched[-1]] == 0.0
    got = m.generate(SHAPE, context_value=IDS, x_T=x_T, noise=noise, sampler=solver, num_steps=S_C, **opts).cpu()
    f = cr.oracle(W)
    ref = cr.chain64(lambda x, t: f(x, t, IDS), ab, sched, x_T, solver, kind, eta=eta, noise=noise)
    err = float((got.double() - ref).abs().max())
    print(f"zero-terminal-SNR {kind} model, {solver} {opts}: max abs difference {err:.2e} (max |x| {float(ref.abs().max()):.3f})")
    assert torch.isfinite(got).all() and err < CHAIN_BAR
    # every intermediate state is finite; graph and eager agree bitwise (seeded: Philox draws the z of eta > 0)
    for step in _intermediates(m, x_T, kind=solver, num_steps=S_C, seed=7, **opts):
        assert torch.isfinite(step).all()
    kw = dict(context_value=IDS, x_T=x_T, seed=7, sampler=solver, num_steps=S_C, **opts)
    a, b = m.generate(SHAPE, use_graph=True, **kw), m.generate(SHAPE, use_graph=False, **kw)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    if not eta:
        assert torch.equal(a.cpu(), got)
    assert {k[1] for k in m._graphs} == {{"ddim": "ddim+frame", "dpmpp": "dpmpp+frame"}[solver]}
    # the native chain launches no conversion
    assert m.sampler(SHAPE, IDS, kind=solver, num_steps=S_C, **opts)._pred_d is None


@pytest.mark.parametrize("solver", ["ddim", "dpmpp"])
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_guided_chain_matches_float64(dev, kind, solver):
    """w = 3, phi = 0.7 on the raw predictions of both halves of the plan (Lin et al. 2023 state the rescale for v)."""
    m, W = cr.cond_model(T_C, 2, prediction=kind, zero_terminal_snr=True)
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(32))
    kw = dict(context_value=IDS, x_T=x_T, sampler=solver, num_steps=S_C, guidance_scale=3.0, guidance_rescale=0.7, negative_context=NEG)
    got = m.generate(SHAPE, **kw).cpu()
    f = cr.oracle(W)
    net = lambda x, t: cr.guide64(f(x, t, IDS), f(x, t, NEG), 3.0, 0.7)
    ref = cr.chain64(net, cr.alpha_bar64(T_C, True), cr.schedule(T_C, S_C), x_T, solver, kind)
    err = float((got.double() - ref).abs().max())
    print(f"guided zero-terminal-SNR {kind} model, {solver}: max abs difference {err:.2e}")
    assert torch.isfinite(got).all() and err < GUIDED_BAR
    assert torch.equal(m.generate(SHAPE, use_graph=False, **kw).cpu(), got)
    plain = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler=solver, num_steps=S_C).cpu()
    assert not torch.equal(plain, got)
    smp = m.sampler(SHAPE, IDS, kind=solver, num_steps=S_C, guidance_scale=3.0, guidance_rescale=0.7, negative_context=NEG, seed=3)
    smp.reset(x_T)
    for _ in range(smp.n_steps):
        smp.step()
        assert torch.isfinite(smp.x).all()


@pytest.mark.parametrize("guided", [False, True], ids=["edit", "guided-edit"])
@pytest.mark.parametrize("solver", ["ddim", "dpmpp"])
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_edit_chain_matches_float64(dev, kind, solver, guided):
    """A half mask at full strength: the chain starts from the x_T generate() draws under the seed, at alpha_bar = 0, and the known
    latent is blended back after every step (at its first level it is noised with sqrt(alpha_bar) of that level, never of T-1)."""
    m, W = cr.cond_model(T_C, 2, prediction=kind, zero_terminal_snr=True)
    g = torch.Generator().manual_seed(33)
    x0 = torch.rand(SHAPE, generator=g) * 2 - 1
    known_noise = torch.randn((S_C + 1,) + SHAPE, generator=g)
    mask = cr.half_mask(2)
    sched, ab = cr.schedule(T_C, S_C), cr.alpha_bar64(T_C, True)
    gkw = dict(guidance_scale=3.0, guidance_rescale=0.7, negative_context=NEG) if guided else {}
    x_T = m.generate(SHAPE, context_value=IDS, seed=11, sampler=solver, num_steps=S_C, steps=0).cpu()       # the draw of seed 11
    assert torch.isfinite(x_T).all() and 0.8 < float(x_T.std()) < 1.2
    blend = cr.edit_blend64(x0, ab, sched, 1 - mask, known_noise)
    kw = dict(mask=mask, strength=1.0, sampler=solver, num_steps=S_C, seed=11, **gkw)
    got = m.edit(x0, IDS, known_noise=known_noise, **kw).cpu()
    f = cr.oracle(W)
    net = (lambda x, t: cr.guide64(f(x, t, IDS), f(x, t, NEG), 3.0, 0.7)) if guided else (lambda x, t: f(x, t, IDS))
    ref = cr.chain64(net, ab, sched, x_T, solver, kind, blend=blend)
    err = float((got.double() - ref).abs().max())
    print(f"zero-terminal-SNR {kind} model, {solver} edit, guided {guided}: max abs difference {err:.2e}")
    assert torch.isfinite(got).all() and err < (GUIDED_BAR if guided else CHAIN_BAR)
    assert torch.equal(got[:, 4:], x0[:, 4:])                               # the kept half is x0 bitwise
    a, b = m.edit(x0, IDS, use_graph=True, **kw), m.edit(x0, IDS, use_graph=False, **kw)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    # every intermediate state is finite, the first step included: the chain stopped after 1 .. S steps
    for k in range(1, S_C + 1):
        assert torch.isfinite(m.edit(x0, IDS, steps=k, **kw)).all(), k


@pytest.mark.parametrize("solver", ["ddim", "dpmpp"])
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_thresholded_chain_matches_float64(dev, kind, solver):
    """The output conv scaled by 3 (tests/test_gpu_threshold.py's weights): the float64 chain's bound exceeds 1 at some step."""
    m, W = cr.cond_model(T_C, 2, W=cr.weights(scale=3.0), prediction=kind, zero_terminal_snr=True)
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(34)) * 1.5
    bounds = []
    kw = dict(context_value=IDS, x_T=x_T, sampler=solver, num_steps=S_C, dynamic_threshold=THR_P, threshold_max=THR_CAP)
    got = m.generate(SHAPE, **kw).cpu()
    f = cr.oracle(W)
    ref = cr.chain64(lambda x, t: f(x, t, IDS), cr.alpha_bar64(T_C, True), cr.schedule(T_C, S_C), x_T, solver, kind,
                     thr=(THR_P, THR_CAP, bounds))
    err = float((got.double() - ref).abs().max())
    print(f"thresholded zero-terminal-SNR {kind} model, {solver}: max abs difference {err:.2e}; s per step {[round(s, 3) for s in bounds]}")
    assert len(bounds) == 2 * S_C and max(bounds) > 1.0
    assert torch.isfinite(got).all() and err < CHAIN_BAR
    assert torch.equal(m.generate(SHAPE, use_graph=False, **kw).cpu(), got)
    assert not torch.equal(m.generate(SHAPE, **{k: v for k, v in kw.items() if "threshold" not in k}).cpu(), got)
    assert {k[1] for k in m._graphs} == {solver + "+thr+frame", solver + "+frame"}
    smp = m.sampler(SHAPE, IDS, kind=solver, num_steps=S_C, dynamic_threshold=THR_P, threshold_max=THR_CAP, seed=3)
    smp.reset(x_T)
    for _ in range(smp.n_steps):
        smp.step()
        assert torch.isfinite(smp.x).all()


def test_single_call_forms_are_one_step_of_the_chain(dev):
    """ddim_step / dpm_step / x0_threshold with prediction="v" on the raw output: the chain's first step, from alpha_bar = 0, bitwise;
    without ``prediction`` the same tensors are read as eps, which has no x0 there."""
    m, W = cr.cond_model(T_C, 2, prediction="v", zero_terminal_snr=True)
    sched = cr.schedule(T_C, S_C)
    x_T = torch.randn(SHAPE, generator=torch.Generator().manual_seed(35))
    pred = m.network([x_T.to(dev), torch.tensor([sched[-1]] * 2), IDS])
    want = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="ddim", num_steps=S_C, steps=1)
    got = m.ddim_step(x_T, pred, sched[-1], sched[-2], prediction="v")
    assert torch.equal(got, want) and torch.isfinite(got).all()
    want = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="dpmpp", num_steps=S_C, steps=1)
    got, x0 = m.dpm_step(x_T, pred, sched[-1], sched[-2], prediction="v")
    assert torch.equal(got, want) and torch.equal(x0, (-pred).clamp(-1, 1))
    s = m.x0_threshold(x_T, pred, sched[-1], 1.0, prediction="v")
    assert torch.equal(s, pred.abs().reshape(2, -1).amax(1).clamp(min=1.0))


def test_native_and_converting_chains_do_not_leak(dev):
    """A zero-terminal-SNR v-model and a plain v-model on the same weights and on plans of equal shape, run alternately: each equals a
    fresh model's result bitwise, and each keeps graphs of its own kinds."""
    z, _ = cr.cond_model(T_C, 2, prediction="v", zero_terminal_snr=True)
    v, _ = cr.cond_model(T_C, 2, prediction="v")
    calls = [dict(sampler="ddim", num_steps=5, eta=0.5), dict(sampler="dpmpp", num_steps=5),
             dict(sampler="ddim", num_steps=5, dynamic_threshold=0.9)]
    fresh = {}
    for name, kw in (("z", dict(zero_terminal_snr=True)), ("v", {})):
        fm, _ = cr.cond_model(T_C, 2, prediction="v", **kw)
        fresh[name] = [fm.generate(SHAPE, context_value=IDS, seed=5, **c).clone() for c in calls]
    for _ in range(2):
        for i, c in enumerate(calls):
            assert torch.equal(z.generate(SHAPE, context_value=IDS, seed=5, **c), fresh["z"][i]), c
            assert torch.equal(v.generate(SHAPE, context_value=IDS, seed=5, **c), fresh["v"][i]), c
            assert not torch.equal(fresh["z"][i], fresh["v"][i]) and torch.isfinite(fresh["z"][i]).all()
    assert {k[1] for k in z._graphs} == {"ddim+frame", "dpmpp+frame", "ddim+thr+frame"}
    assert {k[1] for k in v._graphs} == {"ddim+pred", "dpmpp+pred", "ddim+thr+pred"}


# ---- training --------------------------------------------------------------------------------------------------------------------------
def test_train_step_at_the_last_timestep(dev):
    """One public train_step of a zero-terminal-SNR v-model at t = (T-1, 3): x_t is the noise itself at T-1 and the target -x0.  Loss
    and per-sample losses against torch.autograd in float64, weights after Adam against oracle.ref_train.adam_step, with the bars of
    tests/test_gpu_objective.py::test_train_step_public_api (2e-5 relative; 1e-5 after one step of 2e-4)."""
    from oracle import ref_torch as rt, ref_train as ot
    T, B, lc, lr = 50, 2, 4, 2e-4
    m, W = cr.cond_model(T, B, W=cr.weights(seed=1), prediction="v", zero_terminal_snr=True)
    m.compile(loss="mse_sum", optimizer=SimpleNamespace(learning_rate=lr))
    g = torch.Generator().manual_seed(5)
    lat, noise = torch.randn(SHAPE, generator=g), torch.randn(SHAPE, generator=g)
    t = torch.tensor([T - 1, 3])
    ab = torch.from_numpy(cr.alpha_bar64(T, True))[t].reshape(-1, 1, 1, 1, 1)
    a, s = ab.sqrt(), (1 - ab).sqrt()
    assert float(a[0]) == 0.0 and float(s[0]) == 1.0
    ocfg = rt.UNetConfig(img_size=8, img_channels=4)
    Wd = {k: torch.from_numpy(v).double() for k, v in W.items()}
    Wg = {k: (v.clone().requires_grad_(True) if ot.is_trainable(k) else v) for k, v in Wd.items()}
    noisy = a * lat.double() + s * noise.double()
    pred = ot.unet_forward_train(Wg, ocfg, noisy, t, IDS)
    target = a * noise.double() - s * lat.double()
    per_ref = ((pred - target) ** 2).mean(-1).sum((1, 2, 3)) / (B * lc ** 4 * 1.0)
    lref = per_ref.sum()
    names = [k for k in Wg if Wg[k].requires_grad]
    grads = torch.autograd.grad(lref, [Wg[k] for k in names], allow_unused=True)
    gref = {k: (gr if gr is not None else torch.zeros_like(Wg[k])) for k, gr in zip(names, grads)}
    zeros = {k: torch.zeros_like(v) for k, v in gref.items()}
    Wn, mom, _ = ot.adam_step(Wd, gref, zeros, zeros, 1, lr)
    out = m.train_step((None, None, IDS), latents=lat, t=t, noise=noise)
    print(f"zero-terminal-SNR v, t = {t.tolist()}: loss {out['loss']:.8f} vs autograd {float(lref.detach()):.8f}")
    assert math.isfinite(out["loss"]) and np.allclose(out["loss"], float(lref.detach()), rtol=2e-5)
    per = m.trainer.sample_loss.cpu()
    assert torch.isfinite(per).all() and float(((per - per_ref.detach()).abs() / per_ref.detach()).max()) < 2e-5
    st = m.network.state_dict()
    worst = 0.0
    for k in mom:
        assert np.all(np.isfinite(st[k])), k
        sel = mom[k].abs() > 1e-3 * mom[k].abs().max().clamp_min(1e-30)
        if sel.any():
            worst = max(worst, float((torch.from_numpy(st[k]).double() - Wn[k]).abs()[sel].max()))
    print(f"after one step: max |w - w_ref| = {worst:.3e} (one step of {lr})")
    assert worst < 1e-5
    # min-SNR weighs the pure-noise timestep 0: the step is finite and that sample's loss exactly 0
    m.compile(loss="mse_sum", optimizer=SimpleNamespace(learning_rate=lr), loss_weighting="min_snr")
    out = m.train_step((None, None, IDS), latents=lat, t=t, noise=noise)
    per = m.trainer.sample_loss.cpu()
    assert math.isfinite(out["loss"]) and float(per[0]) == 0.0 and float(per[1]) > 0.0
