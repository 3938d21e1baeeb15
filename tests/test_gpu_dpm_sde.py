"""GPU tier of the stochastic DPM-Solver++(2M) sampler (dm3d_dpm_sde_update, DiffusionModel.dpm_step(sde_eta=), generate / edit /
sampler with "dpmpp_sde").

The float64 reference is tests/chain_reference.py's restatement of the update (Lu et al. 2022, the SDE form of DPM-Solver++(2M) in the
midpoint form) with the network from the CPU oracle (oracle.ref_torch.unet_forward) and alpha_bar from the
float32 table the kernels read.
"""
import math
import os

import numpy as np
import pytest
import torch

import chain_reference as cr

pytestmark = pytest.mark.gpu
CHAIN_BAR = 2e-3        # the existing chain tests' bar (values in [-1, 1] + noise)
KERNEL_BAR = 2e-6       # tests/test_gpu_dpm.py's kernel bar, scaled below by the coefficient mass of the row
T_C, S_C = 20, 5
SHAPE = (2, 8, 8, 8, 4)
IDS = torch.tensor([[[1]], [[0]]])
NEG = torch.tensor([[[0]], [[1]]])
F = np.float32


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return torch.device("cuda:0")


# ---- 1. the kernel against the float64 restatement -----------------------------------------------------------------------------------
CASES = [  # (t, t_prev, t_before or None), one entry per sample: tests/test_gpu_dpm.py's
    ([400, 300, 20], [380, 150, -1], None),                      # first order; sample 2 steps to clean
    ([400, 300, 20], [380, 150, -1], [420, 999, 25]),            # second order; sample 2 to clean (first order whatever the history)
    ([200, 50, 5], [100, 49, 0], [300, 51, 900]),                # second order: a wide, a unit and a tiny step after a far history
    ([5, 1, 0], [-1, 0, -1], None),
]
FLAT = (1, 4 * (65536 + 300))       # 65836 float4: 258 blocks' worth on a grid of 256, so a second trip of the loop with a ragged tail


@pytest.mark.parametrize("eta", [0.5, 1.0])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("clip", [True, False])
def test_kernel_matches_float64_restatement(dev, clip, B, eta):
    """dpm_step(sde_eta=, noise=z) (mode 0) on random x / eps / x0_prev / z with per-sample t.  The bar of x_next is KERNEL_BAR times the
    row's coefficient mass max(1, |c_x| + |c_0| + |c_1| + |c_z| max|z|); the x0 estimate is the plain dpm_step's bitwise."""
    T = 1000
    m, _ = cr.cond_model(T, B)
    ab = cr.alpha_bar64(T)
    g = torch.Generator().manual_seed(131 + B)
    for shape in [(B, 8, 8, 8, 4), (B, 4, 4, 4, 4)] + ([FLAT] if B == 1 else []):
        x, e, h, z = (torch.randn(shape, generator=g) for _ in range(4))
        dx, de, dh, dz = (v.cuda() for v in (x, e, h, z))
        keep = [v.clone() for v in (dx, de, dh, dz)]
        zmax = float(z.abs().max())
        for t, tp, tb in CASES:
            t, tp = t[:B], tp[:B]
            tb = None if tb is None else tb[:B]
            hist = () if tb is None else (dh, torch.tensor(tb))
            got, x0 = m.dpm_step(dx, de, torch.tensor(t), torch.tensor(tp), *hist, clip_x0=clip, sde_eta=eta, noise=dz)
            _, x0_ode = m.dpm_step(dx, de, torch.tensor(t), torch.tensor(tp), *hist, clip_x0=clip)
            torch.cuda.synchronize()
            assert torch.equal(x0, x0_ode)
            got = got.cpu()
            for b in range(B):
                p = -1 if tb is None else tb[b]
                ref, ref0 = cr.dpm64(x[b], e[b], ab, t[b], tp[b], p, h[b], clip, eta, z[b])
                assert float(ref.abs().max()) < 20 and float(ref0.abs().max()) < 20               # O(1) values: the bar is absolute
                c = cr.dpm_row64(ab, t[b], tp[b], p, eta)
                assert (c[3] != 0) == (tp[b] >= 0) and (c[2] != 0) == (p >= 0 and tp[b] >= 0)
                bar = KERNEL_BAR * max(1.0, abs(c[0]) + abs(c[1]) + abs(c[2]) + abs(c[3]) * zmax)
                err = float((got[b].double() - ref).abs().max())
                print(f"shape={shape} clip={clip} eta={eta} t={t[b]} -> {tp[b]} (before {p}): x_next err {err:.2e} (bar {bar:.2e})")
                assert err < bar, (shape, t, tp, tb, b)
                if tp[b] < 0:
                    assert torch.equal(got[b], x0[b].cpu())                                        # the clean row hands on x0 bitwise
        assert all(torch.equal(a, b) for a, b in zip((dx, de, dh, dz), keep))                      # mode 0 leaves every input alone


# ---- 2. eta = 0 is the ODE solver bitwise ---------------------------------------------------------------------------------------------
def test_eta_zero_is_the_ode_solver_bitwise(dev):
    T, B = 1000, 3
    m, _ = cr.cond_model(T, B)
    g = torch.Generator().manual_seed(17)
    x, e, h = (torch.randn((B, 8, 8, 8, 4), generator=g).cuda() for _ in range(3))
    nan = torch.full_like(x, float("nan"))
    for clip in (True, False):
        for t, tp, tb in CASES:
            hist = () if tb is None else (h, torch.tensor(tb))
            want = m.dpm_step(x, e, torch.tensor(t), torch.tensor(tp), *hist, clip_x0=clip)
            for kw in (dict(), dict(seed=3), dict(noise=nan)):                                 # c_z = 0: nothing is drawn, noise is not read
                got = m.dpm_step(x, e, torch.tensor(t), torch.tensor(tp), *hist, clip_x0=clip, sde_eta=0.0, **kw)
                assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (clip, t, kw)
    m, _ = cr.cond_model(T_C, 2)
    x_T = torch.randn(SHAPE, generator=g)
    for kw in (dict(num_steps=S_C), dict(num_steps=7, solver_order=1, clip_x0=False), dict(num_steps=6, lower_order_final=False)):
        for use_graph in (True, False):
            want = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="dpmpp", use_graph=use_graph, **kw)
            got = m.generate(SHAPE, context_value=IDS, x_T=x_T, sampler="dpmpp_sde", sde_eta=0.0, use_graph=use_graph, **kw)
            assert torch.equal(got, want) and torch.isfinite(got).all(), (kw, use_graph)
    assert {"dpmpp", "dpmpp+sde"} <= {k[1] for k in m._graphs}


# ---- 3. the Philox draws --------------------------------------------------------------------------------------------------------------
def test_philox_draws(dev):
    """x = pred = 0 without the clip leaves out = c_z z: the in-kernel draws repeat per seed, differ across seeds and timesteps, are not
    ddim_step's draws at the same seed and timestep (the stream constant is this kernel's own), and are N(0, 1)."""
    from dm3d_amd.diffusion import ddim_coefficients, dpm_sde_coefficients
    T = 1000
    m, _ = cr.cond_model(T, 4)
    zero = torch.zeros((4, 32, 32, 32, 8), device=dev)                      # 1 048 576 draws
    step = lambda t, tp, seed: m.dpm_step(zero, zero, t, tp, clip_x0=False, sde_eta=1.0, seed=seed)[0]
    a, b, c, d = step(500, 480, 11), step(500, 480, 11), step(500, 480, 12), step(520, 500, 11)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    c_z = float(F(dpm_sde_coefficients(m.b.alpha_bar, [500], [480], [-1], 2, 1.0)[0, 3]))
    assert c_z > 0
    zz = (a.double() / c_z).cpu()
    print(f"dpm_sde draws: mean {float(zz.mean()):+.2e}, std {float(zz.std()):.5f}")
    assert abs(float(zz.mean())) < 1e-2 and abs(float(zz.std()) - 1) < 1e-2
    assert float((zz - (c.double() / c_z).cpu()).std()) > 1.0                  # independent streams across seeds
    c_z2 = float(F(dpm_sde_coefficients(m.b.alpha_bar, [520], [500], [-1], 2, 1.0)[0, 3]))
    assert float((zz - (d.double() / c_z2).cpu()).std()) > 1.0                 # and across timesteps
    ddim = m.ddim_step(zero, zero, 500, 480, 1.0, clip_x0=False, seed=11)
    sigma = float(F(ddim_coefficients(m.b.alpha_bar, [500], [480], 1.0)[0, 4]))
    assert float((zz - (ddim.double() / sigma).cpu()).std()) > 1.0             # and from the DDIM kernel's stream
    assert torch.equal(m.dpm_step(zero, zero, 500, 480, clip_x0=False, sde_eta=0.0, seed=11)[0], zero)      # eta = 0: no noise at all
    assert torch.equal(step(500, -1, 11), zero)                                # the row to clean draws none


# ---- 4. chains against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("conditional", [True, False])
def test_chain_matches_float64(dev, conditional, clip, order):
    """8^3 x 4ch, T = 20, S = 5, B = 2 (conditional: one context id per volume), eta = 1 with injected x_T and noise."""
    g = torch.Generator().manual_seed(51)
    x_T = torch.randn(SHAPE, generator=g)
    noise = torch.randn((S_C,) + SHAPE, generator=g)
    kw = dict(x_T=x_T, noise=noise, sampler="dpmpp_sde", num_steps=S_C, clip_x0=clip, solver_order=order)
    if conditional:
        m, W = cr.cond_model(T_C, 2)
        ckw = dict(context_value=IDS)
        f = cr.oracle(W)
        net = lambda x, t: f(x, t, IDS)
    else:
        m, W = cr.uncond_model(T_C, 2)
        ckw = {}
        net = cr.oracle(W, conditional=False)
    got = m.generate(SHAPE, **ckw, **kw).cpu()
    ref = cr.chain64(net, cr.alpha_bar64(T_C), cr.schedule(T_C, S_C), x_T, eta=1.0, noise=noise, order=order, clip=clip)
    err = float((got.double() - ref).abs().max())
    print(f"dpmpp_sde chain conditional={conditional} clip={clip} order={order}: max abs difference {err:.2e}, max |x| {float(ref.abs().max()):.3f}")
    assert torch.isfinite(got).all() and err < CHAIN_BAR
    # the noise does something, and so does the order
    ode = m.generate(SHAPE, x_T=x_T, sampler="dpmpp", num_steps=S_C, clip_x0=clip, solver_order=order, **ckw).cpu()
    assert float((got - ode).abs().max()) > 1e-2
    if order == 2:
        assert not torch.equal(got, m.generate(SHAPE, **ckw, **dict(kw, solver_order=1)).cpu())
    # another eta, the same z: its own float64 chain
    got = m.generate(SHAPE, sde_eta=0.5, **ckw, **kw).cpu()
    ref = cr.chain64(net, cr.alpha_bar64(T_C), cr.schedule(T_C, S_C), x_T, eta=0.5, noise=noise, order=order, clip=clip)
    err = float((got.double() - ref).abs().max())
    print(f"  sde_eta=0.5: max abs difference {err:.2e}")
    assert err < CHAIN_BAR


@pytest.mark.parametrize("strength", [1.0, 0.6])
def test_edit_chain_matches_float64(dev, strength):
    """edit(sampler="dpmpp_sde") with a half mask, injected noise and known_noise: the blend follows every update, the history stays
    unblended, kept voxels are x0 bitwise; strength 0.6 keeps 3 steps and starts first order from q_sample(x0, sched[2])."""
    from dm3d_amd.diffusion import edit_steps, latent_mask
    m, W = cr.cond_model(T_C, 2)
    g = torch.Generator().manual_seed(61)
    x0 = torch.rand(SHAPE, generator=g) * 2 - 1
    n = edit_steps(strength, S_C)
    sched = cr.schedule(T_C, S_C)[:n]
    assert n == (5 if strength == 1.0 else 3)
    noise = torch.randn((n,) + SHAPE, generator=g)
    known_noise = torch.randn((n + 1,) + SHAPE, generator=g)
    mask = cr.half_mask(2, 16, slab=True)
    ab = cr.alpha_bar64(T_C)
    kw = dict(mask=mask, strength=strength, seed=13, sampler="dpmpp_sde", num_steps=S_C)
    if n == S_C:
        x_start = m.edit(x0, IDS, steps=0, **kw).cpu()                    # generate()'s x_T under the seed
    else:
        x_start = cr.known64(x0, ab, sched[-1], known_noise[n])
    got = m.edit(x0, IDS, noise=noise, known_noise=known_noise, **kw).cpu()
    f = cr.oracle(W)
    keep = 1 - latent_mask(mask, SHAPE)
    w = keep.double().unsqueeze(-1)
    blend = cr.edit_blend64(x0, ab, sched, keep, known_noise)
    ref = cr.chain64(lambda x, t: f(x, t, IDS), ab, sched, x_start, eta=1.0, noise=noise, blend=blend)
    err = float((got.double() - ref).abs().max())
    print(f"dpmpp_sde edit chain strength={strength}: max abs difference {err:.2e}")
    assert err < CHAIN_BAR
    kept, regen = (w == 1).expand(SHAPE), (w == 0).expand(SHAPE)
    assert torch.equal(got[kept], x0[kept])                               # the kept region is x0 bitwise
    assert float((got[regen] - x0[regen]).abs().mean()) > 1e-2            # the regenerated one is new
    # seeded runs repeat, through the graph and eagerly, and all-regenerate at strength 1 is generate()
    a, b = m.edit(x0, IDS, **kw), m.edit(x0, IDS, use_graph=False, **kw)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and torch.equal(a.cpu()[kept], x0[kept])
    if n == S_C:
        want = m.generate(SHAPE, context_value=IDS, seed=13, sampler="dpmpp_sde", num_steps=S_C)
        assert torch.equal(m.edit(x0, IDS, seed=13, sampler="dpmpp_sde", num_steps=S_C), want)
    assert "dpmpp-edit+sde" in {k[1] for k in m._graphs}


@pytest.mark.parametrize("phi", [0.0, 0.7])
def test_guided_chain_matches_float64(dev, phi):
    """w = 3 with per-volume contexts; the draws are those of the unguided chain of the same volumes."""
    m, W = cr.cond_model(T_C, 2)
    g = torch.Generator().manual_seed(71)
    x_T = torch.randn(SHAPE, generator=g)
    noise = torch.randn((S_C,) + SHAPE, generator=g)
    f, w = cr.oracle(W), 3.0
    kw = dict(context_value=IDS, x_T=x_T, sampler="dpmpp_sde", num_steps=S_C)
    gkw = dict(guidance_scale=w, negative_context=NEG, guidance_rescale=phi)
    got = m.generate(SHAPE, noise=noise, **gkw, **kw).cpu()
    ref = cr.chain64(lambda x, t: cr.guide64(f(x, t, IDS), f(x, t, NEG), w, phi), cr.alpha_bar64(T_C), cr.schedule(T_C, S_C), x_T,
                     eta=1.0, noise=noise)
    err = float((got.double() - ref).abs().max())
    print(f"guided dpmpp_sde phi={phi} chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR
    assert not torch.equal(got, m.generate(SHAPE, noise=noise, **kw).cpu())                 # guidance does something
    a, b = m.generate(SHAPE, seed=4, **gkw, **kw), m.generate(SHAPE, seed=4, use_graph=False, **gkw, **kw)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert "dpmpp-cfg+sde" in {k[1] for k in m._graphs}                 # (the unguided call above injects noise: it runs eagerly)


def test_thresholded_chain_matches_float64(dev):
    """The output conv scaled by 3 (tests/test_gpu_threshold.py's weights): the float64 chain's bound exceeds 1 at some step."""
    m, W = cr.cond_model(T_C, 2, W=cr.weights(scale=3.0))
    g = torch.Generator().manual_seed(81)
    x_T = torch.randn(SHAPE, generator=g) * 1.5
    noise = torch.randn((S_C,) + SHAPE, generator=g)
    f, bounds = cr.oracle(W), []
    kw = dict(context_value=IDS, x_T=x_T, sampler="dpmpp_sde", num_steps=S_C)
    tkw = dict(dynamic_threshold=0.9, threshold_max=4.0)
    got = m.generate(SHAPE, noise=noise, **tkw, **kw).cpu()
    ref = cr.chain64(lambda x, t: f(x, t, IDS), cr.alpha_bar64(T_C), cr.schedule(T_C, S_C), x_T, eta=1.0, noise=noise,
                     thr=(0.9, 4.0, bounds))
    err = float((got.double() - ref).abs().max())
    print(f"thresholded dpmpp_sde chain: max abs difference {err:.2e}; s per step {[round(s, 3) for s in bounds]}")
    assert len(bounds) == 2 * S_C and max(bounds) > 1.0
    assert torch.isfinite(got).all() and err < CHAIN_BAR
    assert not torch.equal(m.generate(SHAPE, noise=noise, **kw).cpu(), got)
    a, b = m.generate(SHAPE, seed=4, **tkw, **kw), m.generate(SHAPE, seed=4, use_graph=False, **tkw, **kw)
    assert torch.equal(a, b) and torch.isfinite(a).all()
    assert "dpmpp+sde+thr" in {k[1] for k in m._graphs}


# ---- 5. zero-terminal-SNR models ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["v", "x0"])
def test_zero_terminal_snr_first_step(dev, kind):
    """dpm_step(prediction=, sde_eta=) from alpha_bar = 0: the row is (0, alpha_t, 0, sigma_t), so the result is alpha_t x0 + sigma_t z
    with x0 the clipped estimate of the raw prediction, whatever x holds."""
    T = 1000
    m, _ = cr.cond_model(T, 2, prediction=kind, zero_terminal_snr=True)
    ab = cr.alpha_bar64(T, True)
    assert ab[T - 1] == 0.0 and m.b.alpha_bar[T - 1] == 0.0
    g = torch.Generator().manual_seed(91)
    x, p, z = (torch.randn(SHAPE, generator=g) for _ in range(3))
    for eta in (0.5, 1.0):
        for tp in (900, 998):
            out, x0 = m.dpm_step(x, p, T - 1, tp, prediction=kind, sde_eta=eta, noise=z)
            other, _ = m.dpm_step(x * 3 + 1, p, T - 1, tp, prediction=kind, sde_eta=eta, noise=z)
            torch.cuda.synchronize()
            want0 = (-p if kind == "v" else p).double().clamp(-1, 1)                       # v: x0 = 0 x - 1 v
            want = math.sqrt(ab[tp]) * want0 + math.sqrt(1 - ab[tp]) * z.double()
            bar = KERNEL_BAR * max(1.0, math.sqrt(ab[tp]) + math.sqrt(1 - ab[tp]) * float(z.abs().max()))
            err = float((out.cpu().double() - want).abs().max())
            print(f"{kind} first step 999 -> {tp} eta={eta}: err {err:.2e} (bar {bar:.2e})")
            assert torch.isfinite(out).all() and err < bar
            assert float((x0.cpu().double() - want0).abs().max()) < KERNEL_BAR
            assert torch.equal(out, other)                                                 # nothing of x survives


@pytest.mark.parametrize("kind", ["v", "x0"])
def test_zero_terminal_snr_chains(dev, kind):
    """The native chain against float64 with injected x_T and noise; every intermediate state finite; seeded graph and eager chains
    bitwise equal, plain, guided, thresholded and edit."""
    m, W = cr.cond_model(T_C, 2, prediction=kind, zero_terminal_snr=True)
    g = torch.Generator().manual_seed(101)
    x_T = torch.randn(SHAPE, generator=g)
    noise = torch.randn((S_C,) + SHAPE, generator=g)
    sched, ab = cr.schedule(T_C, S_C), cr.alpha_bar64(T_C, True)
    assert ab[sched[-1]] == 0.0
    f = cr.oracle(W)
    got = m.generate(SHAPE, context_value=IDS, x_T=x_T, noise=noise, sampler="dpmpp_sde", num_steps=S_C).cpu()
    ref = cr.chain64(lambda x, t: f(x, t, IDS), ab, sched, x_T, kind=kind, eta=1.0, noise=noise)
    err = float((got.double() - ref).abs().max())
    print(f"zero-terminal-SNR {kind} model, dpmpp_sde: max abs difference {err:.2e}")
    assert torch.isfinite(got).all() and err < CHAIN_BAR
    smp = m.sampler(SHAPE, IDS, kind="dpmpp_sde", num_steps=S_C, seed=7)
    assert smp._pred_d is None and smp.native                              # the native chain launches no conversion
    smp.reset(x_T)
    for _ in range(smp.n_steps):
        smp.step()
        assert torch.isfinite(smp.x).all()
    x0 = torch.rand(SHAPE, generator=g) * 2 - 1
    kw = dict(seed=7, sampler="dpmpp_sde", num_steps=S_C)
    variants = [dict(), dict(guidance_scale=3.0, guidance_rescale=0.7, negative_context=NEG), dict(dynamic_threshold=0.9, threshold_max=4.0)]
    for extra in variants:
        a = m.generate(SHAPE, context_value=IDS, use_graph=True, **kw, **extra)
        b = m.generate(SHAPE, context_value=IDS, use_graph=False, **kw, **extra)
        assert torch.equal(a, b) and torch.isfinite(a).all(), extra
    a, b = (m.edit(x0, IDS, mask=cr.half_mask(2, 16, slab=True), use_graph=ug, **kw) for ug in (True, False))
    assert torch.equal(a, b) and torch.isfinite(a).all() and torch.equal(a.cpu()[:, 5:], x0[:, 5:])
    assert {"dpmpp+sde+frame", "dpmpp-cfg+sde+frame", "dpmpp+sde+thr+frame", "dpmpp-edit+sde+frame"} <= {k[1] for k in m._graphs}


def test_plain_schedule_v_model_converts_first(dev):
    """A v-model on the plain schedule converts to eps after the U-Net, as every chain of it does: its graph kind says so."""
    m, W = cr.cond_model(T_C, 2, prediction="v")
    g = torch.Generator().manual_seed(111)
    x_T = torch.randn(SHAPE, generator=g)
    noise = torch.randn((S_C,) + SHAPE, generator=g)
    f = cr.oracle(W)
    got = m.generate(SHAPE, context_value=IDS, x_T=x_T, noise=noise, sampler="dpmpp_sde", num_steps=S_C).cpu()
    ref = cr.chain64(lambda x, t: f(x, t, IDS), cr.alpha_bar64(T_C), cr.schedule(T_C, S_C), x_T, kind="v", eta=1.0, noise=noise)
    err = float((got.double() - ref).abs().max())
    print(f"plain-schedule v model, dpmpp_sde: max abs difference {err:.2e}")
    assert err < CHAIN_BAR
    a, b = (m.generate(SHAPE, context_value=IDS, seed=2, sampler="dpmpp_sde", num_steps=S_C, use_graph=ug) for ug in (True, False))
    assert torch.equal(a, b) and "dpmpp+sde+pred" in {k[1] for k in m._graphs}


# ---- 6. graphs --------------------------------------------------------------------------------------------------------------------------
def test_graph_equals_eager_repeats_and_serves_every_schedule_and_eta(dev):
    m, _ = cr.cond_model(T_C, 2)
    counts = []
    runs = [dict(num_steps=5), dict(num_steps=8, sde_eta=0.5), dict(timesteps=[0, 3, 11, 19], clip_x0=False), dict(num_steps=20, sde_eta=2.0),
            dict(num_steps=7, lower_order_final=False), dict(num_steps=6, solver_order=1, sde_eta=0.5)]
    outs = []
    for kw in runs:
        a = m.generate(SHAPE, context_value=IDS, seed=5, sampler="dpmpp_sde", use_graph=True, **kw)
        counts.append(len(m._graphs))
        b = m.generate(SHAPE, context_value=IDS, seed=5, sampler="dpmpp_sde", use_graph=False, **kw)
        c = m.generate(SHAPE, context_value=IDS, seed=5, sampler="dpmpp_sde", use_graph=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.isfinite(a).all(), kw
        outs.append(a)
    assert counts == [1] * len(runs) and {k[1] for k in m._graphs} == {"dpmpp+sde"}
    base = dict(context_value=IDS, sampler="dpmpp_sde", num_steps=5)
    assert not torch.equal(outs[0], m.generate(SHAPE, seed=5, sde_eta=0.5, **base))                  # eta is read
    assert not torch.equal(outs[0], m.generate(SHAPE, seed=6, **base))                               # and so is the seed


def test_sde_and_ode_chains_never_replay_each_other(dev):
    """An SDE chain and an ODE chain (and a DDIM chain) alternated on one plan: each is bitwise what it is alone on a fresh model."""
    calls = {"sde": dict(sampler="dpmpp_sde", num_steps=5), "ode": dict(sampler="dpmpp", num_steps=5),
             "ddim": dict(sampler="ddim", num_steps=5, eta=1.0)}
    alone = {k: cr.cond_model(T_C, 2)[0].generate(SHAPE, context_value=0, seed=5, **kw) for k, kw in calls.items()}
    assert not torch.equal(alone["sde"], alone["ode"]) and not torch.equal(alone["sde"], alone["ddim"])
    m, _ = cr.cond_model(T_C, 2)
    for k in ("ode", "sde", "ode", "ddim", "sde", "sde", "ode", "ddim"):
        got = m.generate(SHAPE, context_value=0, seed=5, **calls[k])
        torch.cuda.synchronize()
        assert torch.equal(got, alone[k]), k
    assert {"dpmpp", "dpmpp+sde", "ddim"} <= {k[1] for k in m._graphs}


def test_nan_reaches_its_element_only(dev):
    m, _ = cr.cond_model(1000, 2)
    g = torch.Generator().manual_seed(8)
    x, e, h, z = (torch.randn(SHAPE, generator=g) for _ in range(4))
    e_nan = e.clone()
    e_nan[0, 1, 2, 3, 1] = float("nan")
    for clip in (True, False):
        for hist in ((), (h, 520)):
            for kw in (dict(noise=z), dict(seed=3)):
                out, x0 = m.dpm_step(x, e_nan, 500, 480, *hist, clip_x0=clip, sde_eta=1.0, **kw)
                for v in (out.cpu(), x0.cpu()):
                    assert torch.isnan(v[0, 1, 2, 3, 1]) and int(torch.isnan(v).sum()) == 1
    z_nan = z.clone()
    z_nan[1, 0, 0, 0, 0] = float("nan")
    out, x0 = m.dpm_step(x, e, 500, 480, sde_eta=1.0, noise=z_nan)
    assert torch.isnan(out[1, 0, 0, 0, 0]) and int(torch.isnan(out).sum()) == 1 and not torch.isnan(x0).any()
    out, x0 = m.dpm_step(x, e, 500, -1, sde_eta=1.0, noise=z_nan)                                    # to clean: the noise is not read
    assert not torch.isnan(out).any() and torch.equal(out, x0)
