"""GPU tier of the DDIM sampler (dm3d_ddim_update, DiffusionModel.generate(sampler="ddim"), invert, ddim_step).

The float64 reference is tests/chain_reference.py's restatement of the DDIM update (Song et al., eq. 12) with eps from the CPU oracle
(oracle.ref_torch.unet_forward) and alpha_bar from the oracle's float32 Betas table, the table the kernels read.
"""
import os

import numpy as np
import pytest
import torch

import chain_reference as cr

pytestmark = pytest.mark.gpu
CHAIN_BAR = 2e-3        # the existing chain tests' bar (values in [-1, 1] + noise)


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    torch.set_num_threads(min(16, len(os.sched_getaffinity(0))))
    return torch.device("cuda:0")


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("clip", [True, False])
@pytest.mark.parametrize("eta", [0.0, 0.5, 1.0])
def test_kernel_matches_float64_restatement(dev, eta, clip, B):
    """ddim_step (mode 0) on random x / eps / injected z: interior steps and the k = 0 step (t_prev = -1), per-sample t."""
    T = 1000
    m, _ = cr.cond_model(T, B)
    ab = cr.oracle_alpha_bar(T).double()
    g = torch.Generator().manual_seed(17 + B)
    shape = (B, 8, 8, 8, 4)
    x, e, z = (torch.randn(shape, generator=g) for _ in range(3))
    for t, tp in (([500, 999, 20][:B], [480, 979, -1][:B]), ([5, 0, 1][:B], [-1, -1, 0][:B])):
        got = m.ddim_step(x, e, torch.tensor(t), torch.tensor(tp), eta, noise=z, clip_x0=clip).cpu()
        ref = torch.stack([cr.ddim64(x[b], e[b], float(ab[t[b]]), float(ab[tp[b]]) if tp[b] >= 0 else 1.0, eta, z[b], clip)
                           for b in range(B)])
        assert float(ref.abs().max()) < 20                              # O(1) values: the bar is absolute
        err = float((got.double() - ref).abs().max())
        assert err < 2e-6, (t, tp, err)
    # a NaN in eps reaches the output (through the clip as well)
    e_nan = e.clone()
    e_nan[0, 1, 2, 3, 1] = float("nan")
    got = m.ddim_step(x, e_nan, 500, 480, eta, noise=z, clip_x0=clip).cpu()
    assert torch.isnan(got[0, 1, 2, 3, 1]) and int(torch.isnan(got).sum()) == 1


def test_eta_one_full_schedule_equals_sample(dev):
    """eta = 1, S = T, no clip: one DDIM step is sample()'s posterior mean + sqrt(var) z.  (At small t the float32 tables disagree
    with each other: 1 - alpha_bar_t / alpha_bar_{t-1} in float32 holds beta_t to ~1e-3 relative at t = 1, so the identity is checked
    where they resolve beta, t >= 250 of T = 1000.)"""
    T, B = 1000, 2
    m, _ = cr.cond_model(T, B)
    g = torch.Generator().manual_seed(3)
    shape = (B, 8, 8, 8, 4)
    x, e, z = (torch.randn(shape, generator=g) for _ in range(3))
    for t in ([500, 999], [250, 750]):
        mean, var = m.sample(x, e, torch.tensor(t), shape)
        want = mean.cpu() + var.cpu().sqrt() * z
        got = m.ddim_step(x, e, torch.tensor(t), torch.tensor(t) - 1, 1.0, noise=z, clip_x0=False).cpu()
        assert float((got - want).abs().max()) < 1e-5


def test_philox_draws(dev):
    """x = eps = 0 leaves out = sigma z: the in-kernel draws repeat per seed, differ across seeds and timesteps, and are N(0, 1)."""
    from dm3d_amd.diffusion import ddim_coefficients
    T = 1000
    m, _ = cr.cond_model(T, 4)
    shape = (4, 32, 32, 32, 8)                                              # 1 048 576 draws
    zero = torch.zeros(shape, device=dev)
    a = m.ddim_step(zero, zero, 500, 480, 1.0, seed=11)
    b = m.ddim_step(zero, zero, 500, 480, 1.0, seed=11)
    c = m.ddim_step(zero, zero, 500, 480, 1.0, seed=12)
    d = m.ddim_step(zero, zero, 520, 500, 1.0, seed=11)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    sigma = float(np.float32(ddim_coefficients(m.b.alpha_bar, [500], [480], 1.0)[0, 4]))
    zz = (a.double() / sigma).cpu()
    assert abs(float(zz.mean())) < 1e-2 and abs(float(zz.std()) - 1) < 1e-2
    assert float((a - c).abs().max()) > 0 and float((zz - (c.double() / sigma).cpu()).std()) > 1.0     # independent streams
    # eta = 0: no noise at all
    assert torch.equal(m.ddim_step(zero, zero, 500, 480, 0.0, seed=11), zero)


@pytest.mark.parametrize("eta", [0.0, 0.5])
def test_conditional_chain_matches_float64(dev, eta):
    """8^3 x 4ch, T = 20, S = 5, B = 2 with both context ids (one per volume); eta = 0.5 with injected noise."""
    T, S, B = 20, 5, 2
    m, W = cr.cond_model(T, B)
    g = torch.Generator().manual_seed(21)
    shape = (B, 8, 8, 8, 4)
    x_T = torch.randn(shape, generator=g)
    noise = torch.randn((S,) + shape, generator=g) if eta else None
    ids = torch.tensor([[[1]], [[0]]])
    got = m.generate(shape, context_value=ids, x_T=x_T, noise=noise, sampler="ddim", num_steps=S, eta=eta).cpu()
    f = cr.oracle(W)
    ref = cr.chain64(lambda x, t: f(x, t, ids), cr.oracle_alpha_bar(T).double(), cr.schedule(T, S), x_T, "ddim", eta=eta, noise=noise)
    err = float((got.double() - ref).abs().max())
    print(f"DDIM chain eta={eta}: max abs difference {err:.2e}")
    assert err < CHAIN_BAR
    if eta == 0:                                                            # no noise: the seed does not matter
        again = m.generate(shape, context_value=ids, x_T=x_T, sampler="ddim", num_steps=S, seed=99)
        assert torch.equal(again.cpu(), got)


def test_unconditional_config1_chain(dev):
    """BASELINE config 1 (dm3d.py U-Net, 16^3 x 4ch, B = 1), T = 50, S = 10, eta = 0: the whole chain against float64."""
    T, S = 50, 10
    m, W = cr.uncond_model(T, size=16)
    x_T = torch.randn((1, 16, 16, 16, 4), generator=torch.Generator().manual_seed(4))
    got = m.generate((1, 16, 16, 16, 4), x_T=x_T, sampler="ddim", num_steps=S).cpu()
    f = cr.oracle(W, 16, conditional=False)
    ref = cr.chain64(f, cr.oracle_alpha_bar(T).double(), cr.schedule(T, S), x_T, "ddim")
    assert float((got.double() - ref).abs().max()) < CHAIN_BAR


def test_inversion_matches_float64(dev):
    """invert(): S - 1 deterministic steps tau_0 -> tau_{S-1} (sigma = 0, no clip), 8^3 x 4ch conditional, S = 5."""
    T, S, B = 20, 5, 2
    m, W = cr.cond_model(T, B)
    x0 = torch.rand((B, 8, 8, 8, 4), generator=torch.Generator().manual_seed(5)) * 2 - 1
    got = m.invert(x0, 1, num_steps=S).cpu()
    ab, taus, f = cr.oracle_alpha_bar(T).double(), cr.schedule(T, S), cr.oracle(W)
    ctx = torch.tensor([[[1]]])
    x = x0.double()
    for i in range(S - 1):
        x = cr.ddim64(x, f(x, taus[i], ctx), float(ab[taus[i]]), float(ab[taus[i + 1]]), clip=False)
    assert float((got.double() - x).abs().max()) < CHAIN_BAR
    assert torch.equal(m.invert(x0, 1, num_steps=1).cpu(), x0)             # S = 1: no step
    eager = m.invert(x0, 1, num_steps=S, use_graph=False).cpu()
    assert torch.equal(eager, got)


def test_graph_equals_eager_and_kinds_do_not_leak(dev):
    """A seeded DDIM chain is bitwise equal through the graph and eagerly, for two schedules through the one cached graph; a DDPM
    generate() on the same model afterwards equals one on a fresh model (graph cache and plan state are kept apart)."""
    T, B = 20, 2
    m, _ = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    for kw in (dict(num_steps=5, eta=0.5), dict(timesteps=[0, 3, 11, 19], eta=1.0, clip_x0=False), dict(num_steps=20)):
        a = m.generate(shape, context_value=0, seed=5, sampler="ddim", use_graph=True, **kw)
        b = m.generate(shape, context_value=0, seed=5, sampler="ddim", use_graph=False, **kw)
        c = m.generate(shape, context_value=0, seed=5, sampler="ddim", use_graph=True, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a, c) and torch.isfinite(a).all()
    d = m.generate(shape, context_value=0, seed=6, sampler="ddim", num_steps=5, eta=0.5)
    assert not torch.equal(d, m.generate(shape, context_value=0, seed=5, sampler="ddim", num_steps=5, eta=0.5))
    ddpm = m.generate(shape, context_value=0, seed=5)
    fresh, _ = cr.cond_model(T, B)
    torch.cuda.synchronize()
    assert torch.equal(ddpm, fresh.generate(shape, context_value=0, seed=5))
    # and a DDIM chain after the DDPM one still replays its own graph
    e = m.generate(shape, context_value=0, seed=5, sampler="ddim", num_steps=5, eta=0.5)
    assert torch.equal(e, m.generate(shape, context_value=0, seed=5, sampler="ddim", num_steps=5, eta=0.5, use_graph=False))
    # the public Sampler: S steps, then step() raises until reset()
    smp = m.sampler(shape, 0, seed=5, kind="ddim", num_steps=5, eta=0.5).prepare()
    smp.reset()
    for _ in range(5):
        smp.step()
    assert torch.equal(smp.plan.x, e)
    with pytest.raises(RuntimeError):
        smp.step()


def test_shards_equal_the_whole_batch(dev):
    """parallel.generate_sharded forwards sampler="ddim": B = 4 with a given x_T and eta = 0 equals two B = 2 halves.  The grids differ,
    so eps may differ in its last bits (the existing shard bar: 1e-6 of max |eps|).  One step passes eps on with weight a_eps = 0.58
    where the x0 estimate is clipped (max |x| ~ max |eps| here): 2e-6 of max |x|; the whole chain carries those differences through 10
    U-Net evaluations and is held to 1e-4."""
    from dm3d_amd import parallel
    T = 50
    m, _ = cr.cond_model(T, 4, size=16, C=8)
    shape = (4, 16, 16, 16, 8)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(8))
    for steps, bar in ((1, 2e-6), (None, 1e-4)):
        kw = dict(sampler="ddim", num_steps=10, steps=steps)
        full = parallel.generate_sharded(m, shape, 0, 1, seed=3, x_T=x_T, **kw)
        halves = torch.cat([m.generate((2,) + shape[1:], context_value=1, x_T=x_T[lo:lo + 2], **kw) for lo in (0, 2)], 0)
        torch.cuda.synchronize()
        assert float((halves - full).abs().max() / full.abs().max()) < bar, steps


def test_full_size_steps_match_oracle_and_b32_chain(dev):
    """32^3 x 8ch (h3): three DDIM steps of the S = 50 schedule at B = 2 against the oracle; a whole S = 50 chain of B = 32 through the
    graph is finite with the range guard quiet."""
    T, S, B, C = 1000, 50, 2, 8
    m, W = cr.cond_model(T, B, size=32, C=C, precision="h3")
    shape = (B, 32, 32, 32, C)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(12))
    ids = torch.tensor([[[1]], [[0]]])
    got = m.generate(shape, context_value=ids, x_T=x_T, sampler="ddim", num_steps=S, steps=3).cpu()
    f = cr.oracle(W, 32, C)
    ref = cr.chain64(lambda x, t: f(x, t, ids), cr.oracle_alpha_bar(T).double(), cr.schedule(T, S), x_T, "ddim", steps=3)
    err = float((got.double() - ref).abs().max())
    print(f"3 full-size DDIM steps: max abs difference {err:.2e}, max |x| {float(ref.abs().max()):.3f}")
    # near t = T-1 the x0 estimate is clipped almost everywhere and a step hands eps on to x with weight a_eps ~ 1 (the DDPM posterior
    # weighs it by beta-sized coefficients): the eps contract (1e-3 of max |ref|, BASELINE.json north_star) is the bar
    assert err / float(ref.abs().max()) < 1e-3
    # an untrained network is no denoiser: near t = T-1 a DDIM step hands eps on to x at weight ~1, and these synthetic weights have an
    # eps gain of ~3.5 per step (max |x| 4.5 -> 200 in the three steps above), so the chain would grow geometrically (the DDPM chain is
    # held by its clipped mean).  With the output conv scaled by 0.1 the gain stays below 1, as a trained eps-network's does.
    big, _ = cr.cond_model(T, 32, size=32, C=C, W=cr.weights(32, C, scale=0.1), precision="h3")
    out = big.generate((32, 32, 32, 32, C), context_value=1, seed=7, sampler="ddim", num_steps=S)   # check_range raises if flagged
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0 + 1e-6
