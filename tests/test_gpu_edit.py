"""GPU tier of latent editing (dm3d_edit_update, DiffusionModel.q_sample, DiffusionModel.edit): inpainting with RePaint's
replacement step and image-to-image (SDEdit) starts, for the DDPM and DDIM chains.

The float64 reference is tests/chain_reference.py's restatement of the known-latent step and of the DDIM update, the oracle's DDPM
step (oracle.ref_torch.ddpm_step, in float64) and eps from the CPU oracle (oracle.ref_torch.unet_forward), with alpha_bar from the
oracle's float32 Betas table, the table the kernels read.
"""
import ctypes
import math
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


def test_kernel_matches_float64_restatement(dev):
    """q_sample (mode 0) and the blend (mode 1) on random x / x0 / fractional w / injected z, per-sample rows and the clean row."""
    from oracle import ref_torch as rt
    T, B = 1000, 3
    m, _ = cr.cond_model(T, B)
    ab = cr.oracle_alpha_bar(T).double()
    g = torch.Generator().manual_seed(31)
    for shape in ((B, 8, 8, 8, 4), (B, 4, 4, 4, 8), (B, 4, 4, 4, 2), (B, 4, 4, 4, 1)):        # C % 4 != 0: one lane, several voxels
        x, x0, z = (torch.randn(shape, generator=g) for _ in range(3))
        keep = torch.rand(shape[:4], generator=g)
        keep[keep < 0.25] = 0.0
        keep[keep > 0.75] = 1.0
        for t in ([500, 999, 0], [-1, 3, 250], [-1, -1, -1]):
            q = m.q_sample(x0, torch.tensor(t), noise=z).cpu()
            got = m._edit_call(x0, torch.tensor(t), 1, x=x, keep=keep, noise=z).cpu()
            for bb in range(B):
                kn = cr.known64(x0[bb], ab, t[bb], z[bb])
                err = float((q[bb].double() - kn).abs().max())
                assert err < 2e-6, (shape, t, err)
                if t[bb] < 0:
                    assert torch.equal(q[bb], x0[bb])                               # clean: x0 bitwise
                w = keep[bb].double().unsqueeze(-1)
                ref = w * kn + (1 - w) * x[bb].double()
                assert float((got[bb].double() - ref).abs().max()) < 2e-6, (shape, t)
            w = keep.unsqueeze(-1).expand(shape)
            assert torch.equal(got[w == 0], x[w == 0])                              # w = 0: untouched
            assert torch.equal(got[w == 1], q[w == 1])                              # w = 1: known_t bitwise
    # the reference's forward noising order, against the oracle's q_sample on its own (fp32-rounded) tables
    x0, z = torch.randn((B, 8, 8, 8, 4), generator=g), torch.randn((B, 8, 8, 8, 4), generator=g)
    t = torch.tensor([7, 400, 999])
    assert float((m.q_sample(x0, t, z).cpu() - rt.q_sample(rt.Betas(T), x0, t, z)).abs().max()) < 1e-6
    # a NaN in x survives where it is regenerated, a NaN in x0 reaches the kept voxels only
    shape = (B, 8, 8, 8, 4)
    xn, x0n = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    keep = torch.zeros(shape[:4])
    keep[0, 0, 0, 0] = 1.0
    xn[1, 1, 1, 1, 0] = float("nan")
    x0n[0, 0, 0, 0, 0] = float("nan")
    x0n[2, 2, 2, 2, 0] = float("nan")
    got = m._edit_call(x0n, 5, 1, x=xn, keep=keep).cpu()
    assert int(torch.isnan(got).sum()) == 2 and torch.isnan(got[1, 1, 1, 1, 0]) and torch.isnan(got[0, 0, 0, 0, 0])


def _draws(m, dev, seed, t, kind, shape):
    """The N(0,1) draws of one kernel, recovered from x0 = x = eps = 0."""
    from dm3d_amd import _lib
    from dm3d_amd.diffusion import ddim_coefficients, edit_levels
    zero = torch.zeros(shape, device=dev)
    if kind == "edit":
        return m.q_sample(zero, t, seed=seed).double() / float(np.float32(edit_levels(m.b.alpha_bar, [t])[0, 1]))
    if kind == "ddim":
        sigma = float(np.float32(ddim_coefficients(m.b.alpha_bar, [t], [t - 20], 1.0)[0, 4]))
        return m.ddim_step(zero, zero, t, t - 20, 1.0, seed=seed).double() / sigma
    x = torch.zeros(shape, device=dev)
    tidx = torch.full((shape[0],), t, dtype=torch.int32, device=dev)
    d = m._ddpm_desc(x, zero, tidx, 1, seed=seed)
    _lib.check(_lib.lib().dm3d_ddpm_update(ctypes.byref(d), torch.cuda.current_stream().cuda_stream), "ddpm_update")
    b = m.b
    var = (1 - b.alpha_bar_prev[t]) * b.beta[t] / (1 - b.alpha_bar[t])
    return x.double() / math.exp(0.5 * math.log(var))


def test_philox_draws(dev):
    """x0 = 0 leaves q_sample = sqrt(1-a) z: the draws repeat per seed, differ across seeds and levels, are N(0, 1), and are not the
    DDPM or DDIM update's draws under the same key and timestep."""
    T = 1000
    m, _ = cr.cond_model(T, 4)
    shape = (4, 32, 32, 32, 8)                                              # 1 048 576 draws
    a = _draws(m, dev, 11, 500, "edit", shape)
    b = _draws(m, dev, 11, 500, "edit", shape)
    c = _draws(m, dev, 12, 500, "edit", shape)
    d = _draws(m, dev, 11, 480, "edit", shape)
    torch.cuda.synchronize()
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    for other in (c, d):
        assert abs(float(((a - other) ** 2).mean()) - 2.0) < 2e-2             # independent: var(a - b) = 2
    za = a.cpu()
    assert abs(float(za.mean())) < 1e-2 and abs(float(za.std()) - 1) < 1e-2
    for kind in ("ddpm", "ddim"):
        zo = _draws(m, dev, 11, 500, kind, shape).cpu()
        assert abs(float(zo.std()) - 1) < 1e-2
        corr = float((za * zo).mean() / (za.std() * zo.std()))
        assert abs(corr) < 1e-2 and not torch.equal(za, zo), kind
    # the clean level draws nothing: x0 = 0 stays 0
    assert torch.equal(m.q_sample(torch.zeros(shape, device=dev), -1, seed=11), torch.zeros(shape, device=dev))


@pytest.mark.parametrize("kind,kw", [("ddpm", {}), ("ddim", dict(num_steps=5)), ("ddim", dict(num_steps=5, eta=0.5))])
def test_all_regenerate_at_strength_one_equals_generate(dev, kind, kw):
    T, B = 20, 2
    m, _ = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    x0 = torch.rand(shape, generator=torch.Generator().manual_seed(2)) * 2 - 1
    ids = torch.tensor([[[1]], [[0]]])
    want = m.generate(shape, context_value=ids, seed=9, sampler=kind, **kw)
    for mask in (None, torch.ones((B, 8, 8, 8)), torch.ones((1, 32, 32, 32, 1))):
        got = m.edit(x0, ids, mask=mask, seed=9, sampler=kind, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, want)
    assert not torch.equal(m.edit(x0, ids, seed=10, sampler=kind, **kw), want)


@pytest.mark.parametrize("kind,kw", [("ddpm", {}), ("ddim", dict(num_steps=5, eta=0.5))])
@pytest.mark.parametrize("strength", [1.0, 0.45])
def test_all_keep_returns_x0(dev, kind, kw, strength):
    T, B = 20, 2
    m, _ = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    x0 = torch.rand(shape, generator=torch.Generator().manual_seed(3)) * 2 - 1
    x0[0, 0, 0, 0, 0] = -0.0
    got = m.edit(x0, 1, mask=torch.zeros((1, 16, 16, 16)), strength=strength, seed=4, sampler=kind, **kw)
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), x0) and torch.equal(got.cpu().view(torch.int32), x0.view(torch.int32))


@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
@pytest.mark.parametrize("strength", [1.0, 0.5])
def test_conditional_half_mask_chain_matches_float64(dev, kind, eta, strength):
    """8^3 x 4ch, T = 20 (DDIM: S = 5), B = 2 with both context ids, injected noise and known_noise."""
    from dm3d_amd.diffusion import edit_steps, latent_mask
    T, S, B = 20, 5, 2
    m, W = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    g = torch.Generator().manual_seed(41)
    x0 = torch.rand(shape, generator=g) * 2 - 1
    full = list(range(T)) if kind == "ddpm" else cr.schedule(T, S)
    n = edit_steps(strength, len(full))
    sched = full[:n]
    noise = torch.randn((n,) + shape, generator=g)
    known_noise = torch.randn((n + 1,) + shape, generator=g)
    x_T = torch.randn(shape, generator=g)
    ids = torch.tensor([[[1]], [[0]]])
    mask = cr.half_mask(B, 16, slab=True)
    b = cr.oracle_betas(T)
    ab = b.alpha_bar.double()
    kw = dict(sampler=kind) if kind == "ddpm" else dict(sampler=kind, num_steps=S, eta=eta)
    if n == len(full):
        # the start is generate()'s x_T under the seed: take it from a zero-step chain
        x_start = m.edit(x0, ids, mask=mask, seed=13, steps=0, **kw).cpu()
    else:
        x_start = cr.known64(x0, ab, sched[-1], known_noise[n])
    got = m.edit(x0, ids, mask=mask, strength=strength, seed=13, noise=noise, known_noise=known_noise, **kw).cpu()
    f = cr.oracle(W)
    keep = 1 - latent_mask(mask, shape)
    ref = cr.chain64(lambda x, t: f(x, t, ids), ab, sched, x_start, kind, eta=eta, noise=noise,
                     blend=cr.edit_blend64(x0, ab, sched, keep, known_noise), betas=b)
    err = float((got.double() - ref).abs().max())
    print(f"{kind} eta={eta} strength={strength} edit chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR
    kept = (keep == 1).unsqueeze(-1).expand(shape)
    regen = (keep == 0).unsqueeze(-1).expand(shape)
    assert torch.equal(got[kept], x0[kept])                                 # the kept region is x0 bitwise
    assert float((got[regen] - x0[regen]).abs().mean()) > 1e-2              # the regenerated one is new
    if n < len(full):                                                       # the start draw is the kernel's: seeded run repeats
        a = m.edit(x0, ids, mask=mask, strength=strength, seed=13, **kw)
        b = m.edit(x0, ids, mask=mask, strength=strength, seed=13, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.equal(a.cpu()[kept], x0[kept])


def test_graph_equals_eager_and_kinds_do_not_leak(dev):
    """Seeded edits are bitwise equal through the graph and eagerly, across masks, strengths and schedules through the one cached
    graph per kind; edit and generate interleaved on one plan give the bytes of fresh runs."""
    T, B = 20, 2
    m, _ = cr.cond_model(T, B)
    shape = (B, 8, 8, 8, 4)
    x0 = torch.rand(shape, generator=torch.Generator().manual_seed(6)) * 2 - 1
    mask = cr.half_mask(B, 16, slab=True)
    runs = [dict(sampler="ddpm", mask=mask, strength=0.6), dict(sampler="ddpm", mask=mask[:1].flip(2)),
            dict(sampler="ddim", num_steps=5, eta=0.5, mask=mask, strength=0.7), dict(sampler="ddim", num_steps=10, clip_x0=False)]
    results = []
    for kw in runs:
        a = m.edit(x0, 0, seed=5, use_graph=True, **kw)
        b = m.edit(x0, 0, seed=5, use_graph=False, **kw)
        torch.cuda.synchronize()
        assert torch.equal(a, b) and torch.isfinite(a).all(), kw
        results.append(a)
    gen = {k: m.generate(shape, context_value=0, seed=5, **kw) for k, kw in (("ddpm", {}), ("ddim", dict(sampler="ddim", num_steps=5)))}
    # interleaved on the same plan, against fresh models
    again = [m.edit(x0, 0, seed=5, **kw) for kw in runs]
    fresh, _ = cr.cond_model(T, B)
    for kw, r, a in zip(runs, results, again):
        f = fresh.edit(x0, 0, seed=5, **kw)
        torch.cuda.synchronize()
        assert torch.equal(r, a) and torch.equal(r, f), kw
    fresh2, _ = cr.cond_model(T, B)
    assert torch.equal(gen["ddpm"], fresh2.generate(shape, context_value=0, seed=5))
    assert torch.equal(gen["ddim"], fresh2.generate(shape, context_value=0, seed=5, sampler="ddim", num_steps=5))
    assert torch.equal(m.generate(shape, context_value=0, seed=5), gen["ddpm"])


def test_unconditional_edit(dev):
    """The unconditional model edits without a context: kept voxels are x0, and mask=None at strength 1 is generate()."""
    T = 10
    m, _ = cr.uncond_model(T)
    x0 = torch.rand((1, 8, 8, 8, 4), generator=torch.Generator().manual_seed(7)) * 2 - 1
    assert torch.equal(m.edit(x0, seed=3), m.generate((1, 8, 8, 8, 4), seed=3))
    got = m.edit(x0, mask=cr.half_mask(1, 16, slab=True), strength=0.5, seed=3, sampler="ddim", num_steps=4).cpu()
    assert torch.equal(got[:, 5:], x0[:, 5:]) and not torch.equal(got[:, :4], x0[:, :4])


def test_full_size_ddim_edit_chain(dev):
    """32^3 x 8ch (h3), B = 32: a whole S = 50 DDIM edit chain through the graph with a mask given at 128^3: finite, the range guard
    quiet, kept voxels x0.  The output conv is scaled by 0.1 (untrained weights amplify eps along a DDIM chain)."""
    from dm3d_amd.diffusion import latent_mask
    T, S, B, C = 1000, 50, 32, 8
    m, _ = cr.cond_model(T, B, size=32, C=C, W=cr.weights(32, C, scale=0.1), precision="h3")
    shape = (B, 32, 32, 32, C)
    g = torch.Generator().manual_seed(12)
    x0 = (torch.rand(shape, generator=g) * 2 - 1).to(dev)
    mask = torch.zeros((1, 128, 128, 128, 1))
    mask[0, 30:90, 40:100, 20:80] = 1.0                                    # a box, not aligned to the 4^3 blocks
    ids = torch.randint(0, 2, (B,), generator=g)
    out = m.edit(x0, ids, mask=mask, sampler="ddim", num_steps=S, seed=7)   # check_range raises if flagged
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and float(out.abs().max()) <= 1.0 + 1e-6
    keep = (1 - latent_mask(mask, shape)).to(dev)
    kept = (keep == 1).unsqueeze(-1).expand(shape)
    assert torch.equal(out[kept], x0[kept]) and not torch.equal(out[~kept], x0[~kept])
