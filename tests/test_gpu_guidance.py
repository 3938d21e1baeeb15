"""GPU tier of classifier-free guidance (dm3d_guide_update, guide_eps, generate / edit / sampler with guidance_scale=).

The float64 reference is tests/chain_reference.py's restatement: eps_pos and eps_neg from the CPU oracle (oracle.ref_torch.unet_forward)
under the wanted and the negative context, eps_g = eps_neg + w (eps_pos - eps_neg), the guidance rescale of Lin et al. 2023 (section 3.4)
from population standard deviations per volume, then the DDPM posterior step (the oracle's) or the DDIM update (restated there), with
alpha_bar from the oracle's float32 Betas table, the table the kernels read.  w and phi enter as the float32 the kernel's tables hold.

Measured on an MI355X (profiles/guidance_gpu_run.log), maximum absolute difference to the float64 chain at 8^3 x 4ch, T = 20, B = 2,
w = 3 (bar 1e-2):
    DDPM            phi = 0: 1.50e-05   phi = 0.7: 1.21e-05
    DDIM eta = 0    phi = 0: 2.34e-05   phi = 0.7: 2.59e-05
    DDIM eta = 0.5  phi = 0: 2.84e-05   phi = 0.7: 2.51e-05
three full-size guided DDIM steps (32^3 x 8ch, h3): 6.60e-03 at max |ref| 202.5 = 3.3e-05 relative (bar 5e-3); guide_eps against
float64: 3.5e-06 (bar 8.9e-06) without and 1.7e-06 (bar 2.3e-05) with the rescale, 7.6e-06 (3.3e-05) and 1.3e-05 (8.5e-05) in the
|mean| / std = 100 case.
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


def _per_volume(v, B):
    return [float(np.float32(u)) for u in np.broadcast_to(np.asarray(v, dtype=np.float64).reshape(-1), (B,))]    # the tables are float32


def _guide_as_tables(ep, en, w, phi=0.0):
    """cr.guide64 on w and phi as the tables hold them; also returns max(f, 1) over the volumes."""
    B, factors = ep.shape[0], []
    return cr.guide64(ep, en, _per_volume(w, B), _per_volume(phi, B), factors), max([1.0] + factors)


W3, PHI3 = (7.5, -1.0, 0.3), (0.7, 0.0, 1.0)


@pytest.mark.parametrize("offset", [0.0, 100.0])
def test_kernel_matches_float64_restatement(dev, offset):
    """guide_eps on random predictions with per-volume w, without and with a per-volume rescale; offset 100: |mean| / std = 100, the
    cancellation case of the standard deviations.  The bars are derived (three float32 roundings in the combine, two more with the
    rescale), absolute in M = max(|eps_neg| + |w| |eps_pos - eps_neg|)."""
    m, _ = cr.cond_model(20, 3)
    g = torch.Generator().manual_seed(41)
    shape = (3, 8, 8, 8, 4)
    ep, en = torch.randn(shape, generator=g) + offset, torch.randn(shape, generator=g) + offset
    wv = torch.tensor(_per_volume(W3, 3), dtype=torch.float64).reshape(3, 1, 1, 1, 1)
    M = float((en.double().abs() + wv.abs() * (ep.double() - en.double()).abs()).max())
    ref, _ = _guide_as_tables(ep, en, W3)
    got = m.guide_eps(ep, en, W3).cpu()
    err = float((got.double() - ref).abs().max())
    print(f"guide_eps offset={offset}: phi=0 err {err:.3e} (bar {2.0 ** -22 * M:.3e})")
    assert err <= 2.0 ** -22 * M
    ref, fmax = _guide_as_tables(ep, en, W3, PHI3)
    got = m.guide_eps(ep, en, W3, PHI3).cpu()
    err = float((got.double() - ref).abs().max())
    print(f"guide_eps offset={offset}: per-volume phi err {err:.3e} (bar {2.0 ** -21 * M * fmax:.3e}, max f {fmax:.4f})")
    assert err <= 2.0 ** -21 * M * fmax
    # one scalar for every volume, too
    ref, fmax = _guide_as_tables(ep, en, 3.0, 0.7)
    assert float((m.guide_eps(ep, en, 3.0, 0.7).cpu().double() - ref).abs().max()) <= 2.0 ** -21 * fmax * float(
        (en.double().abs() + 3.0 * (ep.double() - en.double()).abs()).max())


def test_constant_volume_and_nan(dev):
    m, _ = cr.cond_model(20, 3)
    g = torch.Generator().manual_seed(42)
    shape = (3, 8, 8, 8, 4)
    ep, en = torch.randn(shape, generator=g), torch.randn(shape, generator=g)
    # std(eps_g) == 0: f = 1 (w = 0 hands on a constant eps_neg)
    flat = en.clone()
    flat[1] = 0.25
    got = m.guide_eps(ep, flat, (3.0, 0.0, 3.0), 0.5).cpu()
    assert torch.equal(got[1], flat[1]) and torch.isfinite(got).all()
    # a NaN in one element of eps_pos: that element at phi = 0, that whole volume and no other at phi != 0
    bad = ep.clone()
    bad[0, 1, 2, 3, 1] = float("nan")
    got = m.guide_eps(bad, en, W3).cpu()
    assert torch.isnan(got[0, 1, 2, 3, 1]) and int(torch.isnan(got).sum()) == 1
    got = m.guide_eps(bad, en, W3, PHI3).cpu()
    assert torch.isnan(got[0]).all() and not torch.isnan(got[1:]).any()
    bad = ep.clone()
    bad[1, 0, 0, 0, 0] = float("nan")                                       # volume 1 has phi = 0
    got = m.guide_eps(bad, en, W3, PHI3).cpu()
    assert torch.isnan(got[1, 0, 0, 0, 0]) and int(torch.isnan(got).sum()) == 1


def test_bitwise_identities_of_the_combine(dev):
    m, _ = cr.cond_model(20, 3)
    g = torch.Generator().manual_seed(43)
    shape = (3, 8, 8, 8, 4)
    ep, en = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    ep0, en0 = ep.clone(), en.clone()
    assert torch.equal(m.guide_eps(ep, en, 1.0), ep)                        # w = 1, phi = 0
    assert torch.equal(m.guide_eps(ep, en, 1.0, 0.0), ep)
    assert torch.equal(m.guide_eps(ep, en, 0.0), en)                        # w = 0
    nan = torch.full_like(ep, float("nan"))
    assert torch.equal(m.guide_eps(nan, en, 0.0), en)                       # ... and eps_pos is not read
    assert torch.equal(m.guide_eps(ep, nan, 1.0), ep)                       # nor eps_neg at w = 1
    mixed = m.guide_eps(ep, en, (1.0, 0.0, 2.5))
    assert torch.equal(mixed[0], ep[0]) and torch.equal(mixed[1], en[1]) and not torch.equal(mixed[2], ep[2])
    assert torch.equal(m.guide_eps(ep, en, W3, 0.0), m.guide_eps(ep, en, W3))            # phi = 0 is the phi-less call
    assert torch.equal(m.guide_eps(ep, en, W3, (0.0, 0.0, 0.0)), m.guide_eps(ep, en, W3))
    both = m.guide_eps(ep, en, W3, PHI3)
    assert torch.equal(both[1], m.guide_eps(ep, en, W3)[1])                 # a row with phi = 0 among rescaled rows
    assert torch.equal(both, m.guide_eps(ep, en, W3, PHI3))                 # the reduction order is fixed: runs repeat bitwise
    torch.cuda.synchronize()
    assert torch.equal(ep, ep0) and torch.equal(en, en0)                    # the inputs are left untouched


def test_guided_chain_is_the_plain_2b_chain_at_w_one(dev):
    """8^3 x 4ch, T = 20, B = 2, c = (1, 0), n = (0, 1): the guided chain drives the plan of the plain 4-row chain with contexts
    (1, 0, 0, 1), the same U-Net launches, update kernel and Philox counters for rows 0-1."""
    T, B = 20, 2
    m, _ = cr.cond_model(T, 2 * B)
    shape, shape2 = (B, 8, 8, 8, 4), (2 * B, 8, 8, 8, 4)
    c, n = [1, 0], [0, 1]
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(5))
    x_T2 = torch.cat([x_T, x_T])
    for kw in (dict(), dict(sampler="ddim", num_steps=5, eta=0.5)):
        got = m.generate(shape, context_value=c, x_T=x_T, seed=5, guidance_scale=1.0, negative_context=n, **kw)
        plain = m.generate(shape2, context_value=c + n, x_T=x_T2, seed=5, **kw)
        torch.cuda.synchronize()
        assert got.shape == shape and torch.isfinite(got).all()
        assert torch.equal(got, plain[:B]), kw
        assert not torch.equal(plain[:B], plain[B:])                        # the two contexts do differ
    # w = 0 follows the negative branch: without draws (DDIM, eta = 0) that is rows 2: of the plain chain
    kw = dict(sampler="ddim", num_steps=5)
    got = m.generate(shape, context_value=c, x_T=x_T, seed=5, guidance_scale=0.0, negative_context=n, **kw)
    plain = m.generate(shape2, context_value=c + n, x_T=x_T2, seed=5, **kw)
    assert torch.equal(got, plain[B:])
    # the x_T a guided chain draws is the one the unguided chain of the same B volumes draws under the same seed, in both halves
    gs = m.sampler(shape, c, seed=9, guidance_scale=2.0, negative_context=n)
    gs.reset()
    drawn = gs.plan.x.clone()
    ps = m.sampler(shape, c, seed=9)
    ps.reset()
    torch.cuda.synchronize()
    assert torch.equal(drawn[:B], ps.plan.x) and torch.equal(drawn[B:], ps.plan.x) and gs.plan.B == 2 * B and ps.plan.B == B


@pytest.mark.parametrize("phi", [0.0, 0.7])
@pytest.mark.parametrize("kind,eta", [("ddpm", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_guided_chain_matches_float64(dev, kind, eta, phi):
    """8^3 x 4ch, T = 20, B = 2, per-volume contexts, w = 3: DDPM with injected noise; DDIM S = 5 at eta = 0 and at eta = 0.5 with
    injected noise.  Bar: the chain bar times |w| + |1 - w| = 5, the absolute coefficient sum of the two branch predictions."""
    T, S, B, w = 20, 5, 2, 3.0
    m, W = cr.cond_model(T, B)
    g = torch.Generator().manual_seed(23)
    shape = (B, 8, 8, 8, 4)
    x_T = torch.randn(shape, generator=g)
    c, n = torch.tensor([[[1]], [[0]]]), torch.tensor([[[0]], [[1]]])
    f, b = cr.oracle(W), cr.oracle_betas(T)
    ab = b.alpha_bar.double()
    net = lambda x, t: _guide_as_tables(f(x, t, c), f(x, t, n), w, phi)[0]
    if kind == "ddpm":
        noise = torch.randn((T,) + shape, generator=g)
        got = m.generate(shape, context_value=c, x_T=x_T, noise=noise, guidance_scale=w, negative_context=n, guidance_rescale=phi)
        ref = cr.chain64(net, ab, list(range(T)), x_T, "ddpm", noise=noise, betas=b)
    else:
        noise = torch.randn((S,) + shape, generator=g) if eta else None
        got = m.generate(shape, context_value=c, x_T=x_T, noise=noise, sampler="ddim", num_steps=S, eta=eta, guidance_scale=w,
                         negative_context=n, guidance_rescale=phi)
        ref = cr.chain64(net, ab, cr.schedule(T, S), x_T, "ddim", eta=eta, noise=noise)
    err = float((got.cpu().double() - ref).abs().max())
    print(f"guided {kind} eta={eta} phi={phi} chain: max abs difference {err:.2e}")
    assert err < CHAIN_BAR * (abs(w) + abs(1 - w))
    # guidance does something: the chain differs from the unguided one
    plain = m.generate(shape, context_value=c, x_T=x_T, noise=noise, **(dict(sampler="ddim", num_steps=S, eta=eta) if kind == "ddim" else {}))
    assert not torch.equal(plain, got)


def test_graph_equals_eager_and_kinds_do_not_leak(dev):
    """Seeded guided chains of the four kinds are bitwise equal through the graph and eagerly; two scales and a phi = 0 / phi != 0 pair
    go through the one cached graph of their kind; the plain chain of the same 2 B-row plan is untouched by it, and the reverse."""
    T, B = 20, 2
    m, _ = cr.cond_model(T, 2 * B)
    shape, shape2 = (B, 8, 8, 8, 4), (2 * B, 8, 8, 8, 4)
    x0 = torch.rand(shape, generator=torch.Generator().manual_seed(6)) * 2 - 1
    mask = cr.half_mask(B)
    gkw = dict(guidance_scale=3.0, negative_context=[0, 1])
    ddim = dict(sampler="ddim", num_steps=5, eta=0.5)
    calls = {
        "ddpm-cfg": lambda **kw: m.generate(shape, context_value=[1, 0], seed=5, **kw),
        "ddim-cfg": lambda **kw: m.generate(shape, context_value=[1, 0], seed=5, **ddim, **kw),
        "ddpm-edit-cfg": lambda **kw: m.edit(x0, [1, 0], mask=mask, seed=5, **kw),
        "ddim-edit-cfg": lambda **kw: m.edit(x0, [1, 0], mask=mask, strength=0.6, seed=5, **ddim, **kw),
    }
    for kind, call in calls.items():
        outs = []
        for over in (dict(), dict(guidance_scale=[1.5, -0.5]), dict(guidance_rescale=0.7), dict(guidance_rescale=[0.0, 1.0])):
            kw = dict(gkw, **over)
            a = call(use_graph=True, **kw)
            e = call(use_graph=False, **kw)
            a2 = call(use_graph=True, **kw)
            torch.cuda.synchronize()
            assert torch.equal(a, e) and torch.equal(a, a2) and torch.isfinite(a).all(), (kind, over)
            outs.append(a)
        assert not torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2]) and not torch.equal(outs[2], outs[3]), kind
        assert torch.equal(outs[0][0], outs[3][0])                           # volume 0 of the last call has phi = 0
        assert sum(1 for k in m._graphs if k[1] == kind) == 1, kind            # one graph served them all
    assert {k[1] for k in m._graphs} == set(calls)
    # the plain chains of the 2 B-row plan the guided chains drove: as on a fresh model
    fresh, _ = cr.cond_model(T, 2 * B)
    for kw in (dict(), ddim):
        plain = m.generate(shape2, context_value=[1, 0, 0, 1], seed=5, **kw)
        torch.cuda.synchronize()
        assert torch.equal(plain, fresh.generate(shape2, context_value=[1, 0, 0, 1], seed=5, **kw))
    assert {"ddpm", "ddim"} <= {k[1] for k in m._graphs}
    # and the guided chains after that still replay their own graphs
    for kind, call in calls.items():
        assert torch.equal(call(use_graph=True, **gkw), call(use_graph=False, **gkw)), kind
    # the public Sampler: S steps, then step() raises until reset(); an older sampler of the plan is retired
    smp = m.sampler(shape, [1, 0], seed=5, kind="ddim", num_steps=5, eta=0.5, **gkw).prepare()
    smp.reset()
    for _ in range(5):
        smp.step()
    assert torch.equal(smp.x, calls["ddim-cfg"](**gkw)) and torch.equal(smp.plan.x[:B], smp.plan.x[B:])
    with pytest.raises(RuntimeError):
        smp.step()


def test_guided_edit(dev):
    """A half-volume mask keeps x0 bitwise under guidance; at w = 1 the guided edit is the first half of the plain 2 B edit with x0,
    mask and known_noise duplicated."""
    T, B = 20, 2
    m, _ = cr.cond_model(T, 2 * B)
    g = torch.Generator().manual_seed(7)
    shape = (B, 8, 8, 8, 4)
    x0 = torch.rand(shape, generator=g) * 2 - 1
    mask = cr.half_mask(B)
    c, n = [1, 0], [0, 1]
    ddim = dict(sampler="ddim", num_steps=5, eta=0.5)
    for kw in (dict(), dict(strength=0.5), ddim, dict(ddim, strength=0.6)):
        for phi in (0.0, 0.7):
            out = m.edit(x0, c, mask=mask, seed=3, guidance_scale=3.0, negative_context=n, guidance_rescale=phi, **kw).cpu()
            assert torch.equal(out[:, 4:], x0[:, 4:]) and not torch.equal(out[:, :4], x0[:, :4]), (kw, phi)
            assert torch.isfinite(out).all()
        got = m.edit(x0, c, mask=mask, seed=3, guidance_scale=1.0, negative_context=n, **kw)
        plain = m.edit(torch.cat([x0, x0]), c + n, mask=torch.cat([mask, mask]), seed=3, **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, plain[:B]), kw
    # injected known-latent noise (the eager path), duplicated for the plain chain
    for kw, rows in ((dict(strength=0.5), 11), (dict(ddim, strength=0.6), 4)):
        kn = torch.randn((rows,) + shape, generator=g)
        got = m.edit(x0, c, mask=mask, seed=3, known_noise=kn, guidance_scale=1.0, negative_context=n, **kw)
        plain = m.edit(torch.cat([x0, x0]), c + n, mask=torch.cat([mask, mask]), seed=3, known_noise=torch.cat([kn, kn], 1), **kw)
        torch.cuda.synchronize()
        assert torch.equal(got, plain[:B]), kw


def test_per_volume_scales(dev):
    """B = 3 with w = (1, 3, 0) in one call equals, volume by volume, the three calls with one scalar each (the same plan)."""
    T, B = 20, 3
    m, _ = cr.cond_model(T, 2 * B)
    shape = (B, 8, 8, 8, 4)
    c, n, ws = [1, 0, 1], [0, 1, 0], (1.0, 3.0, 0.0)
    for kw in (dict(), dict(sampler="ddim", num_steps=5, eta=0.5), dict(guidance_rescale=0.5),
               dict(sampler="ddim", num_steps=5, guidance_rescale=[0.3, 0.6, 0.9])):
        one = m.generate(shape, context_value=c, seed=11, guidance_scale=ws, negative_context=n, **kw)
        for b, w in enumerate(ws):
            each = m.generate(shape, context_value=c, seed=11, guidance_scale=w, negative_context=n, **kw)
            assert torch.equal(one[b], each[b]), (kw, b)
        assert not torch.equal(one[0], one[2])


def test_full_size_steps_match_oracle_and_b32_chain(dev):
    """32^3 x 8ch (h3), T = 1000: three guided DDIM steps of the S = 50 schedule at B = 2, w = 3, against the oracle under the eps
    contract (1e-3 of max |ref|) times |w| + |1 - w| = 5; one whole guided S = 50 chain of B = 32, a 64-row plan, through the graph
    (output conv scaled by 0.1, as the unguided full-size chain test) is finite, within [-1, 1], and leaves the range guard quiet."""
    T, S, B, C, w = 1000, 50, 2, 8, 3.0
    m, W = cr.cond_model(T, B, size=32, C=C, precision="h3")
    shape = (B, 32, 32, 32, C)
    x_T = torch.randn(shape, generator=torch.Generator().manual_seed(12))
    c, n = torch.tensor([[[1]], [[0]]]), torch.tensor([[[0]], [[1]]])
    got = m.generate(shape, context_value=c, x_T=x_T, sampler="ddim", num_steps=S, steps=3, guidance_scale=w, negative_context=n).cpu()
    f = cr.oracle(W, 32, C)
    ref = cr.chain64(lambda x, t: _guide_as_tables(f(x, t, c), f(x, t, n), w)[0], cr.oracle_alpha_bar(T).double(), cr.schedule(T, S), x_T,
                     "ddim", steps=3)
    err = float((got.double() - ref).abs().max())
    print(f"3 full-size guided DDIM steps: max abs difference {err:.2e}, max |x| {float(ref.abs().max()):.3f}")
    assert err / float(ref.abs().max()) < 1e-3 * (abs(w) + abs(1 - w))
    big, _ = cr.cond_model(T, 32, size=32, C=C, W=cr.weights(32, C, scale=0.1), precision="h3")
    out = big.generate((32, 32, 32, 32, C), context_value=1, seed=7, sampler="ddim", num_steps=S, guidance_scale=w, negative_context=0,
                       guidance_rescale=0.7)                                # check_range raises if flagged
    torch.cuda.synchronize()
    assert out.shape == (32, 32, 32, 32, C) and torch.isfinite(out).all() and float(out.abs().max()) <= 1.0 + 1e-6
