"""tests/chain_reference.py against itself, on the CPU: identities that follow from the formulas, each to 1e-12 relative (float64
expressions of O(1) values over a few steps move by units of 2e-16 when re-associated).  The network is a stand-in, an elementwise
function of (x, t) on a (2, 4, 4, 4, 4) tensor; the oracle U-Net is not needed."""
import math

import numpy as np
import pytest
import torch

import chain_reference as cr

TOL = 1e-12
SHAPE = (2, 4, 4, 4, 4)
SCHEDULES = [(20, 5), (1000, 10)]
CASES = [(400, 380, 420), (300, 150, 999), (200, 100, 300), (50, 49, 51), (5, 0, 900), (20, -1, 25)]     # (s, t, p)


def _net(x, t):
    return torch.tanh(0.7 * x) + 0.01 * t


def _rel(a, b):
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-300))


def _inputs(seed, n):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(SHAPE, generator=g, dtype=torch.float64) for _ in range(n)]


def _ode_row(ab, s, t, p):
    """The ODE row of Lu et al. 2022 as the paper spells it, with r = (lambda_s - lambda_p) / h."""
    if t < 0:
        return 0.0, 1.0, 0.0, 0.0
    al, sg = (lambda i: math.sqrt(ab[i])), (lambda i: math.sqrt(1 - ab[i]))
    lam = lambda i: math.log(al(i) / sg(i))
    h = lam(t) - lam(s)
    A = al(t) * (1 - math.exp(-h))
    if p < 0:
        return sg(t) / sg(s), A, 0.0, 0.0
    r = (lam(s) - lam(p)) / h
    return sg(t) / sg(s), A * (1 + 1 / (2 * r)), -A / (2 * r), 0.0


def test_dpm_row_at_eta_zero_is_the_ode_row():
    ab = cr.alpha_bar64(1000)
    for s, t, p in CASES:
        for q in (p, -1):
            assert cr.dpm_row64(ab, s, t, q) == cr.dpm_row64(ab, s, t, q, 0.0)
            assert _rel(cr.dpm_row64(ab, s, t, q, 0.0), _ode_row(ab, s, t, q)) < TOL, (s, t, q)


def test_first_order_row_without_clip_is_the_ddim_step():
    ab = cr.alpha_bar64(1000)
    x, e = _inputs(1, 2)
    for s, t, _ in CASES:
        out, x0 = cr.dpm64(x, e, ab, s, t, clip=False)
        assert _rel(out, cr.ddim64(x, e, ab[s], ab[t] if t >= 0 else 1.0, clip=False)) < TOL, (s, t)
        assert _rel(x0, cr.x0_64("eps", x, e, ab[s])) == 0.0


@pytest.mark.parametrize("T,S", SCHEDULES)
def test_order_one_chain_without_clip_is_the_ddim_chain(T, S):
    ab, sched, (x_T,) = cr.alpha_bar64(T), cr.schedule(T, S), _inputs(2, 1)
    dpm = cr.chain64(_net, ab, sched, x_T, order=1, clip=False)
    assert _rel(dpm, cr.chain64(_net, ab, sched, x_T, "ddim", clip=False)) < TOL
    assert _rel(dpm, cr.chain64(_net, ab, sched, x_T, order=2, clip=False)) > 1e-6        # the second-order rows do something


def test_guidance_at_w_one_is_the_positive_branch():
    pos, neg = _inputs(3, 2)
    assert _rel(cr.guide64(pos, neg, 1.0), pos) < TOL
    assert _rel(cr.guide64(pos, neg, [1.0, 1.0], [0.0, 0.0]), pos) < TOL
    factors = []
    mixed = cr.guide64(pos, neg, [1.0, 3.0], [0.0, 0.7], factors)                        # one value per volume
    assert _rel(mixed[0], pos[0]) < TOL and _rel(mixed[1], cr.guide64(pos[1:], neg[1:], 3.0, 0.7)[0]) == 0.0 and len(factors) == 1


@pytest.mark.parametrize("T,S", SCHEDULES)
def test_sde_chain_at_eta_zero_is_the_ode_chain(T, S):
    ab, sched, (x_T,) = cr.alpha_bar64(T), cr.schedule(T, S), _inputs(4, 1)
    noise = torch.randn((S,) + SHAPE, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    for kw in (dict(), dict(order=1, clip=False), dict(lower_order_final=False), dict(thr=(0.9, 4.0, []))):
        ode = cr.chain64(_net, ab, sched, x_T, **kw)
        assert _rel(cr.chain64(_net, ab, sched, x_T, eta=0.0, noise=noise, **kw), ode) < TOL, kw
        assert _rel(cr.chain64(_net, ab, sched, x_T, eta=1.0, noise=noise, **kw), ode) > 1e-3, kw      # ... and eta is read


@pytest.mark.parametrize("solver", ["ddim", "dpmpp"])
@pytest.mark.parametrize("T,S", SCHEDULES)
def test_steps_is_a_prefix_of_states(T, S, solver):
    ab, sched, (x_T,) = cr.alpha_bar64(T), cr.schedule(T, S), _inputs(6, 1)
    noise = torch.randn((S,) + SHAPE, generator=torch.Generator().manual_seed(7), dtype=torch.float64)
    states = []
    last = cr.chain64(_net, ab, sched, x_T, solver, eta=0.5, noise=noise, states=states)
    assert len(states) == S and _rel(last, states[-1]) == 0.0
    assert _rel(cr.chain64(_net, ab, sched, x_T, solver, eta=0.5, noise=noise, steps=0), x_T) == 0.0
    for k in range(1, S + 1):
        assert _rel(cr.chain64(_net, ab, sched, x_T, solver, eta=0.5, noise=noise, steps=k), states[k - 1]) < TOL, k


@pytest.mark.parametrize("eta,tiny", [(0.0, 1e-12), (1.0, 1e-12), (0.5, 1e-24)])
def test_start_row_at_alpha_bar_zero_is_the_limit_of_the_general_row(eta, tiny):
    """At eta = 0 and eta = 1 the row is smooth in alpha_s = sqrt(alpha_bar): at alpha_bar = 1e-12 the general row lies within ~1e-6
    relative of the limit written out, and is held to 1e-5.  At a fractional eta c_x = (sigma_t / sigma_s) exp(-eta h) falls as
    alpha_s^eta only, so eta = 0.5 is evaluated where that is 1e-6 as well: alpha_bar = 1e-24."""
    ab = cr.alpha_bar64(20, ztsnr=True)
    assert ab[-1] == 0.0
    near = ab.copy()
    near[-1] = tiny
    for t in (14, 3):
        limit, general = cr.dpm_row64(ab, 19, t, -1, eta), cr.dpm_row64(near, 19, t, -1, eta)
        assert limit[2] == 0.0 and general[2] == 0.0
        assert np.abs(np.array(limit) - np.array(general)).max() / np.abs(np.array(limit)).max() < 1e-5, (t, limit, general)
    # a history level at alpha_bar = 0 leaves the step after it first order
    assert cr.dpm_row64(ab, 14, 9, 19, eta) == cr.dpm_row64(ab, 14, 9, -1, eta)
