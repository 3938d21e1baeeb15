"""CPU tier of the exact-sum cases (tests/h3_exact_cases.py): every case x pattern meets the exactness budget and the lossless-split
assertions; the host model of the h3 contraction equals the float64 reference bit for bit under five random summation orders (and is
inside the stated bar for both-lo and the prologue forms); dropping ONE al.bh or ah.bl piece — any tap, any 8-channel slot — moves at
least one output by a whole quantum, so the exact patterns catch it; the same drop on the dense Gaussian operands of
tests/test_gpu_infer_kernels.py mostly stays under that suite's 2e-5 bar (figures in the last test but one), which is the gap the exact
patterns close."""
import numpy as np
import pytest

import h3_exact_cases as hx
import test_gpu_infer_kernels as tk

ORDERS = 5


def _cases():
    out = [(n, hx.exact_form(tk.CONV_BY_NAME[n])) for n in hx.EXACT_CONV]
    out += [(n + " (H2 in)", hx.exact_form(tk.CONV_BY_NAME[n], x_h2=True)) for n in hx.H2_IN_TOO]
    return out


def _perm(seed):
    g = np.random.default_rng(seed)
    return lambda n: g.permutation(n)


@pytest.mark.parametrize("name,s", _cases(), ids=[n for n, _ in _cases()])
def test_budget_and_lossless_splits(name, s):
    for pattern in hx.PATTERNS:
        for rot in hx.ROTATIONS:
            h = hx.conv_host(s, pattern, rot)
            q, ratio = hx.budget(s, h, pattern)
            if pattern in hx.EXACT:
                assert ratio < hx.BUDGET
                ref = hx.conv_finish(h, h["res"])
                assert np.array_equal(ref.astype(np.float32).astype(np.float64), ref), "the reference itself is no float32"
                assert np.array_equal(ref / q, np.rint(ref / q)), "the reference is off the quantum grid"
    cin, taps = s["c1"] + s["c2"], (64 if s["tr"] else s["ks"] ** 3)
    if s["cout"] % 64 == 0:
        assert (hx.live_mask(taps, cin, 64, 16).sum(1) == 1).all(), "every (tap, ci) is live in exactly one channel of a column tile"
    assert hx.live_mask(taps, cin, s["cout"], 21).any(1).all()


@pytest.mark.parametrize("name", hx.INEXACT_CONV)
def test_inexact_forms_have_room_for_their_step(name):
    s = tk.CONV_BY_NAME[name]
    assert hx.is_inexact(s)
    for pattern in ("act-lo", "wgt-lo"):
        h = hx.conv_host(s, pattern, 1)
        hx.budget(s, h, pattern)
        assert max(float(np.abs(v).max()) for v in (h["bias"], h["vec"], h["res"])) <= 0.5


HOST_DIRECT = ("v3 td4 nct4 full 16B", "v3 td4 partial 6x5x7 cout40", "v3 dual input 16+12", "tap k3 s2 5x6x8", "tap k4 s2 6x8x4", "parity upsample 4^3")
HOST_WINO = ("wino Cin32", "wino Cin48 B2")


@pytest.mark.parametrize("name", HOST_DIRECT)
def test_host_model_equals_float64_in_any_order(name):
    s = hx.exact_form(tk.CONV_BY_NAME[name], B=1)
    for pattern in hx.PATTERNS:
        h = hx.conv_host(s, pattern, 21)
        ref = hx.conv_only64(s, h)
        if pattern == "hi":                                   # (the im2col of the model against the reference's own geometry, in float64)
            A, W = hx.im2col(s, hx.conv_x(h)).astype(np.float64), h["kernel"].reshape(-1, s["cout"]).astype(np.float64)
            assert np.array_equal((A @ W).reshape(ref.shape), ref)
        for o in range(ORDERS if pattern != "hi" else 2):
            got = hx.direct_contract(s, h, _perm(o)).astype(np.float64)
            if pattern in hx.EXACT:
                assert np.array_equal(got, ref), f"{name} / {pattern}, order {o}"
            else:
                assert (np.abs(got - ref) <= hx.BOTH_LO_TOL * h["abs"]).all(), f"{name} / {pattern}, order {o}"
                assert not np.array_equal(got, ref)


@pytest.mark.parametrize("name", HOST_WINO)
def test_wino_model_equals_float64_in_any_order(name):
    s = hx.exact_form(tk.CONV_BY_NAME[name], B=1)
    for pattern in hx.PATTERNS:
        h = hx.conv_host(s, pattern, 16)
        ref = hx.conv_only64(s, h)
        for o, fold in ((0, True), (1, False), (2, True), (3, True), (4, True)):
            got = hx.wino_contract(hx.conv_x(h), h["kernel"], h["w_exp"], _perm(o), fold=fold).astype(np.float64)
            if pattern in hx.EXACT:
                assert np.array_equal(got, ref), f"{name} / {pattern}, order {o}"
            else:
                assert (np.abs(got - ref) <= hx.BOTH_LO_TOL * h["abs"]).all(), f"{name} / {pattern}, order {o}"


def test_prologue_form_inside_its_bar_on_the_model():
    """The model with the prologue evaluated in float32 (the kernel's arithmetic) against the float64 prologue: inside ELEM_TOL sum|a||b|."""
    s = dict(tk.CONV_BY_NAME["v3 td4 nct4 full 16B"], B=1)
    for pattern in ("act-lo", "wgt-lo"):
        h = hx.conv_host(s, pattern, 1)
        x = hx.conv_x(h)
        z = x * h["pro"][0] + h["pro"][1]
        a32 = (z / (np.float32(1) + np.exp(-z))).astype(np.float32)
        h32 = dict(h, x1=a32, x2=None)
        plain = hx.exact_form(s)
        got = hx.direct_contract(plain, h32, _perm(0)).astype(np.float64)
        ref = hx.conv_only64(plain, dict(h, x1=hx._acts64(h, x), x2=None))
        assert (np.abs(got - ref) <= hx.conv_bar(s, h, pattern)).all()


def _caught(got, ref, q):
    return float(np.abs(got.astype(np.float64) - ref).max()) >= q


@pytest.mark.parametrize("term", hx.TERMS)
def test_drop_one_piece_is_caught_direct(term):
    s = hx.exact_form(tk.CONV_BY_NAME["v3 td4 nct4 full 16B"], B=1, dims=(4, 4, 4))
    pattern = "act-lo" if term == "al_bh" else "wgt-lo"
    h = hx.conv_host(s, pattern, 1)
    q, _ = hx.budget(s, h, pattern)
    ref = hx.conv_only64(s, h)
    assert np.array_equal(hx.direct_contract(s, h).astype(np.float64), ref)
    for tap in range(27):
        for slot in range(s["c1"] // 8):
            assert _caught(hx.direct_contract(s, h, drop=(term, tap, slot)), ref, q), f"dropping {term} at tap {tap}, slot {slot} goes unseen"
    other = "wgt-lo" if term == "al_bh" else "act-lo"          # the mirror pattern holds no such piece: nothing to lose there
    ho = hx.conv_host(s, other, 1)
    assert np.array_equal(hx.direct_contract(s, ho, drop=(term, 13, 0)).astype(np.float64), hx.conv_only64(s, ho))


@pytest.mark.parametrize("term", hx.TERMS)
def test_drop_one_piece_is_caught_wino(term):
    s = hx.exact_form(tk.CONV_BY_NAME["wino Cin32"], dims=(4, 4, 4))
    pattern = "act-lo" if term == "al_bh" else "wgt-lo"
    h = hx.conv_host(s, pattern, 16)
    q, _ = hx.budget(s, h, pattern)
    ref = hx.conv_only64(s, h)
    for tap in range(9):
        for slot in range(s["c1"] // 8):
            got = hx.wino_contract(hx.conv_x(h), h["kernel"], h["w_exp"], drop=(term, tap, slot, (tap + slot) % 4))
            assert _caught(got, ref, q), f"dropping {term} at (dz, dy) = {divmod(tap, 3)}, slot {slot} goes unseen"


@pytest.mark.parametrize("name", ["wino Cin32", "v3 td4 nct4 full 16B"])
def test_the_same_drop_passes_the_gaussian_bar(name):
    """What this file closes: on the dense Gaussian operands of the parity suite a lost piece hides under LAYER_TOL = 2e-5, measured as
    test_conv3d measures it (max|err| over max|stored reference|).  Most drops do, not all: a piece lost for one (tap, input channel) has a
    median of 5e-6 .. 1e-5 and a
    worst of 1.6e-5 .. 3.0e-5 over the 54 sampled; a whole 8-channel slot of a tap has a median of 1.5-1.7e-5, a worst of 2.5-3.9e-5, and
    71-96 % of the 108 (tap, slot) choices per term and case are under the bar.  (An estimate of 2e-6 / 6e-6 of max|ref| holds for a typical
    output; the bar takes the maximum over 32768 outputs, four to five times the typical one.)  Asserted: the median drop of either kind,
    and more than half of them, pass the Gaussian bar unseen; the exact patterns catch every one (test_drop_one_piece_is_caught_*)."""
    s = dict(tk.CONV_BY_NAME[name], B=1)
    h = tk._conv_host(s, np.random.default_rng(sum(map(ord, name))))
    ref_max = float(np.abs(tk._conv_finish(h, h["res"])).max())
    clean = hx.gaussian_drop_error(s, h, ("al_bh", 27, 0), ref_max)     # (tap 27 does not exist: nothing dropped)
    assert clean < 1e-6
    for term in hx.TERMS:
        slots = np.array([hx.gaussian_drop_error(s, h, (term, tap, slot), ref_max) for tap in range(27) for slot in range(s["c1"] // 8)])
        ones = np.array([hx.gaussian_drop_error(s, h, (term, tap, (5 * tap + j) % s["c1"]), ref_max, channels=1) for tap in range(27) for j in (0, 13)])
        print(f"{name} {term}: one (tap, ci) dropped: worst {ones.max():.2e}; one (tap, slot): median {np.median(slots):.2e}, worst {slots.max():.2e}, "
              f"{(slots < tk.LAYER_TOL).mean():.0%} under {tk.LAYER_TOL}")
        assert clean < ones.min()
        for errs in (ones, slots):
            assert np.median(errs) < tk.LAYER_TOL and (errs < tk.LAYER_TOL).mean() > 0.5


def test_gemm_and_mlp_models():
    for pattern in hx.PATTERNS:
        p = hx.gemm_problem(pattern, 33, 16, 48, 1, 0, 1, "n", 2, tk.RELU, 0.5)
        ref = np.einsum("mk,nk->mn", p["a"][0].astype(np.float64), p["b"][0].astype(np.float64))
        got = hx.h3_contract(p["a"][0], np.ascontiguousarray(p["b"][0].T), 48, _perm(3)).astype(np.float64)
        if pattern in hx.EXACT:
            assert np.array_equal(got, ref)
        else:
            assert (np.abs(got - ref) <= hx.BOTH_LO_TOL * p["prod_abs"][0] / 0.5).all()
    for k in (16, 48, 272):
        for pattern in hx.EXACT:
            hx.gemm_problem(pattern, 200, 144, k, 2, 1, 0, "m", 2, tk.NONE, 2.0)
    p = hx.mlp_problem(8)
    for o in range(ORDERS):
        got, hid = hx.mlp_contract(p, _perm(o))
        assert np.array_equal(hid.astype(np.float64), p["hidden"]) and np.array_equal(got.astype(np.float64), p["ref"])
    got, _ = hx.mlp_contract(p, drop=("al_bh", 0, 5))
    assert _caught(got, p["ref"], p["q"])
