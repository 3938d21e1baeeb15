"""CPU checks of tests/attention_logit_cases.py: every constructed pattern drives the branch of the lazy running maximum it is listed for
(`branch_trace`, the rule as csrc/dm3d_attn_h3.hip documents it), survives the DM3D_FMT_H2 rounding of its operands, and — with
everything exact but the float16 hi + lo split of the probabilities (`emulate_h2_probabilities`) — uses at most half of its `bound`,
while `tail_floor` under a v with a mean demonstrably needs the floor term of that bound.  No GPU, no library call."""
import numpy as np
import pytest

import attention_logit_cases as lc

LQ = 128                                    # one workgroup of the fused kernel: four waves of 32 queries
FUSED_LKS = (32, 64, 256, 4096)
E = np.exp


def _fused_cases():
    """(pattern, lk, v kind) as tests/test_gpu_attention_logits.py runs the fused form."""
    out = []
    for lk in FUSED_LKS:
        for name in lc.pattern_names(lk, lc.LONG_PATTERNS if lk == 4096 else None):
            for kind in (("zero_mean", "with_mean") if name.startswith("tail_floor") else ("zero_mean",)):
                out.append((name, lk, kind))
    return out


def _trace(name, lk):
    return lc.branch_trace(lc.scores(name, LQ, lk))


# ---- branch_trace: each pattern drives what it is listed for ---------------------------------------------------------------------------
@pytest.mark.parametrize("lk", FUSED_LKS)
def test_flat_and_one_hot_move_on_tile_0_only(lk):
    for name in lc.pattern_names(lk, [n for n in lc.PATTERNS if n.startswith(("flat", "tail_floor"))] + ["one_hot(0)", "one_hot(31)"]):
        tr = _trace(name, lk)
        assert tr["fired"][:, 0].all() and not tr["fired"][:, 1:].any(), name
    for name in lc.pattern_names(lk, ["one_hot(32)", "one_hot(last)"]):          # the logit 0 arrives in a later tile: one more move, by 30
        if lk > lc.TILE:
            tr, t_hot = _trace(name, lk), (32 if name == "one_hot(32)" else lk - 1) // lc.TILE
            assert tr["fired"].sum(-1).tolist() == [2] * 4 and tr["fired"][:, t_hot].all(), name
            assert np.allclose(tr["alpha"][:, t_hot], E(lc.LOW))


@pytest.mark.parametrize("lk", [64, 256, 4096])
def test_stairs(lk):
    nt = lk // lc.TILE
    up85, up75, down = _trace("stairs_up(8.5)", lk), _trace("stairs_up(7.5)", lk), _trace("stairs_down(8.5)", lk)
    assert up85["fired"].all(), "a step of 8.5 moves the reference on every tile"
    assert np.allclose(up85["alpha"][:, 1:], E(-8.5)) and np.allclose(up85["pmax"], 1.0)
    # a step of 7.5: the reference lags by 7.5 on the odd tiles (no move, p up to e^7.5 into the float16 split) and catches up by 15 on the even ones
    assert up75["fired"].tolist() == [[t % 2 == 0 for t in range(nt)]] * 4
    assert np.allclose(up75["alpha"][:, 2::2], E(-15.0)) and (up75["alpha"][:, 1::2] == 1.0).all()
    assert (up75["pmax"] > E(7.0)).all() and np.allclose(up75["pmax"], E(7.5))
    assert down["fired"][:, 0].all() and not down["fired"][:, 1:].any(), "the maximum sits in tile 0: the reference never moves again"
    assert np.allclose(down["l"], 1.0 + 31 * E(-lc.DROP) + sum(E(-8.5 * t) * (1.0 + 31 * E(-lc.DROP)) for t in range(1, nt)))


@pytest.mark.parametrize("lk", [64, 256, 4096])
def test_lone_mover(lk):
    """One lane trips the ballot of its wave on every tile; the lanes that do not move take alpha == 1 exactly."""
    rows = np.arange(LQ)
    for name, movers in (("lone_mover(one rises)", rows % lc.WAVE_ROWS == lc.MOVER), ("lone_mover(one flat)", rows % lc.WAVE_ROWS != lc.MOVER)):
        tr = _trace(name, lk)
        assert tr["fired"].all(), name
        assert movers.sum() == (4 if "rises" in name else 4 * 31)
        assert (tr["alpha"][~movers, 1:] == 1.0).all() and np.allclose(tr["alpha"][movers, 1:], E(-8.5)), name
        assert np.allclose(tr["l"][~movers], lk)                                   # flat rows: lk probabilities of 1


@pytest.mark.parametrize("lk", [64, 256, 4096])
def test_mixed_wave_gives_every_kind_of_lane_its_own_history(lk):
    tr = _trace("mixed_wave", lk)
    nt = lk // lc.TILE
    # one_hot's key 37 trips the ballot on tile 1 and drags the stairs_up(7.5) lanes along (by 7.5, which alone would not have moved them):
    # their alternation then falls on the odd tiles
    assert tr["fired"].tolist() == [[t == 0 or t % 2 == 1 for t in range(nt)]] * 4
    a = tr["alpha"]
    assert (a[1::4, 1:] == 1.0).all() and (a[3::4, 1:] == 1.0).all(), "stairs_down and flat lanes never move while their neighbours do"
    assert np.allclose(a[2::4, 1], E(lc.LOW)) and (a[2::4, 2:] == 1.0).all()
    assert np.allclose(a[0::4, 1], E(-7.5)) and np.allclose(a[0::4, 3::2], E(-15.0)) and (a[0::4, 2::2] == 1.0).all()
    for c0 in (64, -64):                                                            # a common shift changes nothing past tile 0
        sh = _trace(f"offset({c0:+d})", lk)
        assert np.array_equal(sh["fired"], tr["fired"]) and np.array_equal(sh["alpha"], a) and np.array_equal(sh["pmax"], tr["pmax"])


@pytest.mark.parametrize("name,lk,kind", _fused_cases())
def test_probabilities_fit_float16(name, lk, kind):
    """Nothing that goes into the split exceeds exp(THRESHOLD), far below the largest float16."""
    pmax = _trace(name, lk)["pmax"]
    assert pmax.max() <= E(lc.THRESHOLD) < lc.F16_MAX and pmax.min() >= 1.0 - 1e-12


# ---- the operands ----------------------------------------------------------------------------------------------------------------------
def _problems():
    out = [(n, 1, LQ, lk, 256, True, k) for n, lk, k in _fused_cases()] + [("mixed_wave", 2, LQ, 64, 256, True, "zero_mean")]
    three = ["flat(0)", "flat(-3.25)", "one_hot(0)", "one_hot(31)", "one_hot(32)", "one_hot(last)", "stairs_up(8.5)", "mixed_wave",
             "tail_floor(17.2)", "tail_floor(17.4)", "offset(+64)", "offset(-64)"]
    return out + [(n, 2, 64, lk, 32, True, "zero_mean") for lk in (48, 112) for n in three]


_CACHE = {}


def _problem(name, B, lq, lk, c, h2, kind):
    key = (name, B, lq, lk, c, h2, kind)
    if key not in _CACHE:
        _CACHE.clear()                                        # one at a time: a 4096-key problem holds some 20 MB
        _CACHE[key] = lc.attention_problem(name, B, lq, lk, c, 1 if h2 else 0, B > 1 and c == 256, kind)
    return _CACHE[key]


@pytest.mark.parametrize("case", _problems(), ids=lambda c: f"{c[0]}-B{c[1]}-lk{c[3]}-c{c[4]}-{c[6]}")
def test_pattern_survives_its_operands(case):
    """|q|, |k| inside float16 range, everything finite, and the scores of the DECODED operands are the pattern: exactly where its logits
    are multiples of 1/4, within the 2^-21 of a DM3D_FMT_H2 value for tail_floor — whose tail stays on its side of 2^-25."""
    p = _problem(*case)
    for w in ("qw", "kw", "vtw"):
        x = lc.h2_decode(p[w])
        assert np.isfinite(x).all() and np.abs(x).max() < lc.F16_MAX
    assert np.isfinite(p["ref"]).all() and np.isfinite(p["S"]).all()
    if case[0].startswith("tail_floor"):
        assert np.abs(p["scores"] - p["S"]).max() <= np.abs(p["S"]).max() * 2.0 ** -21
        tail = np.sort(lc.softmax64(p["scores"]), -1)[..., :-1]
        lo, hi = (1.0, 1.5) if "17.2" in case[0] else (0.5, 1.0)
        assert (tail > lo * lc.H2_FLOOR).all() and (tail < hi * lc.H2_FLOOR).all()
    else:
        assert np.array_equal(p["scores"], p["S"])


# ---- the bound against the emulated split ----------------------------------------------------------------------------------------------
def _emulated(p):
    """(error of the emulated split, max |ref|): the reference's own scores and v, only the probabilities rounded."""
    got = lc.emulate_h2_probabilities(p["scores"], p["v"]) + p["res"]
    return float(np.abs(got - p["ref"]).max()), float(np.abs(p["ref"]).max())


@pytest.mark.parametrize("case", _problems(), ids=lambda c: f"{c[0]}-B{c[1]}-lk{c[3]}-c{c[4]}-{c[6]}")
def test_emulated_split_uses_at_most_half_the_bound(case):
    p = _problem(*case)
    err, refmax = _emulated(p)
    total, terms = lc.bound("attention", p["name"], p["S"], True, p["v"], p["ref"])
    print(f"{case}: emulated {err / refmax:.2e} of bound {total:.2e} = {lc.describe(terms)}")
    assert err / refmax <= 0.5 * total
    assert (terms["floor"] > 0) == case[0].startswith("tail_floor"), "the floor term is taken for tail_floor alone"


@pytest.mark.parametrize("case", [c for c in _problems() if c[0].startswith("tail_floor") and c[6] == "with_mean"], ids=lambda c: f"{c[0]}-lk{c[3]}")
def test_tail_floor_exercises_the_floor(case):
    """Under v = 1 + 0.25 N every tail probability errs the same way (17.2: up to 2^-24, 17.4: down to 0), so the output is off by about
    (lk - 1) * 2.6e-8 (2.8e-8): at least a quarter of the floor lk * 2^-25.  At 4096 keys that alone is past the bound without its floor
    term, so the floor term is what lets the case pass — and a kernel that lost more than the format does would not."""
    p = _problem(*case)
    err, refmax = _emulated(p)
    lk = case[3]
    assert err >= 0.25 * lk * lc.H2_FLOOR
    total, terms = lc.bound("attention", p["name"], p["S"], True, p["v"], p["ref"])
    if lk == 4096:              # (lk * 2^-25 reaches LAYER_TOL only from 672 keys on: the shorter rows exercise the rounding, not the bound)
        assert err / refmax > total - terms["floor"], "the case would pass with the floor term removed"
        with_zero_mean = _emulated(_problem(*case[:6], "zero_mean"))[0]
        assert with_zero_mean < 0.25 * err, "with a zero-mean v the same loss averages away"


@pytest.mark.parametrize("cols", [8, 64, 100, 256, 512, 1024, 1040, 4112])
def test_softmax_rows_matrix(cols):
    """The matrix the softmax_rows tests use: its H2 rounding alone — per element 2^-25 absolute below the float16 normals, 2^-22 relative
    above (hi and lo carry 11 bits each) — stays within half the bound."""
    names, S = lc.softmax_rows_matrix(cols)
    assert np.isfinite(S).all() and len(set(names)) == len(names)
    P = lc.softmax64(S)
    err = np.abs(lc.h2_round(P) - P)
    assert (err <= lc.H2_FLOOR + P * 2.0 ** -22).all()
    err = err.max(-1)
    for n, s, e in zip(names, S, err):
        total, terms = lc.bound("softmax_rows", n, s[None], True, ref=P)
        assert e / P.max() <= 0.5 * total and (terms["floor"] > 0) == n.startswith("tail_floor")
