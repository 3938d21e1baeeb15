"""Constructed logit rows for the attention and softmax entries of the C ABI (plain helper, numpy only, no test in it;
tests/test_attention_logits_host.py checks it on the CPU, tests/test_gpu_attention_logits.py feeds it to the kernels).

The random attention tests draw q and k from N(0, 0.7^2): their logits lie within about +-2 of each other, so the lazy running maximum of
csrc/dm3d_attn_h3.hip moves on tile 0 and never again, and the float16 hi + lo split of the probabilities never meets a value near its
subnormal step.  Here the score matrix S (in post-scale units: what goes into exp) is BUILT, and q, k are derived from it:

  unit keys (the score matrix fits the channels: lk <= c, or S has period c along the keys):
      k[j] = a e_(j mod c),  q[i] = S[i, :c] / (a scale)          ->  score(i, j) = S[i, j mod c]
  row kinds (any lk, at most c different rows in S):
      q[i] = e_kind(i) / (a scale),  k[j] = a sum_g S_g[j] e_g    ->  score(i, j) = S_kind(i)[j]
      (the same idea with the roles of q and k exchanged: the 4096-key rows of `stairs_*` and `tail_floor` do not repeat after 256 keys)

with a and scale powers of two.  Either way a score is ONE product of the contraction, and every pattern but `tail_floor` uses logits that
are multiples of 1/4, so the operands are exact in DM3D_FMT_H2 and the kernels see S itself; the float64 reference is computed from the
decoded operands all the same (`attention_problem`), as tests/test_gpu_infer_kernels.py::_attn_problem does.

`branch_trace` is a numpy model of the lazy-maximum rule as the comment in csrc/dm3d_attn_h3.hip states it (a model of the documented
rule, not a probe of the kernel: if the rule changes, this function and DESIGN.md section 4.4 change with it).  `bound` is what a case
may miss the float64 reference by, `emulate_h2_probabilities` what the float16 split of the probabilities alone costs."""
import zlib

import numpy as np

from guarded_buffers import h2_decode, h2_encode

# The project's bars, max |err| / max |ref| (tests/test_gpu_infer_kernels.py, "Tolerances": contractions 2e-5, row kernels 3e-6).
LAYER_TOL, ROW_TOL = 2e-5, 3e-6
TILE, WAVE_ROWS, THRESHOLD = 32, 32, 8.0      # keys per tile, queries per wave, the lazy maximum's slack (csrc/dm3d_attn_h3.hip)
F16_MAX = 65504.0
F32_EPS = 2.0 ** -24                           # relative rounding error of a float32
H2_FLOOR = 2.0 ** -25                          # a float16 steps by 2^-24 below 2^-14: hi + lo loses up to half a step per probability
LOW, DROP = -30.0, 4.0                         # one_hot's other logits; how far a tile's other keys sit below its maximum
MOVER = 5                                      # the query of a wave that `lone_mover` singles out
PEAK = 3                                       # tail_floor's logit 0: in tile 0, so that every other key of the row is split against it


# ---- rows (float64 [lk]) -----------------------------------------------------------------------------------------------------------------
def _peak_of_tile(t, n):
    """Where inside tile t (n keys long: the last tile of a row may be short) the tile's maximum sits: it wanders through the tile."""
    return min((7 * t + 3) % TILE, n - 1)


def row_flat(lk, level=0.0):
    return np.full(lk, float(level))


def row_one_hot(lk, j):
    r = np.full(lk, LOW)
    r[j] = 0.0
    return r


def row_stairs(lk, step, down=False):
    """The maximum of 32-key tile t is step * t (down: -step * t), the rest of the tile DROP below it."""
    r = np.empty(lk)
    for t in range(-(-lk // TILE)):
        n = min(TILE, lk - t * TILE)
        top = (-step if down else step) * t
        r[t * TILE:t * TILE + n] = top - DROP
        r[t * TILE + _peak_of_tile(t, n)] = top
    return r


def row_tail_floor(lk, delta):
    r = np.full(lk, -float(delta))
    r[min(PEAK, lk - 1)] = 0.0
    return r


# ---- score matrices (float64 [lq, lk]) -------------------------------------------------------------------------------------------------
def _rows(lq, *kinds):
    """Query i takes kinds[i % len(kinds)]."""
    return np.stack([kinds[i % len(kinds)] for i in range(lq)])


def flat(level):
    return lambda lq, lk: _rows(lq, row_flat(lk, level))


def one_hot(j):
    """j: a key, or "last"."""
    return lambda lq, lk: _rows(lq, row_one_hot(lk, lk - 1 if j == "last" else j))


def stairs_up(step):
    return lambda lq, lk: _rows(lq, row_stairs(lk, step))


def stairs_down(step):
    return lambda lq, lk: _rows(lq, row_stairs(lk, step, down=True))


def lone_mover(flat_one=False):
    """Within each block of 32 queries, query MOVER follows stairs_up(8.5) and the other 31 are flat (flat_one: the other way round)."""
    def build(lq, lk):
        up, level = row_stairs(lk, 8.5), row_flat(lk)
        return np.stack([up if (i % WAVE_ROWS == MOVER) != flat_one else level for i in range(lq)])
    return build


def mixed_wave(lq, lk):
    """Queries alternate stairs_up(7.5), stairs_down(8.5), one_hot, flat: every lane of a wave has its own history of rescales."""
    return _rows(lq, row_stairs(lk, 7.5), row_stairs(lk, 8.5, down=True), row_one_hot(lk, min(TILE + 5, lk - 1)), row_flat(lk))


def tail_floor(delta):
    return lambda lq, lk: _rows(lq, row_tail_floor(lk, delta))


def offset(c0):
    return lambda lq, lk: mixed_wave(lq, lk) + float(c0)


# name -> builder.  tail_floor: 17.2 puts every tail probability at exp(-17.2) = 3.4e-8, just above 2^-25 = 2.98e-8 (float16 rounds it UP to
# 2^-24), 17.4 at 2.8e-8, just below (rounds to 0).  It alone has the H2 floor term in its bound.
PATTERNS = {
    "flat(0)": flat(0.0),
    "flat(-3.25)": flat(-3.25),
    "one_hot(0)": one_hot(0),
    "one_hot(31)": one_hot(31),
    "one_hot(32)": one_hot(32),
    "one_hot(last)": one_hot("last"),
    "stairs_up(7.5)": stairs_up(7.5),
    "stairs_up(8.5)": stairs_up(8.5),
    "stairs_down(8.5)": stairs_down(8.5),
    "lone_mover(one rises)": lone_mover(),
    "lone_mover(one flat)": lone_mover(flat_one=True),
    "mixed_wave": mixed_wave,
    "tail_floor(17.2)": tail_floor(17.2),
    "tail_floor(17.4)": tail_floor(17.4),
    "offset(+64)": offset(64),
    "offset(-64)": offset(-64),
}
FLOOR_PATTERNS = ("tail_floor",)
LONG_PATTERNS = [n for n in PATTERNS if n.startswith(("stairs", "lone_mover", "mixed_wave", "tail_floor"))]      # also run at lk = 4096


def pattern_names(lk, names=None):
    """The patterns that exist at lk keys: one_hot(31) is one_hot(last) at lk = 32, and key 32 needs a second tile."""
    out = []
    for n in (PATTERNS if names is None else names):
        if (n == "one_hot(31)" and lk - 1 <= 31) or (n == "one_hot(32)" and lk - 1 <= 32):
            continue
        out.append(n)
    return out


def scores(name, lq, lk):
    return PATTERNS[name](lq, lk)


def softmax_rows_matrix(cols):
    """(names, S [rows, cols]) for dm3d_softmax_rows[_h2]: one pattern per row, as float32 holds it.  one_hot at 0, 63, 64 and cols - 1:
    first element, last lane of the first 64-stride of a wave, first lane of the second, last element.  The two offset rows are the
    rising and the falling stairs of mixed_wave, shifted."""
    rows = [("flat(0)", row_flat(cols)), ("flat(-3.25)", row_flat(cols, -3.25))]
    rows += [(f"one_hot({j})", row_one_hot(cols, j)) for j in sorted({0, 63, 64, cols - 1}) if j < cols]
    rows += [("stairs_up(7.5)", row_stairs(cols, 7.5)), ("stairs_up(8.5)", row_stairs(cols, 8.5)), ("stairs_down(8.5)", row_stairs(cols, 8.5, down=True))]
    rows += [("tail_floor(17.2)", row_tail_floor(cols, 17.2)), ("tail_floor(17.4)", row_tail_floor(cols, 17.4))]
    rows += [("offset(+64)", row_stairs(cols, 7.5) + 64.0), ("offset(-64)", row_stairs(cols, 8.5, down=True) - 64.0)]
    return [n for n, _ in rows], np.stack([r for _, r in rows]).astype(np.float32).astype(np.float64)


# ---- operands ------------------------------------------------------------------------------------------------------------------------------
def operands(S, c, scale, a=16.0):
    """S [..., lq, lk] -> float32 q [..., lq, c], k [lk, c] with q k^T scale = S (see the module docstring for the two constructions)."""
    S = np.asarray(S, np.float64)
    lk = S.shape[-1]
    assert np.log2(a) % 1 == 0 and np.log2(scale) % 1 == 0, "a and scale are powers of two: dividing by them is exact"
    q, k = np.zeros(S.shape[:-1] + (c,)), np.zeros((lk, c))
    if lk <= c or np.array_equal(S, S[..., np.arange(lk) % c]):
        k[np.arange(lk), np.arange(lk) % c] = a
        q[..., :min(lk, c)] = S[..., :c] / (a * scale)
    else:
        kinds, which = np.unique(S.reshape(-1, lk), axis=0, return_inverse=True)
        assert len(kinds) <= c, f"{len(kinds)} different rows do not fit {c} channels"
        k[:, :len(kinds)] = a * kinds.T
        q.reshape(-1, c)[np.arange(which.size), which.reshape(-1)] = 1.0 / (a * scale)
    return q.astype(np.float32), k.astype(np.float32)


def seeded(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def values(rng, kind, *shape):
    """v: "zero_mean" N(0, 1), or "with_mean" 1 + 0.25 N(0, 1) — under which lost or inflated tail mass no longer averages away."""
    g = rng.standard_normal(shape)
    return ({"zero_mean": g, "with_mean": 1.0 + 0.25 * g}[kind]).astype(np.float32)


def softmax64(S):
    S = np.asarray(S, np.float64)
    e = np.exp(S - S.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


RES_STD = 0.25       # the residual is kept smaller than the attention output: max |ref| is the scale of every bound


def attention_problem(name, B, lq, lk, c, fmt, bcast, v_kind="zero_mean", res=True):
    """The dict tests/test_gpu_infer_kernels.py::_attn_desc takes (q / k / v^T as float32, or as DM3D_FMT_H2 words when fmt), plus S, the
    decoded v and the float64 reference of the decoded operands.  Sample b of a batch has its queries rolled by b, so that the waves of
    the two samples hold different lanes.  The offset patterns draw the v and residual of mixed_wave, which they are compared with."""
    rng = seeded("mixed_wave" if name.startswith("offset") else name, B, lq, lk, c, fmt, bcast, v_kind)
    scale = 2.0 ** np.floor(np.log2(float(c) ** -0.5))          # c^-0.5 where that is a power of two (c = 256, 64), the next one below otherwise
    S = np.stack([np.roll(scores(name, lq, lk), b, axis=0) for b in range(B)])
    q, k = operands(S, c, scale)
    nb = 1 if bcast else B
    k = np.ascontiguousarray(np.broadcast_to(k, (nb, lk, c)))
    v = values(rng, v_kind, nb, lk, c)
    vt = np.ascontiguousarray(v.transpose(0, 2, 1))
    p = dict(name=name, B=B, lq=lq, lk=lk, c=c, fmt=fmt, bcast=bcast, scale=float(scale), v_kind=v_kind, S=S)
    p["qw"], p["kw"], p["vtw"] = (h2_encode(t) if fmt else t for t in (q, k, vt))
    q, k, vt = (h2_decode(p[w]) if fmt else p[w].astype(np.float64) for w in ("qw", "kw", "vtw"))
    p["res"] = (rng.standard_normal((B, lq, c)) * RES_STD).astype(np.float32) if res else None
    p["v"] = np.broadcast_to(vt.transpose(0, 2, 1), (B, lk, c))
    p["scores"] = np.einsum("blc,bkc->blk", q, np.broadcast_to(k, (B, lk, c))) * scale
    p["ref"] = softmax64(p["scores"]) @ p["v"] + (0.0 if p["res"] is None else p["res"].astype(np.float64))
    return p


# ---- the lazy running maximum ----------------------------------------------------------------------------------------------------------
def branch_trace(S, tile=TILE, wave_rows=WAVE_ROWS, threshold=THRESHOLD):
    """The rule of csrc/dm3d_attn_h3.hip on score rows S [lq, lk]: per tile a query's maximum mloc; `moved = mloc > m_run + threshold`
    (m_run starts at -inf); if ANY query of the wave moved, EVERY query of it takes m_new = max(m_run, mloc), scales its accumulators and
    its row sum by alpha = exp(m_run - m_new) and goes on with m_run = m_new; then p = exp(s - m_run) goes into the float16 split.
    Returns fired [waves, tiles] (bool), alpha [lq, tiles], pmax [lq] (the largest p of the query) and l [lq] (its final row sum)."""
    S = np.asarray(S, np.float64)
    lq, lk = S.shape
    assert lq % wave_rows == 0
    nt = -(-lk // tile)
    fired, alpha = np.zeros((lq // wave_rows, nt), bool), np.ones((lq, nt))
    m_run, l_run, pmax = np.full(lq, -np.inf), np.zeros(lq), np.zeros(lq)
    for t in range(nt):
        s = S[:, t * tile:(t + 1) * tile]
        mloc = s.max(-1)
        moved = mloc > m_run + threshold
        fired[:, t] = moved.reshape(-1, wave_rows).any(-1)
        wave_fired = np.repeat(fired[:, t], wave_rows)
        m_new = np.where(wave_fired, np.maximum(m_run, mloc), m_run)
        with np.errstate(invalid="ignore"):
            alpha[:, t] = np.where(m_new > m_run, np.exp(m_run - m_new), 1.0)       # exp(-inf) = 0 on the first tile
        m_run = m_new
        p = np.exp(s - m_run[:, None])
        pmax = np.maximum(pmax, p.max(-1))
        l_run = l_run * alpha[:, t] + p.sum(-1)
    return dict(fired=fired, alpha=alpha, pmax=pmax, l=l_run)


# ---- what the float16 split of the probabilities costs -------------------------------------------------------------------------------------
def h2_round(P):
    """float32(P) through the DM3D_FMT_H2 coder: hi + lo as the kernels store or multiply it."""
    P = np.asarray(P, np.float32)
    pad = -P.shape[-1] % 16
    W = h2_encode(np.pad(P, [(0, 0)] * (P.ndim - 1) + [(0, pad)]))
    return h2_decode(W)[..., :P.shape[-1]]


def emulate_h2_probabilities(S, v):
    """softmax(S) in float64, pushed through float16 hi + lo, times v, over the UNSPLIT row sum (l_run of the fused kernel and the row
    sum of softmax_rows_h2 are summed from the float32 values): everything exact but the split."""
    P = softmax64(S)
    return (h2_round(P) @ np.asarray(v, np.float64)) / P.sum(-1, keepdims=True)


# ---- the bound ---------------------------------------------------------------------------------------------------------------------------
def score_term(S):
    """A float32 score carries an absolute error of about |S| 2^-24, which exp turns into the same RELATIVE error of p, numerator and
    row sum alike: 2 max|S| 2^-24.  Next to nothing (<= 4e-6) for all patterns but `offset` and the 4096-key stairs."""
    return 2.0 * float(np.abs(S).max()) * F32_EPS


def bound(entry, name, S, h2, v=None, ref=None):
    """The allowed max |err| / max |ref| of a case, as (total, {term: value}).
    entry: "attention" or "softmax_rows"; h2: the probabilities pass through float16 hi + lo on the way (the fused form, the three-launch
    form with fmt = H2, softmax_rows_h2).
      bar    the project's own: LAYER_TOL for the attention entries, ROW_TOL for softmax_rows.
      score  score_term(S).
      floor  only for FLOOR_PATTERNS (tail_floor) on an h2 path: each probability may be off by H2_FLOOR = 2^-25, so the
             output by at most lk 2^-25 max|v| (after normalisation: the row sum is >= 1, the reference maximum never exceeding the
             true one), relative to max|ref|; for softmax_rows_h2, whose output is the probabilities, 2^-25 per element.
             (The three-launch form with precision H3 on float32 operands splits P inside its GEMM as well; at the lk <= 112 it is run
             with here that is at most 112 * 2^-25 = 3.3e-6, which LAYER_TOL carries.)"""
    terms = {"bar": LAYER_TOL if entry == "attention" else ROW_TOL, "score": score_term(S), "floor": 0.0}
    if h2 and name.startswith(FLOOR_PATTERNS):
        refmax = float(np.abs(ref).max())
        terms["floor"] = (S.shape[-1] * H2_FLOOR * float(np.abs(v).max()) if entry == "attention" else H2_FLOOR) / refmax
    return sum(terms.values()), terms


def describe(terms):
    return " + ".join(f"{k} {x:.2e}" for k, x in terms.items() if x)
