"""What the tests of the normalisation statistics under a mean offset share (plain helper, no test in it): the inputs, float32
restatements of each kernel's summation order beside the float64 references of oracle/ref_kernels.py, and the bars.
tests/test_norm_offsets_host.py holds the models to float64 on the CPU and pins their errors (tests/golden/norm_offset_model_errors.json);
tests/test_gpu_norm_offsets.py holds the HIP kernels to the bars built from them.

The inputs.  x = offset + std * N(0, 1) in float32, offset = +-r * std, r = |mean| / std in R_VALUES.  A kernel that forms
E[x^2] - m^2 from sums rounded to float32 loses about r^2 * 2^-24 of the variance, so r is the axis that matters.  For the
per-channel statistics (BatchNormalization) the sign changes from channel to channel.  For GroupNormalization the sign is constant
within a group and changes from group to group: mixed signs inside one group would turn the offset into spread (group variance about
r^2 std^2) and test nothing.  mode="one" puts the offset on the first channel of every group only.  mode="lattice" (r = 100) replaces the
noise by integers in {-1, 0, 1}: every 64-voxel slot sum is then exact in float32, the slot model's error is 0 and the bar LAYER_TOL, while
the sum over slots and channels needs more than 24 bits: the case that tells a float64 dm3d_groupnorm_finalize2 from a float32 one.
For the row kernels (LayerNormalization) the offset is per row.

The models, each in its kernel's own operation order (csrc/dm3d_elem.hip, csrc/dm3d_train.hip):
  stats_chain     groupnorm_stats_kernel: slabs = clamp(voxels / (vox_par * 16), 1, 64) blocks per sample, vox_par = 256 / min(c/4, 256)
                  voxel lanes per block; a thread adds the voxels v0 + vl, v0 + vl + vox_par, ... of its slab one after the other; the
                  partials of a quad and the slabs are then added in float64.  dtype=float64 is the kernel as it stands; dtype=float32 the
                  per-thread sums it kept before (s += t, ss += t*t with the product rounded), kept here as the measured reason.
  slot_partials   groupnorm_partials_kernel: per (sample, 64-voxel slot, channel) s += t and q = fmaf(t, t, q) in voxel order, stored as
                  float32; groupnorm_finalize2_kernel adds slots and channels in float64.  The conv epilogues' gn_stats has the same
                  layout with a tile order of its own; it is held to the same model.
  ln_stats        the row kernels (layernorm3, layernorm3_h2, layernorm_bwd): two passes over a row held in registers, a float32 mean
                  (lane sums in the kernel's order, xor butterfly across the 64 lanes) and a float32 sum of squared deviations.
  ln_stats_one_pass   what those kernels must never become: E[x^2] - m^2 in float32.  The negative control of the row cases.
  bn_act_bwd_f32  dm3d_bn_act_bwd on float32 scale / shift / mean / rstd: u = fma(x, scale, shift) carries r * 2^-24 whatever the
                  statistics kernel does, since shift itself is a float32 of magnitude r.

The bars.  err(got, ref) = max |got - ref| / max |ref|, as tests/test_gpu_train_kernels.py measures.  bar(existing, model_err) =
max(existing, 4 * model_err) with the factor of tests/metrics_reference.py (FMA contraction, another but fixed summation order);
model_err is the model's error against float64 on the very input, computed from the references alone.  existing is LAYER_TOL for
statistics and ROW_TOL for row kernels.  A kernel that accumulates in float64 has a float64-ordered model, whose error stays
under 1e-9: its bar is the existing one at every r."""
import functools
import json
import os

import numpy as np
import torch

from oracle import ref_kernels as rk

LAYER_TOL, ROW_TOL = 2e-5, 3e-6
MARGIN = 4.0
EPS = 1e-3
R_VALUES = (0, 10, 30, 100, 1000)
STD = 1.5                                  # of the statistics inputs
LN_STD = 2.0                               # of the row inputs
MOMENTUM = 0.9
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "norm_offset_model_errors.json")

# (batch, voxels, c): 37 voxels in one ragged slab; c = 12: 85 voxel lanes, one idle thread; six slabs of 28 lanes; c > 1024: the quad loop runs twice
BN_SHAPES = [(2, 37, 20), (3, 321, 12), (2, 3000, 36), (1, 4096, 1028)]
# (batch, voxels, c1, c2, groups): group 2 of 20 | 12 straddles the two inputs (and V = 70 leaves a slot of 6 voxels); 47 slots; 64 groups
GN_SHAPES = [(2, 70, 20, 12, 4), (2, 3000, 60, 40, 4), (1, 65, 1024, 1024, 64)]
LN_SHAPES = [(5, 48), (1025, 256), (5, 1024)]                       # (rows, c): one lane group; a ragged last block; the widest row
BN_BWD_SHAPE = (1031, 12, 24)                                       # (rows, c1, c2)
BN_BWD_R = (0, 30)
GN_RUNS = [(r, "mixed") for r in R_VALUES] + [(1000, "one"), (100, "lattice")]          # (r, mode) of the GroupNormalization cases
CONV_R = (0, 10, 100)


def shape_id(shape):
    return "x".join(str(int(v)) for v in shape)


def err(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.abs(got - ref).max() / max(float(np.abs(ref).max()), 1e-30))


def bar(existing, model_err):
    return max(existing, MARGIN * model_err)


def _t64(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


# ---- inputs --------------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31)


def channel_offsets(c, r, std=STD, groups=None, mode="mixed"):
    """Per-channel offsets: +-r*std alternating per channel (groups None), per group (mode "mixed"), or r*std on the first channel of
    every group and 0 elsewhere (mode "one")."""
    if groups is None:
        sign = np.where(np.arange(c) % 3 == 1, -1.0, 1.0)
        return sign * r * std
    gc = c // groups
    g = np.arange(c) // gc
    if mode == "one":
        return np.where(np.arange(c) % gc == 0, r * std, 0.0)
    return np.where(g % 2 == 1, -1.0, 1.0) * r * std


@functools.lru_cache(maxsize=None)
def stats_input(batch, voxels, c, r, groups=None, mode="mixed"):
    """float32 [batch, voxels, c] (read-only), gamma, beta [c]."""
    rng = np.random.default_rng(_seed(batch, voxels, c, r, groups or 0, ("mixed", "one", "lattice").index(mode)))
    noise = rng.integers(-1, 2, (batch, voxels, c)) if mode == "lattice" else STD * rng.standard_normal((batch, voxels, c))
    x = (channel_offsets(c, r, STD, groups, mode)[None, None, :] + noise).astype(np.float32)
    gamma = (1.0 + 0.3 * rng.standard_normal(c)).astype(np.float32)
    beta = (0.5 * rng.standard_normal(c)).astype(np.float32)
    for a in (x, gamma, beta):
        a.setflags(write=False)
    return x, gamma, beta


@functools.lru_cache(maxsize=None)
def moving_input(c):
    rng = np.random.default_rng(_seed(c, 99))
    mm, mv = rng.standard_normal(c).astype(np.float32), (np.abs(rng.standard_normal(c)) + 0.1).astype(np.float32)
    mm.setflags(write=False), mv.setflags(write=False)
    return mm, mv


@functools.lru_cache(maxsize=None)
def row_input(rows, c, r):
    """x (per-row offsets +-r*LN_STD), dy float32 [rows, c]; three (gamma, beta) pairs."""
    rng = np.random.default_rng(_seed(rows, c, r, 5))
    off = np.where(np.arange(rows) % 3 == 1, -1.0, 1.0) * r * LN_STD
    x = (off[:, None] + LN_STD * rng.standard_normal((rows, c))).astype(np.float32)
    dy = rng.standard_normal((rows, c)).astype(np.float32)
    params = tuple(((rng.random(c) + 0.5).astype(np.float32), rng.standard_normal(c).astype(np.float32)) for _ in range(3))
    for a in (x, dy) + tuple(p for gb in params for p in gb):
        a.setflags(write=False)
    return x, dy, params


# ---- groupnorm_stats_kernel ------------------------------------------------------------------------------------------------------------
def stats_launch(voxels, c):
    """(slabs, slab length, vox_par) of dm3d_groupnorm_stats."""
    lanes = min(c // 4, 256)
    vox_par = 256 // lanes
    slabs = min(max(voxels // (vox_par * 16), 1), 64)
    return slabs, -(-voxels // slabs), vox_par


def stats_chain(x, dtype):
    """acc float64 [batch, c, 2] of one dm3d_groupnorm_stats launch over x [batch, voxels, c] with per-thread sums of `dtype`."""
    B, V, c = x.shape
    slabs, slab, vox_par = stats_launch(V, c)
    xs = np.asarray(x, dtype)
    sq = (xs * xs).astype(dtype)                                  # float32: the rounded product; float64: exact for float32 inputs
    acc = np.zeros((B, c, 2), np.float64)
    for g in range(slabs):
        v0, v1 = g * slab, min(g * slab + slab, V)
        for vl in range(vox_par):
            if v0 + vl >= v1:
                break
            acc[..., 0] += np.cumsum(xs[:, v0 + vl:v1:vox_par], axis=1, dtype=dtype)[:, -1].astype(np.float64)
            acc[..., 1] += np.cumsum(sq[:, v0 + vl:v1:vox_par], axis=1, dtype=dtype)[:, -1].astype(np.float64)
    return acc


def stats_chain_cat(x, c1, dtype):
    """Two launches at chan_off 0 and c1 into one accumulator (one launch when c1 is the whole width)."""
    if c1 == x.shape[-1]:
        return stats_chain(x, dtype)
    return np.concatenate([stats_chain(x[..., :c1], dtype), stats_chain(x[..., c1:], dtype)], 1)


# ---- groupnorm_partials_kernel -----------------------------------------------------------------------------------------------------------
def slot_partials(x, order):
    """part [batch, slots, c, 2] of dm3d_groupnorm_partials: order "f32" as the kernel adds (float32 result), "f64" the float64 slot sums."""
    if order == "f64":
        return rk.groupnorm_partials(_t64(x)).numpy()
    B, V, c = x.shape
    slots = -(-V // 64)
    xp = np.zeros((B, slots * 64, c), np.float32)
    xp[:, :V] = x
    xp = xp.reshape(B, slots, 64, c)
    s, q = np.zeros((B, slots, c), np.float32), np.zeros((B, slots, c), np.float32)
    for v in range(64):                                           # the zero padding adds +0 and fma(0, 0, q) = q: the ragged slot is exact
        t = xp[:, :, v]
        s = (s + t).astype(np.float32)
        q = (t.astype(np.float64) * t.astype(np.float64) + q.astype(np.float64)).astype(np.float32)      # fmaf: the product is exact in float64
    return np.stack([s, q], -1)


def slot_partials_cat(x, c1, order):
    p1 = slot_partials(x[..., :c1], order)
    return p1, (slot_partials(x[..., c1:], order) if c1 < x.shape[-1] else None)


def group_scale_shift(acc, voxels, groups, gamma, beta, eps=EPS, dtype=np.float64):
    """groupnorm_finalize[2]: per-(sample, channel) sums [batch, c, 2] -> scale, shift [batch, c]; dtype float32 sums the channels (and, for
    partials, the slots) in float32 instead: the mutation a test must catch."""
    B, c, _ = acc.shape
    gc = c // groups
    tot = np.asarray(acc, dtype).reshape(B, groups, gc, 2).sum(2, dtype=dtype).astype(np.float64)
    n = float(voxels) * gc
    m = tot[..., 0] / n
    rstd = 1.0 / np.sqrt(np.maximum(tot[..., 1] / n - m * m, 0.0) + eps)
    sc = np.asarray(gamma, np.float64)[None] * np.repeat(rstd, gc, 1)
    return sc, np.asarray(beta, np.float64)[None] - np.repeat(m, gc, 1) * sc


def partials_to_acc(p1, p2):
    """float64 sum over the slots of one or two partial buffers -> [batch, c1 + c2, 2]."""
    parts = [np.asarray(p, np.float64).sum(1) for p in (p1, p2) if p is not None]
    return np.concatenate(parts, 1)


def gn_reference(x, groups, gamma, beta):
    return [t.numpy() for t in rk.groupnorm_scale_shift(_t64(x), groups, EPS, _t64(gamma), _t64(beta))]


def bn_reference(x, gamma, beta, moving, unbiased):
    """scale, shift, mean, rstd (+ moving mean, moving var) in float64."""
    mm, mv = (_t64(moving[0]), _t64(moving[1])) if moving is not None else (None, None)
    return [t.numpy() for t in rk.batchnorm_finalize(rk.moments_acc(_t64(x)), x.shape[1], EPS, _t64(gamma), _t64(beta), mm, mv, MOMENTUM, unbiased)]


def bn_from_acc(acc, voxels, gamma, beta, moving, unbiased):
    mm, mv = (_t64(moving[0]), _t64(moving[1])) if moving is not None else (None, None)
    return [t.numpy() for t in rk.batchnorm_finalize(_t64(acc), voxels, EPS, _t64(gamma), _t64(beta), mm, mv, MOMENTUM, unbiased)]


BN_OUTPUTS = ("scale", "shift", "mean", "rstd", "moving_mean", "moving_var")


def bn_model_error(shape, r, dtype):
    """Worst error over the six outputs (unbiased moving variance) of stats_chain(dtype) -> batchnorm_finalize against float64."""
    x, gamma, beta = stats_input(*shape, r)
    mov = moving_input(shape[2])
    ref = bn_reference(x, gamma, beta, mov, 1)
    got = bn_from_acc(stats_chain(x, dtype), shape[1], gamma, beta, mov, 1)
    return max(err(g, f) for g, f in zip(got, ref))


def gn_model_error(shape, r, kind, mode="mixed"):
    """Worst error of (scale, shift): kind "chain32" / "chain64" (stats -> finalize), "slot32" (partials -> finalize2) or "slot32_sum32"
    (the same with the slots and channels added in float32: what dm3d_groupnorm_finalize2 must not do)."""
    B, V, c1, c2, groups = shape
    x, gamma, beta = stats_input(B, V, c1 + c2, r, groups, mode)
    ref = gn_reference(x, groups, gamma, beta)
    if kind == "slot32":
        acc = partials_to_acc(*slot_partials_cat(x, c1, "f32"))
    elif kind == "slot32_sum32":
        p1, p2 = slot_partials_cat(x, c1, "f32")
        sums = np.concatenate([p.sum(1, dtype=np.float32) for p in (p1, p2) if p is not None], 1)
        return max(err(g, f) for g, f in zip(group_scale_shift(sums, V, groups, gamma, beta, dtype=np.float32), ref))
    else:
        acc = stats_chain_cat(x, c1, np.float32 if kind == "chain32" else np.float64)
    got = group_scale_shift(acc, V, groups, gamma, beta)
    return max(err(g, f) for g, f in zip(got, ref))


def slot_bar(x, c1, groups, gamma, beta):
    """(bar, model error) of partials -> finalize2 on this very input."""
    ref = gn_reference(x, groups, gamma, beta)
    got = group_scale_shift(partials_to_acc(*slot_partials_cat(x, c1, "f32")), x.shape[1], groups, gamma, beta)
    e = max(err(g, f) for g, f in zip(got, ref))
    return bar(LAYER_TOL, e), e


# ---- the row kernels -----------------------------------------------------------------------------------------------------------------------
def _wave_sum(s):
    """wave_sum: xor butterfly over 64 lanes in float32 (every lane ends with the same value)."""
    idx = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        s = (s + s[:, idx ^ o]).astype(np.float32)
    return s[:, 0]


def ln_stats(x, form="f4"):
    """(mean, rstd) float32 [rows] of the two-pass row kernels.  form "f4": layernorm3_kernel / layernorm_bwd_kernel (lane owns the float4s
    lane, lane + 64, ...); "h2": layernorm3_h2_kernel (lane owns the 8-channel groups lane and lane + 64)."""
    x = np.asarray(x, np.float32)
    rows, c = x.shape
    f32 = np.float32
    if form == "f4":
        xp = np.zeros((rows, 1024), f32)
        xp[:, :c] = x
        v = xp.reshape(rows, 4, 64, 4)                            # [row][j][lane][e]
        valid = (np.arange(256).reshape(4, 64) < c // 4)[None, :, :, None]
        s = np.zeros((rows, 64), f32)
        for j in range(4):
            s = (s + ((v[:, j, :, 0] + v[:, j, :, 1]) + (v[:, j, :, 2] + v[:, j, :, 3]))).astype(f32)
        mean = (_wave_sum(s) / f32(c)).astype(f32)
        d = (v - mean[:, None, None, None]).astype(f32)
        dd = np.where(valid, (d * d).astype(f32), f32(0))
        q = np.zeros((rows, 64), f32)
        for j in range(4):
            for e in range(4):
                q = (q + dd[:, j, :, e]).astype(f32)
    else:
        xp = np.zeros((rows, 1024), f32)
        xp[:, :c] = x
        v = xp.reshape(rows, 2, 64, 2, 4)                         # [row][j][lane][half][e]
        valid = (np.arange(128).reshape(2, 64) < c // 8)[None, :, :, None]
        s = np.zeros((rows, 64), f32)
        for j in range(2):
            for e in range(4):
                s = (s + (v[:, j, :, 0, e] + v[:, j, :, 1, e])).astype(f32)
        mean = (_wave_sum(s) / f32(c)).astype(f32)
        d = (v - mean[:, None, None, None, None]).astype(f32)
        dd = (d * d).astype(f32)
        pair = np.where(valid, (dd[:, :, :, 0, :] + dd[:, :, :, 1, :]).astype(f32), f32(0))
        q = np.zeros((rows, 64), f32)
        for j in range(2):
            for e in range(4):
                q = (q + pair[:, j, :, e]).astype(f32)
    var = ((_wave_sum(q) / f32(c)).astype(f32) + f32(EPS)).astype(f32)
    return mean, (1.0 / np.sqrt(var.astype(np.float64))).astype(f32)


def ln_stats_one_pass(x):
    """(mean, rstd) float32 from E[x^2] - m^2 with float32 sums: the form the row kernels avoid."""
    x = np.asarray(x, np.float32)
    c = np.float32(x.shape[1])
    m = (x.sum(1, dtype=np.float32) / c).astype(np.float32)
    ex2 = ((x * x).astype(np.float32).sum(1, dtype=np.float32) / c).astype(np.float32)
    var = np.maximum((ex2 - (m * m).astype(np.float32)).astype(np.float32), np.float32(0))
    return m, (1.0 / np.sqrt((var + np.float32(EPS)).astype(np.float64))).astype(np.float32)


def ln_forward_f32(x, mean, rstd, gamma, beta):
    """((x - mean) * rstd) * gamma + beta, every operation rounded to float32."""
    x = np.asarray(x, np.float32)
    xh = ((x - mean[:, None]).astype(np.float32) * rstd[:, None]).astype(np.float32)
    return ((xh * gamma[None]).astype(np.float32) + beta[None]).astype(np.float32)


def ln_bwd_f32(x, mean, rstd, gamma, dy):
    """dx, dgamma, dbeta of dm3d_layernorm_bwd from float32 row statistics: elementwise float32, the row means in float32, the sums over
    rows in float64 (their order is the kernel's own; the existing bar covers it)."""
    f32 = np.float32
    x, dy = np.asarray(x, f32), np.asarray(dy, f32)
    c = f32(x.shape[1])
    xh = ((x - mean[:, None]).astype(f32) * rstd[:, None]).astype(f32)
    dg = (dy * gamma[None]).astype(f32)
    s1 = (dg.sum(1, dtype=f32) / c).astype(f32)
    s2 = ((dg * xh).astype(f32).sum(1, dtype=f32) / c).astype(f32)
    dx = (rstd[:, None] * ((dg - s1[:, None]).astype(f32) - (xh * s2[:, None]).astype(f32)).astype(f32)).astype(f32)
    return dx, (dy * xh).astype(f32).astype(np.float64).sum(0), dy.astype(np.float64).sum(0)


def ln_reference(x, gamma, beta):
    return rk.layernorm(_t64(x), _t64(gamma), _t64(beta), EPS).numpy()


def ln_forward_model_error(rows, c, r, form, stats=ln_stats):
    x, _, params = row_input(rows, c, r)
    mean, rstd = stats(x, form) if stats is ln_stats else stats(x)
    return max(err(ln_forward_f32(x, mean, rstd, g, b), ln_reference(x, g, b)) for g, b in params)


def ln_bwd_reference(rows, c, r):
    x, dy, params = row_input(rows, c, r)
    return [t.numpy() for t in rk.layernorm_bwd(_t64(x), _t64(params[0][0]), _t64(dy), EPS)]


def ln_bwd_model_errors(rows, c, r, stats=ln_stats):
    """(dx, dgamma, dbeta) errors of the float32 model."""
    x, dy, params = row_input(rows, c, r)
    mean, rstd = stats(x, "f4") if stats is ln_stats else stats(x)
    got = ln_bwd_f32(x, mean, rstd, params[0][0], dy)
    return tuple(err(g, f) for g, f in zip(got, ln_bwd_reference(rows, c, r)))


# ---- dm3d_bn_act_bwd on the statistics of an offset tensor -----------------------------------------------------------------------------------
SILU = 2


@functools.lru_cache(maxsize=None)
def bn_bwd_input(r):
    """x [1, rows, c1 + c2] (per-channel offsets), g [rows, c], gamma, beta."""
    rows, c1, c2 = BN_BWD_SHAPE
    x, gamma, beta = stats_input(1, rows, c1 + c2, r)
    g = np.random.default_rng(_seed(rows, r, 17)).standard_normal((rows, c1 + c2)).astype(np.float32)
    g.setflags(write=False)
    return x, g, gamma, beta


def bn_bwd_reference(r):
    """dx, dgamma, dbeta, red in float64 from the float64 statistics of the input."""
    x, g, gamma, beta = bn_bwd_input(r)
    sc, sh, mean, rstd = (_t64(v) for v in bn_reference(x, gamma, beta, None, 1))
    return [t.numpy() for t in rk.bn_act_bwd(_t64(g), _t64(x[0]), sc, sh, mean, rstd, SILU)]


def bn_act_bwd_f32(r):
    """The same from the float64 statistics rounded once to float32 (the best dm3d_batchnorm_finalize can hand over), the elementwise part
    in float32 in the kernel's order, the sums over rows in float64."""
    f32 = np.float32
    x, g, gamma, beta = bn_bwd_input(r)
    sc, sh, mean, rstd = (v.astype(f32) for v in bn_reference(x, gamma, beta, None, 1))
    xv = x[0]
    u = (xv.astype(np.float64) * sc.astype(np.float64) + sh.astype(np.float64)).astype(f32)            # fmaf
    du = (g * rk.act_grad(torch.from_numpy(u), SILU).numpy().astype(f32)).astype(f32)
    xh = ((xv - mean[None]).astype(f32) * rstd[None]).astype(f32)
    s, sx = du.astype(np.float64).sum(0), (du * xh).astype(f32).astype(np.float64).sum(0)
    n = xv.shape[0]
    m1, m2 = (s / n).astype(f32), (sx / n).astype(f32)
    dx = (sc[None] * ((du - m1[None]).astype(f32) - (xh * m2[None]).astype(f32)).astype(f32)).astype(f32)
    return dx, sx, s, np.stack([s, sx], -1)


def bn_bwd_model_errors(r):
    """Errors of (dx, dgamma, dbeta, red) of the float32 model against float64."""
    return tuple(err(g, f) for g, f in zip(bn_act_bwd_f32(r), bn_bwd_reference(r)))


# ---- every model error the bars are built from ---------------------------------------------------------------------------------------------
def model_errors():
    """{"<entry>/<shape>/r<r>": error}: what tests/golden/norm_offset_model_errors.json records (python tests/norm_offset_cases.py writes it)."""
    out = {}
    for shape in BN_SHAPES:
        for r in R_VALUES:
            out[f"bn_chain64/{shape_id(shape)}/r{r}"] = bn_model_error(shape, r, np.float64)
            out[f"bn_chain32/{shape_id(shape)}/r{r}"] = bn_model_error(shape, r, np.float32)
    for shape in GN_SHAPES:
        for r, mode in GN_RUNS:
            tag = f"{shape_id(shape)}/r{r}" + ("" if mode == "mixed" else mode)
            for kind in ("chain64", "chain32", "slot32", "slot32_sum32"):
                out[f"gn_{kind}/{tag}"] = gn_model_error(shape, r, kind, mode)
    for rows, c in LN_SHAPES:
        for r in R_VALUES:
            tag = f"{rows}x{c}/r{r}"
            out[f"ln_two_pass_f4/{tag}"] = ln_forward_model_error(rows, c, r, "f4")
            out[f"ln_two_pass_h2/{tag}"] = ln_forward_model_error(rows, c, r, "h2")
            out[f"ln_one_pass/{tag}"] = ln_forward_model_error(rows, c, r, None, ln_stats_one_pass)
            for name, e in zip(("dx", "dgamma", "dbeta"), ln_bwd_model_errors(rows, c, r)):
                out[f"ln_bwd_{name}/{tag}"] = e
    for r in BN_BWD_R:
        for name, e in zip(("dx", "dgamma", "dbeta", "red"), bn_bwd_model_errors(r)):
            out[f"bn_act_bwd_{name}/{shape_id(BN_BWD_SHAPE)}/r{r}"] = e
    return out


def recorded_model_errors():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    errors = model_errors()
    with open(GOLDEN, "w") as f:
        json.dump({k: float(f"{v:.4e}") for k, v in errors.items()}, f, indent=0, sort_keys=True)
        f.write("\n")
    for k in sorted(errors):
        print(f"{k}: {errors[k]:.2e}")
