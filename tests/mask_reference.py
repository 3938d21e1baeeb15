"""The authority of the mask-channel scores (plain helper, no test in it; tests/test_mask_host.py checks it on the CPU against closed forms
and scipy, tests/test_gpu_mask.py holds the kernels to it): MONAI's definitions restated in numpy, int64 and float64.  It imports nothing
from the package.

    mask        value > threshold (NaN is background), per volume and channel of a channel window (first, count)
    counts      |X|, |Y|, |X and Y|;  Dice = 2 |X and Y| / (|X| + |Y|),  IoU = |X and Y| / |X or Y|,  both NaN where X is empty
    surface     mask XOR erosion by the 6-neighbour cross with a zero border
    map         at every voxel the smallest dz^2 + dy^2 + dx^2 to a surface voxel, by brute force over the surface voxel set; INT32_MAX
                everywhere when the set is empty
    directed    X -> Y: the map of Y's surface at X's surface voxels
    HD = the larger directed maximum, HD_p = the larger directed np.percentile(.., method="linear"), ASSD = the mean of both directed
    sets together; NaN if either surface is empty.  Distances are sqrt of the integers, sums by math.fsum (one rounding).

The bar of the GPU tests on hd, hd_percentile and assd is relative: (n + 4) * 2^-52 with n the surface voxels summed (both directions);
both sides start from the same integers, each sqrt and each add contributes at most one rounding of 2^-53 relative, and all terms are
non-negative.  Counts, surfaces and maps are compared for equality."""
import functools
import math

import numpy as np

INT32_MAX = 2 ** 31 - 1
THRESHOLD = 0.5
CX, X0C, CY, Y0C, NC = 3, 1, 2, 0, 2            # x [B, D, H, W, 3] read through the window (1, 2), y [B, D, H, W, 2] through (0, 2)
BATCH = 2
PERCENTILES = (95.0, 50.0)

# (d, h, w): degenerate axes twice; odd extents; one past a wave and past power-of-two tiles on every axis; a column longer than 128 on
# h and on d.  The kernel stages 32 neighbouring columns a block, whatever their length, and walks 1024 voxels a block in its streaming
# passes: (17, 33, 65) is one past 32 on h, past 64 on w and 36 blocks of voxels; no further tile length exists.
SHAPES = ((1, 1, 1), (1, 9, 1), (5, 7, 9), (17, 33, 65), (3, 130, 6), (130, 3, 5))
# the mask kinds of (x, y) at position (b, c) = divmod(index, 2) of a case
GROUPS = {"shapes": (("balls", "balls2"), ("speckle", "speckle2"), ("blob", "balls"), ("full", "balls2")),
          "edges": (("single", "single2"), ("empty", "balls"), ("balls2", "empty"), ("empty", "empty"))}
CASES = tuple((s, g) for s in SHAPES for g in GROUPS)


def case_id(case):
    return "x".join(map(str, case[0])) + "-" + case[1]


# ---- the definitions -----------------------------------------------------------------------------------------------------------------
def masks(t, first, count, threshold=THRESHOLD):
    """[B, D, H, W, C] values -> bool [B, count, D, H, W]: the binarised channel window."""
    with np.errstate(invalid="ignore"):
        m = np.asarray(t)[..., first:first + count] > np.float32(threshold)
    return np.ascontiguousarray(np.moveaxis(m, -1, 1))


def erode(m):
    """One volume [D, H, W]: erosion by the 6-neighbour cross, everything outside the volume background."""
    p = np.pad(m, 1, constant_values=False)
    c = p[1:-1, 1:-1, 1:-1]
    return c & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:]


def surface(m):
    return m ^ erode(m)


def sq_distance_map(feat, chunk=1 << 22):
    """One volume of features [D, H, W] bool -> int64 [D, H, W]: brute force over the feature voxel set, in chunks of voxels.  The
    squared distance is one dot product of integers, [z, y, x, |v|^2, 1] . [-2 sz, -2 sy, -2 sx, 1, |s|^2]: every product and partial
    sum is an integer far below 2^53, so float64 carries it exactly."""
    s = np.argwhere(feat).astype(np.float64)
    out = np.full(feat.shape, INT32_MAX, np.int64)
    if not len(s):
        return out
    v = np.argwhere(np.ones(feat.shape, bool)).astype(np.float64)
    va = np.concatenate([v, (v * v).sum(1, keepdims=True), np.ones((len(v), 1))], 1)
    sa = np.concatenate([-2 * s, np.ones((len(s), 1)), (s * s).sum(1, keepdims=True)], 1).T.copy()
    flat = out.reshape(-1)
    step = max(1, chunk // len(s))
    for i in range(0, len(v), step):
        flat[i:i + step] = (va[i:i + step] @ sa).min(axis=1).astype(np.int64)
    return out


def overlap_counts(mx, my):
    """bool [B, nc, D, H, W] twice -> int64 [B, nc, 3]: |X|, |Y|, |X and Y|."""
    ax = (2, 3, 4)
    return np.stack([mx.sum(ax), my.sum(ax), (mx & my).sum(ax)], -1).astype(np.int64)


def dice_iou(counts):
    """int64 [..., 3] -> float64 Dice and IoU, NaN where the truth is empty."""
    x, y, b = (counts[..., k].astype(np.float64) for k in range(3))
    with np.errstate(invalid="ignore", divide="ignore"):
        dice = np.where(x > 0, 2 * b / (x + y), np.nan)
        iou = np.where(x > 0, b / (x + y - b), np.nan)
    return dice, iou


def directed(surf_from, map_to):
    """The sorted squared distances (int64) of one direction."""
    return np.sort(map_to[surf_from])


def interpolation_ranks(n, percentile):
    """(lo, hi, t) of numpy's linear rule on n sorted values."""
    r = (n - 1) * (percentile / 100.0)
    lo = int(math.floor(r))
    return lo, min(lo + 1, n - 1), r - lo


def surface_stats(mx, my, percentile=95.0, maps=None):
    """One volume's masks [D, H, W] -> dict(hd, hd_percentile, assd, surface_x, surface_y, n, split): float64 by the definitions; n the
    voxels summed (``maps``: the squared maps of the two surfaces where the caller has them); split: whether a direction's two
    interpolation ranks fall on different squared distances with 0 < t < 1."""
    sx, sy = surface(mx), surface(my)
    nx, ny = int(sx.sum()), int(sy.sum())
    out = dict(surface_x=float(nx), surface_y=float(ny), n=nx + ny, split=False, hd=math.nan, hd_percentile=math.nan, assd=math.nan)
    if not nx or not ny:
        return out
    map_x, map_y = maps if maps is not None else (sq_distance_map(sx), sq_distance_map(sy))
    dxy, dyx = directed(sx, map_y), directed(sy, map_x)
    fx, fy = np.sqrt(dxy.astype(np.float64)), np.sqrt(dyx.astype(np.float64))
    out["hd"] = float(max(fx[-1], fy[-1]))
    out["hd_percentile"] = float(max(np.percentile(fx, percentile, method="linear"), np.percentile(fy, percentile, method="linear")))
    out["assd"] = math.fsum(fx.tolist() + fy.tolist()) / (nx + ny)
    for dsq in (dxy, dyx):
        lo, hi, t = interpolation_ranks(len(dsq), percentile)
        out["split"] |= bool(dsq[lo] != dsq[hi] and 0.0 < t < 1.0)
    return out


def bound(n):
    """The relative bar on hd, hd_percentile and assd of a (volume, channel) whose surfaces hold n voxels together."""
    return (n + 4) * 2.0 ** -52


def within(got, ref, n):
    """Whether got meets ref: both NaN, or |got - ref| <= bound(n) |ref|."""
    if math.isnan(ref):
        return math.isnan(got)
    return abs(got - ref) <= bound(n) * abs(ref)


# ---- the inputs ----------------------------------------------------------------------------------------------------------------------
def _ellipsoids(shape, rng, count):
    z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
    m = np.zeros(shape, bool)
    for _ in range(count):
        c = [rng.uniform(0, n - 1) for n in shape]
        r = [max(0.8, rng.uniform(0.15, 0.3) * n) for n in shape]
        m |= ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 <= 1.0
        m[tuple(int(round(v)) for v in c)] = True
    return m


def mask_of(kind, shape, seed=0):
    """bool [D, H, W], fixed seeds."""
    rng = np.random.default_rng([seed, sum(map(ord, kind))] + list(shape))
    if kind in ("balls", "balls2"):
        return _ellipsoids(shape, rng, 3)
    if kind in ("speckle", "speckle2"):
        return rng.random(shape) < 0.5
    if kind == "blob":                                                          # an ellipsoid about the corner voxel: touches three faces
        z, y, x = np.meshgrid(*(np.arange(n, dtype=np.float64) for n in shape), indexing="ij")
        r = [max(1.0, 0.6 * n) for n in shape]
        return (z / r[0]) ** 2 + (y / r[1]) ** 2 + (x / r[2]) ** 2 <= 1.0
    if kind == "full":
        return np.ones(shape, bool)
    if kind in ("single", "single2"):
        m = np.zeros(shape, bool)
        m[tuple(int(rng.integers(0, n)) for n in shape)] = True
        return m
    assert kind == "empty", kind
    return np.zeros(shape, bool)


def values_of(m, rng):
    """float32 values whose binarisation at THRESHOLD is m: the mask in (0.5, 1], the background in [0, 0.5] with exact 0.5 and NaN in it."""
    u = rng.random(m.shape)
    v = np.where(m, 0.5 + 0.5 * (1.0 - u) + 1e-3, 0.5 * u).astype(np.float32)
    bg = np.flatnonzero(~m.reshape(-1))
    flat = v.reshape(-1)
    flat[bg[::7]] = 0.5                                                         # not above the threshold
    flat[bg[3::11]] = np.nan                                                    # background
    return v


@functools.lru_cache(maxsize=None)
def make_case(case):
    """(x [B, D, H, W, CX], y [B, D, H, W, CY]) float32; the channels outside x's window hold values on both sides of the threshold."""
    shape, group = case
    rng = np.random.default_rng([7] + list(shape) + [len(group)])
    x = rng.random((BATCH,) + shape + (CX,)).astype(np.float32)
    y = rng.random((BATCH,) + shape + (CY,)).astype(np.float32)
    for i, (kx, ky) in enumerate(GROUPS[group]):
        b, c = divmod(i, NC)
        x[b, ..., X0C + c] = values_of(mask_of(kx, shape), rng)
        y[b, ..., Y0C + c] = values_of(mask_of(ky, shape, seed=1), rng)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


@functools.lru_cache(maxsize=None)
def reference(case):
    """dict: mx, my (bool [B, nc, D, H, W]), counts (int64 [B, nc, 3]), surf_x, surf_y (bool), map_x, map_y (int64: the squared maps of
    the two surfaces), stats {percentile: [B][nc] dicts of surface_stats}."""
    x, y = make_case(case)
    mx, my = masks(x, X0C, NC), masks(y, Y0C, NC)
    kinds = GROUPS[case[1]]
    for i, (kx, ky) in enumerate(kinds):
        b, c = divmod(i, NC)
        assert np.array_equal(mx[b, c], mask_of(kx, case[0])) and np.array_equal(my[b, c], mask_of(ky, case[0], seed=1))
    sx = np.stack([np.stack([surface(mx[b, c]) for c in range(NC)]) for b in range(BATCH)])
    sy = np.stack([np.stack([surface(my[b, c]) for c in range(NC)]) for b in range(BATCH)])
    map_x = np.stack([np.stack([sq_distance_map(sx[b, c]) for c in range(NC)]) for b in range(BATCH)])
    map_y = np.stack([np.stack([sq_distance_map(sy[b, c]) for c in range(NC)]) for b in range(BATCH)])
    stats = {p: [[surface_stats(mx[b, c], my[b, c], p, (map_x[b, c], map_y[b, c])) for c in range(NC)] for b in range(BATCH)] for p in PERCENTILES}
    return dict(mx=mx, my=my, counts=overlap_counts(mx, my), surf_x=sx, surf_y=sy, map_x=map_x, map_y=map_y, stats=stats)
