"""What the tests of the 3-D multi-scale SSIM share (plain helper, no test in it): a numpy restatement of the definition, the inputs, the
cases and the bar.  include/dm3d.h (dm3d_ms_ssim_desc) states the same formulas; this file is the authority.

x and y are [B, D, H, W, C]; volume b of x is compared with volume b of y, channel by channel (Wang, Simoncelli, Bovik 2003, in 3-D):

  window   g[i] = exp(-(i - (F-1)/2)^2 / (2 sigma^2)), i = 0..F-1, normalised to sum 1; the window is g (x) g (x) g, applied along W, then
           H, then D with no padding: (D-F+1) x (H-F+1) x (W-F+1) outputs
  scale j  L = max_val, c1 = (0.01 L)^2, c2 = (0.03 L)^2;  mx = F(x), my = F(y), sxy = F(x y), sq = F(x^2 + y^2)
           lum = (2 mx my + c1) / (mx^2 + my^2 + c1);  cs = (2 sxy - 2 mx my + c2) / (sq - mx^2 - my^2 + c2)
           CS_j = mean over outputs of cs;  S_j = mean over outputs of lum cs
  between  x and y become their 2 x 2 x 2 means; an odd edge drops its last plane; L stays
  result   mean over channels of prod_{j < M-1} max(CS_j, 0)^w_j * max(S_{M-1}, 0)^w_{M-1}, w = power_factors (float32 values), M = len(w)
  max_val  None: max(y) - min(y) per volume
  refused  min(D, H, W) >> (M - 1) < F: ValueError naming the largest M that fits

order="f64" evaluates all of it in float64.  order="f32" does what the kernels document: g rounded to float32, the pooled sum as
seven float32 additions in (dz, dy, dx) index order times 0.125, the products x*y and x*x + y*y rounded to float32, each filter pass
acc = fma(g[i], v[i], acc) from 0 in tap order (emulated as in metrics_reference.py), the formula in float32 in dm3d_ssim's order, lum*cs
in float32; sums, means, powers and the product in float64, the result rounded to float32.

The bar.  |order="f32" - order="f64"| is the error float32 arithmetic makes on an input; its worst over every input of
tests/test_gpu_msssim.py is MSSSIM_F32_WORST, measured on the CPU (tests/test_msssim_host.py measures it again and holds the
constant to it within 1 %), and the kernels get four times that, the project's rule for SSIM: the factor is for another, fixed
summation order."""
import numpy as np

from metrics_reference import _fma32, _max_val, compared, make_pair

TILE = (32, 16, 32)                       # DM3D_MSSSIM_TD / TH / TW: the kernel's tile of outputs along (D, H, W)
POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
# (cx, x0c, cy, y0c, nc), as metrics_reference.CHANNELS
CHANNELS = [(1, 0, 2, 0, 1), (2, 0, 2, 0, 2), (3, 1, 2, 1, 1)]
ONE = CHANNELS[0]
TD, TH, TW = TILE
# ((B, D, H, W), channels, filter_size, scales, max_val): max_val None, a number, or one number per volume.  A single scale runs with the
# power factor 1, more scales with the first ones of POWER_FACTORS.
CASES = [
    ((1, 12, 12, 12), ONE, 3, 3, None),                                       # 12 -> 6 -> 3
    ((1, 12, 12, 12), CHANNELS[1], 3, 3, None),
    ((1, 12, 12, 12), CHANNELS[2], 3, 3, 1.0),
    ((1, 13, 9, 22), ONE, 3, 2, None),                                        # odd and unequal edges: 13 x 9 x 22 -> 6 x 4 x 11
    ((2, 13, 9, 22), CHANNELS[1], 3, 2, (0.9, 1.3)),                          # two volumes, a max_val each
    ((1, 16, 16, 16), ONE, 7, 2, None),
    ((2, 16, 16, 16), CHANNELS[2], 7, 2, None),
    ((1, 22, 23, 44), ONE, 11, 2, None),
    ((1, 22, 23, 44), ONE, 11, 2, 1.0),                                       # explicit max_val against None
    # one tile exactly (edge + F - 1) and one point past it, on each axis
    ((1, TD + 2, 5, 6), ONE, 3, 1, None), ((1, TD + 3, 5, 6), ONE, 3, 1, None),
    ((1, 5, TH + 2, 6), ONE, 3, 1, None), ((1, 5, TH + 3, 6), ONE, 3, 1, None),
    ((1, 5, 6, TW + 2), ONE, 3, 1, None), ((1, 5, 6, TW + 3), ONE, 3, 1, None),
    # the same where the next scale's tile count changes too: 2 (TD + 2) + 1 -> TD + 2 along D, three tiles then one
    ((1, 2 * (TD + 2) + 1, 6, 7), ONE, 3, 2, None),
]

MSSSIM_F32_WORST = 8.88e-7                # worst |f32 - f64| of the restatement over CASES and extra_inputs() (measured_worst() on the CPU)
MSSSIM_TOL = 4 * MSSSIM_F32_WORST


def case_id(case):
    (b, d, h, w), (cx, x0c, cy, y0c, nc), f, m, mv = case
    tail = "" if mv is None else "-L" + ("x".join(str(v) for v in mv) if isinstance(mv, tuple) else str(mv))
    return f"{b}x{d}x{h}x{w}-cx{cx}+{x0c}-cy{cy}+{y0c}-nc{nc}-F{f}-M{m}{tail}"


def case_power(case):
    m = case[3]
    return (1.0,) if m == 1 else POWER_FACTORS[:m]


def case_max_val(case):
    mv = case[4]
    return np.asarray(mv, np.float32) if isinstance(mv, tuple) else mv


def window(filter_size=11, filter_sigma=1.5):
    i = np.arange(filter_size, dtype=np.float64)
    g = np.exp(-(i - 0.5 * (filter_size - 1)) ** 2 / (2.0 * float(np.float32(filter_sigma)) ** 2))
    return g / g.sum()


def max_scales(spatial, filter_size):
    n = 0
    while n < 5 and (min(spatial) >> n) >= filter_size:
        n += 1
    return n


def _filter(v, axis, g, order):
    """The VALID pass of the taps g along `axis`, taps in index order."""
    n = v.shape[axis] - (len(g) - 1)
    take = lambda k: np.take(v, np.arange(k, k + n), axis=axis)
    if order == "f64":
        acc = np.zeros(take(0).shape, np.float64)
        for k in range(len(g)):
            acc = acc + g[k] * take(k)
        return acc
    g32 = g.astype(np.float32)
    acc = np.zeros(take(0).shape, np.float32)
    for k in range(len(g)):
        acc = _fma32(np.broadcast_to(g32[k], acc.shape), take(k), acc)
    return acc


def pool(v):
    """[B, D, H, W, C] -> [B, D//2, H//2, W//2, C]: the mean of each 2 x 2 x 2 brick in v's dtype, the eight values added in (dz, dy, dx)
    index order; an odd edge drops its last plane, as avg_pool3d(kernel_size=2) does."""
    d2, h2, w2 = v.shape[1] // 2, v.shape[2] // 2, v.shape[3] // 2
    acc = None
    for dz in range(2):
        for dy in range(2):
            for dx in range(2):
                t = v[:, dz:2 * d2:2, dy:2 * h2:2, dx:2 * w2:2, :]
                acc = t.copy() if acc is None else acc + t
    return acc * v.dtype.type(0.125)


def scale_terms(x, y, L, g, order):
    """(CS, S) float64 [B, C] of one scale: the means over the valid map of cs and of lum*cs."""
    t = x.dtype.type
    two = t(2.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        c1, c2 = (t(0.01) * L) ** 2, (t(0.03) * L) ** 2
        F = lambda v: _filter(_filter(_filter(v, 3, g, order), 2, g, order), 1, g, order)      # along W, then H, then D
        mx, my, sxy, sq = F(x), F(y), F(x * y), F(x * x + y * y)
        n0, d0 = (mx * my) * two, mx * mx + my * my
        lum = (n0 + c1) / (d0 + c1)
        cs = ((sxy * two - n0) + c2) / ((sq - d0) + c2)
        return cs.astype(np.float64).mean(axis=(1, 2, 3)), (lum * cs).astype(np.float64).mean(axis=(1, 2, 3))


def ms_ssim(x, y, max_val=None, power_factors=POWER_FACTORS, filter_size=11, filter_sigma=1.5, order="f64", terms=False):
    """[B] float64 (at "f32": float32 values) for x, y [B, D, H, W, C] of one shape.  terms=True: also the list over scales of
    (CS_j, S_j) [B, C]."""
    assert order in ("f64", "f32") and x.shape == y.shape and x.ndim == 5
    assert filter_size % 2 == 1 and 3 <= filter_size <= 11 and 1 <= len(power_factors) <= 5 and all(w > 0 for w in power_factors)
    m, fit = len(power_factors), max_scales(x.shape[1:4], filter_size)
    if m > fit:
        raise ValueError(f"{m} scales of a {x.shape[1]} x {x.shape[2]} x {x.shape[3]} volume leave an edge smaller than filter_size={filter_size}; "
                         f"at most {fit} scales fit")
    t = np.float64 if order == "f64" else np.float32
    x, y = np.asarray(x).astype(t), np.asarray(y).astype(t)
    L = _max_val(y, max_val, order).reshape(-1, 1, 1, 1, 1)
    g = window(filter_size, filter_sigma)
    w = np.asarray(power_factors, np.float32).astype(np.float64)
    per, prod = [], 1.0
    for j in range(m):
        if j:
            x, y = pool(x), pool(y)
        cs, s = scale_terms(x, y, L, g, order)
        per.append((cs, s))
        prod = prod * np.maximum(s if j == m - 1 else cs, 0.0) ** w[j]
    out = prod.mean(axis=1)
    out = out if order == "f64" else out.astype(np.float32).astype(np.float64)
    return (out, per) if terms else out


def case_pair(case):
    """The compared channel windows of the case's inputs, as two arrays of one shape."""
    shape, ch = case[0], case[1]
    return compared(*make_pair(shape, ch), ch)


_REFERENCE = {}


def reference(case):
    """(float64 result [B], per-scale terms) of a case, computed once."""
    key = case_id(case)
    if key not in _REFERENCE:
        xc, yc = case_pair(case)
        out, per = ms_ssim(xc, yc, case_max_val(case), case_power(case), case[2], order="f64", terms=True)
        out.setflags(write=False)
        _REFERENCE[key] = (out, per)
    return _REFERENCE[key]


# ---- the inputs of the pair-table tests: volumes that are all correlated with one another ------------------------------------------
PAIR_TABLE = dict(channels=CHANNELS[2], filter_size=3, power=POWER_FACTORS[:2], x_index=[2, 0, 1, 0], y_index=[0, 1, 1, 0],
                  max_val=np.array([1.0, 0.8, 1.2, 0.9], np.float32))
BATCH = dict(filter_size=3, power=POWER_FACTORS[:3], max_val=1.1)


def pair_table_inputs():
    """x [3, 13, 9, 22, 3] and y [2, 13, 9, 22, 2]: one field plus a small noise per volume in the compared channels."""
    cx, x0c, cy, y0c, _ = PAIR_TABLE["channels"]
    base, _ = make_pair((1, 13, 9, 22), PAIR_TABLE["channels"], seed=1)
    rng = np.random.default_rng(5)
    x = (base + 0.03 * rng.standard_normal((3, 13, 9, 22, cx))).astype(np.float32)
    y = rng.uniform(0.0, 1.0, (2, 13, 9, 22, cy)).astype(np.float32)
    y[..., y0c] = base[..., x0c] + (0.03 * rng.standard_normal((2, 13, 9, 22))).astype(np.float32)
    return x, y


def pair_table_rows():
    """The compared channel windows of the rows PAIR_TABLE selects, as two arrays of one shape."""
    xc, yc = compared(*pair_table_inputs(), PAIR_TABLE["channels"])
    return xc[PAIR_TABLE["x_index"]], yc[PAIR_TABLE["y_index"]]


def batch_volumes(n=4):
    """n volumes [n, 12, 12, 12, 1] for pairwise_ms_ssim: one field plus a small noise each."""
    base, _ = make_pair((1, 12, 12, 12), (1, 0, 1, 0, 1), seed=2)
    rng = np.random.default_rng(11)
    return (base + 0.03 * rng.standard_normal((n, 12, 12, 12, 1))).astype(np.float32)


def batch_rows(n=4):
    """The pairs i < j of batch_volumes(n) in lexicographic order, as two arrays of one shape."""
    v = batch_volumes(n)
    order = [(i, j) for i in range(n) for j in range(i + 1, n)]
    return v[[i for i, _ in order]], v[[j for _, j in order]]


def extra_inputs():
    """{name: (x rows, y rows, max_val, power, filter_size)} of the GPU tests' inputs that are not in CASES."""
    t, b = PAIR_TABLE, BATCH
    return {"pair-table": pair_table_rows() + (t["max_val"], t["power"], t["filter_size"]),
            "batch": batch_rows() + (b["max_val"], b["power"], b["filter_size"])}


def measured_worst():
    """(worst |f32 - f64| over CASES and extra_inputs(), {id: figure})."""
    per = {}
    for case in CASES:
        xc, yc = case_pair(case)
        f32 = ms_ssim(xc, yc, case_max_val(case), case_power(case), case[2], order="f32")
        per[case_id(case)] = float(np.abs(f32 - reference(case)[0]).max())
    for name, (xr, yr, mv, power, f) in extra_inputs().items():
        per[name] = float(np.abs(ms_ssim(xr, yr, mv, power, f, order="f32") - ms_ssim(xr, yr, mv, power, f)).max())
    return max(per.values()), per


if __name__ == "__main__":
    worst, per = measured_worst()
    for k, e in per.items():
        print(f"{k}: {e:.3e}")
    print(f"worst: {worst:.4e}")
