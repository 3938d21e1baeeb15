"""What the tests of the reconstruction metrics share (plain helper, no test in it): a numpy restatement of tf.image.ssim / tf.image.psnr
applied to a volume, the inputs, the cases and the bars.

The restatement is written from the formulas (include/dm3d.h, dm3d_metric_desc, states the same ones): x is the truth, y the
reconstruction, both [B, D, H, W, C]; every depth slice is an image of C channels.

  window   g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)), i = 0..10, normalised to sum 1; the 2-D window is g (x) g, VALID: (H-10) x (W-10) outputs
  SSIM     L = max_val, c1 = (0.01 L)^2, c2 = (0.03 L)^2;  mx = F(x), my = F(y), sxy = F(x y), sq = F(x^2 + y^2)
           lum = (2 mx my + c1) / (mx^2 + my^2 + c1);  cs = (2 sxy - 2 mx my + c2) / (sq - mx^2 - my^2 + c2)
           slice value = mean over outputs of lum cs, then mean over channels
  PSNR     mse = mean over H, W, C of (x - y)^2;  20 log10 L - 10 log10 mse
  max_val  None: max(y) - min(y) per volume, what the reference's test_step passes

order="f64" evaluates all of it in float64.  order="f32" does what the kernel documents: g rounded to float32, the products x*y and
x*x + y*y rounded to float32, F as the row pass then the column pass, each acc = fma(g[i], v[i], acc) from 0 in tap order i = 0..10
(the fma is emulated: a float32 product is exact in float64, and the one float64 addition is then rounded to float32), the formula
in float32 in TensorFlow's order, the per-pixel product lum*cs in float32; sums and means in float64, the result rounded to float32.
PSNR at "f32": mse rounded to float32, each of the two terms rounded to float32, one float32 subtraction.

The bars.  |order="f32" - order="f64"| of this restatement is the error float32 arithmetic makes on an input (its dominant term the
cancellation in sq - mx^2 - my^2 against c2); the worst of it over every input of tests/test_gpu_metrics.py is SSIM_F32_WORST (PSNR:
PSNR_F32_WORST, in dB), measured on the CPU, and the kernels get four times that: the factor is for FMA contraction and a different
but fixed summation order.  tests/test_metrics_host.py measures both figures again and holds the constants to them; an input whose
figure passed 1e-4 would be too flat for float32 and would have to be replaced."""
import numpy as np

TILE = 32                                 # DM3D_SSIM_TILE: the edge of the kernel's output tile
# (B, D, H, W): one window; one row of windows with a partial tile; partial tiles both ways; one tile exactly (TILE + 10) and one past
# it (TILE + 11) on each axis; full tiles at the workload's slice size
SHAPES = [(2, 3, 11, 11), (1, 2, 12, 43), (2, 2, 37, 50), (1, 1, 42, 42), (1, 1, 43, 42), (1, 1, 42, 43), (1, 1, 43, 43), (1, 2, 128, 128)]
# (cx, x0c, cy, y0c, nc): channel 0 of a 2-channel y against a 1-channel x; two channels of two; a window that starts past channel 0
CHANNELS = [(1, 0, 2, 0, 1), (2, 0, 2, 0, 2), (3, 1, 2, 1, 1)]
EXPLICIT_MAX_VAL = 1.0                    # the extra case per shape family: max_val given, not derived

SSIM_F32_WORST = 6.75e-6                  # worst |f32 - f64| of the restatement over those inputs (measured_worst() on the CPU)
PSNR_F32_WORST = 2.05e-6                  # the same for PSNR, in dB
SSIM_TOL = 4 * SSIM_F32_WORST
PSNR_TOL = 4 * PSNR_F32_WORST


def cases():
    """(shape, channels, max_val) of every parity case."""
    out = [(s, c, None) for s in SHAPES for c in CHANNELS[:2]]
    out += [(SHAPES[2], CHANNELS[2], None), (SHAPES[2], CHANNELS[0], EXPLICIT_MAX_VAL), (SHAPES[7], CHANNELS[1], EXPLICIT_MAX_VAL)]
    return out


def case_id(case):
    (b, d, h, w), (cx, x0c, cy, y0c, nc), mv = case
    return f"{b}x{d}x{h}x{w}-cx{cx}+{x0c}-cy{cy}+{y0c}-nc{nc}" + ("" if mv is None else f"-L{mv}")


def make_pair(shape, channels, seed=0):
    """x, y float32 [B, D, H, W, cx / cy]: x a smooth field plus noise in [0, 1], like a min-max-normalised MRI volume; the compared
    channels of y are x's plus small noise (SSIM well inside (0, 1)), the others unrelated (a mask-like field)."""
    b, d, h, w = shape
    cx, x0c, cy, y0c, nc = channels
    rng = np.random.default_rng(1000 * seed + 7 * h + w + cx + 3 * cy + 11 * y0c)
    zz, yy, xx = np.meshgrid(np.arange(d), np.arange(h), np.arange(w), indexing="ij")
    x = np.empty((b, d, h, w, cx), np.float64)
    for i in range(b):
        for c in range(cx):
            ph = rng.uniform(0, 2 * np.pi, 3)
            f = 0.5 + 0.2 * np.sin(2 * np.pi * yy / 17.0 + ph[0]) * np.cos(2 * np.pi * xx / 23.0 + ph[1]) + 0.15 * np.sin(0.7 * zz + ph[2])
            x[i, ..., c] = f + 0.08 * rng.standard_normal((d, h, w))
    x = np.clip(x, 0.0, 1.0).astype(np.float32)
    y = rng.uniform(0.0, 1.0, (b, d, h, w, cy)).astype(np.float32)
    y[..., y0c:y0c + nc] = x[..., x0c:x0c + nc] + (0.03 * rng.standard_normal((b, d, h, w, nc))).astype(np.float32)
    return x, y


def window():
    i = np.arange(11, dtype=np.float64)
    g = np.exp(-(i - 5.0) ** 2 / (2.0 * 1.5 ** 2))
    return g / g.sum()


def _fma32(a, b, c):
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _filter(v, axis, order):
    """The 11-tap VALID pass along `axis`, taps in index order."""
    g = window()
    n = v.shape[axis] - 10
    take = lambda k: np.take(v, np.arange(k, k + n), axis=axis)
    if order == "f64":
        acc = np.zeros(take(0).shape, np.float64)
        for k in range(11):
            acc = acc + g[k] * take(k)
        return acc
    g32 = g.astype(np.float32)
    acc = np.zeros(take(0).shape, np.float32)
    for k in range(11):
        acc = _fma32(np.broadcast_to(g32[k], acc.shape), take(k), acc)
    return acc


def _max_val(y, max_val, order):
    """[B] in the order's type: the given value, or max - min of y per volume (exact in float64; one float32 subtraction at "f32")."""
    b = y.shape[0]
    t = np.float64 if order == "f64" else np.float32
    if max_val is None:
        flat = y.reshape(b, -1)
        return flat.max(axis=1).astype(t) - flat.min(axis=1).astype(t)
    return np.broadcast_to(np.asarray(max_val, np.float32).astype(t), (b,)).copy()


def ssim(x, y, max_val=None, order="f64"):
    """[B, D] float64 (at "f32": float32 values) for x, y [B, D, H, W, C] of one shape."""
    assert order in ("f64", "f32") and x.shape == y.shape and x.ndim == 5 and x.shape[2] >= 11 and x.shape[3] >= 11
    t = np.float64 if order == "f64" else np.float32
    x, y = np.asarray(x).astype(t), np.asarray(y).astype(t)
    L = _max_val(y, max_val, order).reshape(-1, 1, 1, 1, 1)
    two = t(2.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        c1, c2 = (t(0.01) * L) ** 2, (t(0.03) * L) ** 2                       # one multiplication, then the square: one more
        F = lambda v: _filter(_filter(v, 3, order), 2, order)                  # the row pass (along W), then the column pass (along H)
        mx, my, sxy, sq = F(x), F(y), F(x * y), F(x * x + y * y)
        n0, d0 = (mx * my) * two, mx * mx + my * my
        lum = (n0 + c1) / (d0 + c1)
        cs = ((sxy * two - n0) + c2) / ((sq - d0) + c2)
        v = (lum * cs).astype(np.float64)
    out = v.mean(axis=(2, 3)).mean(axis=2)                                     # over the outputs, then over the channels
    return out if order == "f64" else out.astype(np.float32).astype(np.float64)


def sse(x, y):
    """[B, D] float64: the sum over H, W, C of (x - y)^2 (a float32 difference is exact in float64)."""
    e = np.asarray(x, np.float64) - np.asarray(y, np.float64)
    return (e * e).sum(axis=(2, 3, 4))


def psnr(x, y, max_val=None, order="f64"):
    """[B, D] float64 (at "f32": float32 values); +inf where a slice matches exactly."""
    assert order in ("f64", "f32") and x.shape == y.shape and x.ndim == 5
    L = _max_val(np.asarray(y), max_val, order).astype(np.float64).reshape(-1, 1)
    mse = sse(x, y) / float(x.shape[2] * x.shape[3] * x.shape[4])
    with np.errstate(divide="ignore"):
        if order == "f64":
            return 20.0 * np.log10(L) - 10.0 * np.log10(mse)
        mse = mse.astype(np.float32).astype(np.float64)
        return ((20.0 * np.log10(L)).astype(np.float32) - (10.0 * np.log10(mse)).astype(np.float32)).astype(np.float64)


def compared(x, y, channels):
    """The channel windows the kernel compares, as two arrays of one shape."""
    cx, x0c, cy, y0c, nc = channels
    return x[..., x0c:x0c + nc], y[..., y0c:y0c + nc]


def measured_worst():
    """(worst |f32 - f64| of ssim, of psnr in dB, {case id: (ssim figure, psnr figure)}) over every parity case."""
    per = {}
    for case in cases():
        shape, ch, mv = case
        xc, yc = compared(*make_pair(shape, ch), ch)
        es = float(np.abs(ssim(xc, yc, mv, "f32") - ssim(xc, yc, mv, "f64")).max())
        ep = float(np.abs(psnr(xc, yc, mv, "f32") - psnr(xc, yc, mv, "f64")).max())
        per[case_id(case)] = (es, ep)
    return max(v[0] for v in per.values()), max(v[1] for v in per.values()), per


if __name__ == "__main__":
    ws, wp, per = measured_worst()
    for k, (es, ep) in per.items():
        print(f"{k}: ssim {es:.3e}  psnr {ep:.3e} dB")
    print(f"worst: ssim {ws:.4e}  psnr {wp:.4e} dB")
