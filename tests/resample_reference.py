"""numpy restatement, in float64, of the volume preprocessing entries (include/dm3d.h, "Volume preprocessing"; plain helper, no test in
it, nothing imported from the package): the cubic B-spline prefilter of scipy.ndimage.spline_filter(order=3, mode="mirror"), the
coordinate rule and the three interpolation orders of scipy.ndimage.affine_transform(mode="constant") with mirrored taps, dipy's reslice
rule, the reference's transform_image, normalisation and augmentation, and the host side of the augmentation's Philox draw.
tests/test_resample_host.py holds it to scipy and to closed forms; tests/test_gpu_resample.py compares the kernels with it.

Every operation is written in the order the kernels use (elementwise numpy float64 operations are IEEE, as the device's are, and the
library builds without contraction), so inside / outside and floor decisions agree with the device bit for bit.

The bar on interpolated values.  The kernels keep coordinates, weights, coefficients and sums in float64 and round once, at the float32
store.  So the float32 evaluation of the restatement is its float64 value rounded to float32, RESAMPLE_F32_WORST is the worst
|f32 - f64| of that over every interpolating case of the GPU tests (the host test holds the constant to what it measures), and the bar
is four times that.  transform_image chains three resamples with a float32 store after each; the values of each of its stages, before
their store, are in the measured set, and its end-to-end comparison has the same bar."""
import numpy as np

POLE = np.sqrt(3.0) - 2.0
GAIN = (1.0 - POLE) * (1.0 - 1.0 / POLE)
SPLINE_TILE = 32                          # DM3D_SPLINE_LANES: lines a workgroup stages side by side
STREAM_AUGMENT = 0xA063

RESAMPLE_F32_WORST = 5.94e-08             # worst |f32 - f64| over interpolating_values() (tests/test_resample_host.py measures 5.9374e-08)
RESAMPLE_TOL = 4 * RESAMPLE_F32_WORST
AUGMENT_TOL = 2.0 ** -24                  # a float64 value in [0, 1] rounded once (2^-25) and the same again for the mean's summation order


# ---- prefilter -------------------------------------------------------------------------------------------------------------------------
def _power(n):
    p = 1.0
    for _ in range(n - 1):
        p *= POLE
    return p


def spline_filter1d(c, axis):
    """One axis of the prefilter on float64 data; a line of length 1 is returned as it is."""
    c = np.moveaxis(np.array(c, np.float64), axis, 0).copy()
    n = c.shape[0]
    if n > 1:
        c *= GAIN
        zn1 = _power(n)
        c0, zi = c[0] + zn1 * c[n - 1], POLE
        for i in range(1, n - 1):
            c0 = c0 + zi * (c[i] + zn1 * c[n - 1 - i])
            zi *= POLE
        c[0] = c0 / (1.0 - zn1 * zn1)
        for i in range(1, n):
            c[i] = c[i] + POLE * c[i - 1]
        c[n - 1] = (POLE * c[n - 2] + c[n - 1]) * POLE / (POLE * POLE - 1.0)
        for i in range(n - 2, -1, -1):
            c[i] = POLE * (c[i + 1] - c[i])
    return np.moveaxis(c, 0, axis)


def spline_filter(x):
    """The last three axes of x (float32 or float64) filtered along w, then h, then d: float64 coefficients."""
    c = np.asarray(x, np.float64)
    for axis in (-1, -2, -3):
        c = spline_filter1d(c, axis)
    return c


# ---- coordinates and interpolation -----------------------------------------------------------------------------------------------------
def coordinates(matrix, offset, output_shape):
    """[3, od, oh, ow] float64: ((o0 M[h][0] + o1 M[h][1]) + o2 M[h][2]) + offset[h]."""
    m, off = np.asarray(matrix, np.float64), np.broadcast_to(np.asarray(offset, np.float64), (3,))
    if m.shape == (3,):
        m = np.diag(m)
    oz, oy, ox = np.meshgrid(*(np.arange(s, dtype=np.float64) for s in output_shape), indexing="ij")
    return np.stack([((oz * m[h, 0] + oy * m[h, 1]) + ox * m[h, 2]) + off[h] for h in range(3)])


def inside_mask(coords, shape):
    ok = np.ones(coords.shape[1:], bool)
    for h in range(3):
        ok &= (coords[h] >= 0.0) & (coords[h] <= float(shape[h] - 1))
    return ok


def mirror(i, n):
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.mod(i, period)
    return np.where(i < n, i, period - i)


def _taps(c, n, order):
    """Indices [N, order + 1] and weights [N, order + 1] of one axis for inside coordinates c [N]."""
    if order == 0:
        return np.floor(c + 0.5).astype(np.int64)[:, None], np.ones((c.size, 1))
    fl = np.floor(c)
    x = c - fl
    start = fl.astype(np.int64) - order // 2
    idx = mirror(start[:, None] + np.arange(order + 1)[None, :], n)
    if order == 1:
        w0 = 1.0 - x
        return idx, np.stack([w0, 1.0 - w0], 1)
    y = 1.0 - x
    w1 = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0
    w2 = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0
    w0 = y * y * y / 6.0
    return idx, np.stack([w0, w1, w2, ((1.0 - w0) - w1) - w2], 1)


def interpolate(src, coords, order, cval=0.0):
    """float64 [od, oh, ow]: src (data at orders 0 and 1, coefficients at order 3) at coords; cval (as float32) outside."""
    src = np.asarray(src, np.float64)
    ok = inside_mask(coords, src.shape)
    out = np.full(ok.shape, float(np.float32(cval)))
    c = [coords[h][ok] for h in range(3)]
    (iz, wz), (iy, wy), (ix, wx) = (_taps(c[h], src.shape[h], order) for h in range(3))
    t = np.zeros(c[0].size)
    for i in range(order + 1):
        for j in range(order + 1):
            for k in range(order + 1):
                t = t + ((src[iz[:, i], iy[:, j], ix[:, k]] * wz[:, i]) * wy[:, j]) * wx[:, k]
    out[ok] = t
    return out


def affine_transform(x, matrix, offset=0.0, output_shape=None, order=3, cval=0.0, prefilter=True):
    """One volume x [d, h, w] -> float64 [od, oh, ow]; matrix a 3-vector, [3, 3] or [4, 4] homogeneous."""
    m = np.asarray(matrix, np.float64)
    if m.shape == (4, 4):
        m, offset = m[:3, :3], m[:3, 3]
    shape = tuple(x.shape) if output_shape is None else tuple(output_shape)
    src = spline_filter(x) if order == 3 and prefilter else np.asarray(x, np.float64)
    return interpolate(src, coordinates(m, offset, shape), order, cval)


def f32(v):
    """The device's store: float64 rounded once to float32."""
    return np.asarray(v, np.float64).astype(np.float32)


def f32_gap(v):
    v = np.asarray(v, np.float64)
    return float(np.abs(f32(v).astype(np.float64) - v).max())


# ---- the reference's pipeline ----------------------------------------------------------------------------------------------------------
def reslice(x, affine, zooms, new_zooms, order=1, cval=0.0):
    """dipy's rule; returns (float64 volume, affine2)."""
    zooms, new_zooms = np.asarray(zooms, np.float64), np.asarray(new_zooms, np.float64)
    R = new_zooms / zooms
    new_shape = tuple(int(s) for s in np.round(zooms / new_zooms * np.array(x.shape, np.float64)).astype(np.int64))
    Rx = np.eye(4)
    Rx[:3, :3] = np.diag(R)
    return affine_transform(x, R, 0.0, new_shape, order, cval), np.asarray(affine, np.float64) @ Rx


def transform_image(x, affine, voxsize, scale=2, init_shape=(256, 256, 256), between=f32, stages=None):
    """The reference's transform_image; `between` is applied to the volume after each resample (the device stores float32); a list
    given as `stages` receives the float64 values of the three resamples before their store."""
    image2, affine2 = reslice(x, affine, voxsize, (1.0, 1.0, 1.0))
    image2_f64, image2 = image2, between(image2)
    affine2 = affine2.copy()
    affine2[:3, 3] += np.array([s // 2 for s in init_shape], np.float64)
    centred_f64 = affine_transform(image2, np.linalg.inv(affine2), output_shape=tuple(init_shape), order=3)
    centred = between(centred_f64)
    out, _ = reslice(centred, np.eye(4), (1.0, 1.0, 1.0), (float(scale),) * 3)
    if stages is not None:
        stages += [image2_f64, centred_f64, out]
    return out, affine2


def normalize(x):
    """(folded float32 min, max, float64 normalised volume) of one float32 volume."""
    a = np.abs(np.asarray(x, np.float32))
    mn, mx = a.min(), a.max()
    return mn, mx, (a.astype(np.float64) - float(mn)) / (float(mx) - float(mn))


def augment(image, mask, flip, brightness, contrast):
    """One sample [d, h, w, c] float32 with float32 factors: float64 image, mask flipped alike."""
    t = np.clip(np.asarray(image, np.float64) * float(np.float32(brightness)), 0.0, 1.0)
    mean = t.sum() / t.size
    out = np.clip((1.0 + float(np.float32(contrast))) * (t - mean) + mean, 0.0, 1.0)
    if flip:
        out, mask = out[::-1], (None if mask is None else mask[::-1])
    return out, mask


def augment_draw(seed, batch, flip_chance=0.6, brightness_range=(0.9, 1.1), contrast_range=(0.9, 1.1)):
    """The host side of dm3d_augment's draw, from oracle/ref_philox.py's Philox4x32-10 (tests/test_philox_host.py holds that to the
    known-answer vectors): counter (i, 0, 0, STREAM_AUGMENT), key seed; u_k = float32(word_k) * 2^-32; float32 arithmetic throughout.
    Returns (flip int32 [B], brightness float32 [B], contrast float32 [B])."""
    from oracle import ref_philox as rp
    seed = int(seed) & (2 ** 64 - 1)
    words = rp.philox4x32_10(np.arange(batch, dtype=np.uint64), 0, 0, STREAM_AUGMENT, seed & rp.MASK32, seed >> 32)
    u = [w.astype(np.float32) * rp.TWO_M32_F32 for w in words[:3]]
    lo_b, hi_b, lo_c, hi_c = (np.float32(v) for v in (*brightness_range, *contrast_range))
    flip = np.where(u[0] < np.float32(flip_chance), 0, 1).astype(np.int32)
    return flip, lo_b + (hi_b - lo_b) * u[1], lo_c + (hi_c - lo_c) * u[2]


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
IN_SHAPE, OUT_SHAPE = (9, 12, 7), (10, 6, 13)
CVALS = (0.0, -0.375)
SEED = 20261021


def _rotation(ax, ay, az):
    cx, sx, cy, sy, cz, sz = np.cos(ax), np.sin(ax), np.cos(ay), np.sin(ay), np.cos(az), np.sin(az)
    return (np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]]) @
            np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]))


def generic_matrices(batch=3):
    """[batch, 3, 3] and [batch, 3]: rotation, shear and non-unit scale about the volume centres with a fractional offset, a different
    one per volume; tests/test_resample_host.py checks that 20 % to 80 % of the outputs fall outside and that no coordinate lies within
    1e-6 of an integer."""
    mats, offs = [], []
    c_in, c_out = (np.array(IN_SHAPE) - 1) / 2.0, (np.array(OUT_SHAPE) - 1) / 2.0
    for b in range(batch):
        rot = _rotation(0.21 + 0.13 * b, -0.17 + 0.11 * b, 0.29 - 0.19 * b)
        shear = np.array([[1.0, 0.11 + 0.03 * b, -0.07], [0.0, 1.0, 0.13 - 0.05 * b], [0.0, 0.0, 1.0]])
        scale = np.array(IN_SHAPE) / np.array(OUT_SHAPE) * (1.27 + 0.09 * b)
        m = rot @ shear @ np.diag(scale)
        mats.append(m)
        offs.append(c_in - m @ c_out + np.array([0.3137, -0.4213, 0.1871]) * (b + 1))
    return np.array(mats), np.array(offs)


def volumes(shape, batch, seed=SEED):
    """float32 [batch, *shape] in [0, 1]."""
    return np.random.default_rng(seed).random((batch,) + tuple(shape), dtype=np.float32)


def exact_cases():
    """(name, input shape, matrix 3-vector, offset, output shape): every coordinate is an integer or a half, some exactly 0 and n - 1,
    and the last outputs of the diag(0.5) and shift cases fall outside."""
    return [("identity", (5, 6, 7), (1.0, 1.0, 1.0), (0.0, 0.0, 0.0), (5, 6, 7)),
            ("shift", (5, 6, 7), (1.0, 1.0, 1.0), (2.0, -1.0, 3.0), (5, 6, 7)),
            ("diag2", (9, 12, 7), (2.0, 2.0, 2.0), (0.0, 0.0, 0.0), (5, 6, 4)),
            ("diag0.5", (5, 4, 3), (0.5, 0.5, 0.5), (0.0, 0.0, 0.0), (10, 8, 6))]


def thin_case():
    """A volume with a line of 1 (d) and a line of 2 (h): (shape, matrix, offset, output shape).  Row 0 of the matrix and its offset
    are zero, so the d coordinate is exactly 0 = n - 1 for every output."""
    return (1, 2, 5), np.array([[0.0, 0.0, 0.0], [0.03, 0.29, 0.011], [0.07, 0.013, 0.61]]), np.array([0.0, 0.0531, 0.2917]), (3, 4, 6)


PREFILTER_SHAPES = [(2, 3, 17), (17, 2, 3), (3, 17, 2), (SPLINE_TILE + 1, 3, 5), (5, SPLINE_TILE + 1, 3), (3, 5, SPLINE_TILE + 1),
                    (3, SPLINE_TILE + 1, SPLINE_TILE + 3), (1, 2, 5), (512, 2, 3)]          # 512: DM3D_SPLINE_MAX_EXTENT, the largest LDS image

# transform_image end to end
TI_SHAPE, TI_VOXSIZE, TI_INIT, TI_SCALE = (10, 12, 9), (1.5, 1.0, 2.0), (16, 16, 16), 2


def ti_affine():
    """A scanner affine for TI_SHAPE: the voxel sizes, a small rotation, and the volume centred on the world origin."""
    lin = _rotation(0.08, -0.05, 0.11) @ np.diag(TI_VOXSIZE)
    a = np.eye(4)
    a[:3, :3] = lin
    a[:3, 3] = -lin @ ((np.array(TI_SHAPE) - 1) / 2.0) + np.array([0.217, -0.331, 0.129])
    return a


def interpolating_values():
    """Every float64 value the GPU tests compare an interpolated float32 against (the cases behind RESAMPLE_F32_WORST)."""
    out = []
    mats, offs = generic_matrices()
    x = volumes(IN_SHAPE, 3)
    for order in (1, 3):
        for cval in CVALS:
            out += [affine_transform(x[b], mats[b], offs[b], OUT_SHAPE, order, cval) for b in range(3)]
    shape, m, off, oshape = thin_case()
    out += [affine_transform(volumes(shape, 1)[0], m, off, oshape, order) for order in (1, 3)]
    x2 = volumes(IN_SHAPE + (2,), 2, SEED + 1)
    out += [affine_transform(x2[b, ..., c], mats[b], offs[b], OUT_SHAPE, 3) for b in range(2) for c in range(2)]
    x3 = volumes(TI_SHAPE, 2)
    for b in range(2):
        transform_image(x3[b], ti_affine(), TI_VOXSIZE, TI_SCALE, TI_INIT, stages=out)
    return out
