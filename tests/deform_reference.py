"""numpy restatement of the spatial augmentation entries (include/dm3d.h, "Spatial augmentation"; plain helper, no test in it, nothing
imported from the package): the separable Gaussian filter of scipy.ndimage.gaussian_filter(order=0), the Philox draw and the smoothing
of an elastic displacement field, the coordinate rule of the warp and the matrix composition of data.random_affine.  The interpolation
is tests/resample_reference.py's.  tests/test_deform_host.py holds it to scipy; tests/test_gpu_deform.py compares the kernels with it.

Every operation is written in the order the kernels use (elementwise numpy operations are IEEE, as the device's are, and the library
builds without contraction), so the filter and the field are expected bit for bit, and inside / outside and floor decisions of the warp
agree with the device."""
import numpy as np

import resample_reference as rr

STREAM_ELASTIC = 0xE1A5
GAUSS_MAX_RADIUS = 64
MODES = ("reflect", "mirror", "nearest", "constant")


# ---- the Gaussian filter -----------------------------------------------------------------------------------------------------------------
def gaussian_weights(sigma, truncate=4.0):
    """(r, w[0 .. r]) as scipy forms them: r = int(truncate sigma + 0.5), exp(-0.5 / sigma^2 k^2) over -r .. r divided by the sum."""
    sigma = float(sigma)
    r = int(truncate * sigma + 0.5)
    k = np.arange(-r, r + 1)
    phi = np.exp(-0.5 / (sigma * sigma) * k ** 2)
    phi = phi / phi.sum()
    return r, phi[r:]


def _tap(i, n, mode):
    """Where the taps i (any integers) of a line of n lie in the line; -1 reads cval."""
    i = np.asarray(i, np.int64)
    if mode == "nearest":
        return np.clip(i, 0, n - 1)
    if mode == "constant":
        return np.where((i >= 0) & (i < n), i, -1)
    if mode == "mirror":
        return rr.mirror(i, n)
    assert mode == "reflect"
    i = np.mod(i, 2 * n)
    return np.where(i < n, i, 2 * n - 1 - i)


def gaussian_filter1d(x, sigma, axis, mode="reflect", cval=0.0, truncate=4.0):
    """One axis pass on float32 data: t = x[l] w0, then t += (x[l-k] + x[l+k]) w_k for k = r .. 1 in float64, stored as float32."""
    r, w = gaussian_weights(sigma, truncate)
    a = np.moveaxis(np.asarray(x, np.float32), axis, 0)
    n = a.shape[0]
    ext = np.concatenate([a.astype(np.float64), np.full((1,) + a.shape[1:], float(cval))])          # row n (index -1) holds cval
    pos = np.arange(n)
    t = ext[pos] * w[0]
    for k in range(r, 0, -1):
        t = t + (ext[_tap(pos - k, n, mode)] + ext[_tap(pos + k, n, mode)]) * w[k]
    return np.ascontiguousarray(np.moveaxis(t.astype(np.float32), 0, axis))


def gaussian_filter(x, sigma, mode="reflect", cval=0.0, truncate=4.0):
    """The last three axes of float32 x filtered along d, then h, then w; an axis with sigma <= 1e-15 is left out.  float32."""
    sig = np.broadcast_to(np.asarray(sigma, np.float64), (3,))
    out = np.array(x, np.float32)
    for a in range(3):
        if sig[a] > 1e-15:
            out = gaussian_filter1d(out, sig[a], a - 3, mode, cval, truncate)
    return out


# ---- the elastic field -------------------------------------------------------------------------------------------------------------------
def uniform_field(n, seed, draw=0):
    """float32 [n]: element e is 2 v - 1, v = float32(word e & 3) * 2^-32 of the block of counter (lo32(e >> 2), hi32(e >> 2), draw,
    STREAM_ELASTIC) under the key seed (oracle/ref_philox.py's Philox4x32-10)."""
    from oracle import ref_philox as rp
    seed = int(seed) & (2 ** 64 - 1)
    b = np.arange((n + 3) // 4, dtype=np.uint64)
    words = rp.philox4x32_10(b & np.uint64(rp.MASK32), b >> np.uint64(32), draw, STREAM_ELASTIC, seed & rp.MASK32, seed >> 32)
    v = np.stack(words, 1).reshape(-1)[:n].astype(np.float32) * rp.TWO_M32_F32
    out = np.float32(2.0) * v - np.float32(1.0)
    assert out.dtype == np.float32
    return out


def elastic_field(shape, batch, alpha, sigma, seed, draw=0):
    """float32 [batch, 3, D, H, W]: gaussian_filter(U(-1, 1), sigma, "constant", 0) * alpha, alpha per component, one float32 multiply."""
    u = uniform_field(batch * 3 * int(np.prod(shape)), seed, draw).reshape((batch, 3) + tuple(shape))
    gain = np.broadcast_to(np.asarray(alpha, np.float64), (3,)).astype(np.float32)
    out = np.ascontiguousarray(gaussian_filter(u, sigma, "constant", 0.0) * gain[None, :, None, None, None])
    assert out.dtype == np.float32
    return out


# ---- the warp ----------------------------------------------------------------------------------------------------------------------------
def warp_coordinates(matrix, offset, field):
    """[3, od, oh, ow] float64: ((((o0 M[h][0] + o1 M[h][1]) + o2 M[h][2]) + offset[h]) + (double)field[h]; matrix None is the identity."""
    m = np.eye(3) if matrix is None else np.asarray(matrix, np.float64)
    if m.shape == (4, 4):
        m, offset = m[:3, :3], m[:3, 3]
    return rr.coordinates(m, offset, field.shape[1:]) + np.asarray(field).astype(np.float64)


def warp(x, field, matrix=None, offset=0.0, order=1, cval=0.0, prefilter=True):
    """One volume x [d, h, w] at warp_coordinates: float64 [od, oh, ow] (resample_reference.interpolate)."""
    src = rr.spline_filter(x) if order == 3 and prefilter else np.asarray(x, np.float64)
    return rr.interpolate(src, warp_coordinates(matrix, offset, field), order, cval)


# ---- random_affine's matrices ------------------------------------------------------------------------------------------------------------
def affine_matrices(shape, batch, seed, rotate_range=0.0, scale_range=0.0, translate_range=0.0):
    """[batch, 4, 4] float64 as data.random_affine states them: angles, scales, shifts drawn in that order from
    numpy.random.Generator(numpy.random.Philox(seed)); M = Rd Rh Rw diag(scales); offset = (centre - M centre) + shifts."""
    rot, sc, tr = (np.broadcast_to(np.asarray(v, np.float64), (3,)) for v in (rotate_range, scale_range, translate_range))
    rng = np.random.Generator(np.random.Philox(seed))
    angles = rng.uniform(-rot, rot, (batch, 3))
    scales = rng.uniform(1.0 - sc, 1.0 + sc, (batch, 3))
    shifts = rng.uniform(-tr, tr, (batch, 3))
    centre = (np.array(shape, np.float64) - 1.0) / 2.0
    out = np.zeros((batch, 4, 4))
    for b in range(batch):
        M = rr._rotation(*angles[b]) @ np.diag(scales[b])
        out[b, :3, :3], out[b, :3, 3], out[b, 3, 3] = M, (centre - M @ centre) + shifts[b], 1.0
    return out


# ---- the inputs of the GPU tests ---------------------------------------------------------------------------------------------------------
TAIL_SHAPES = [(5, 9, 37), (1, 6, 70), (3, 3, 3)]     # partial 16-wide bricks, a wave crossed, H W = 333: a partial group of 32 lines; r > n
SIGMAS = (0.7, 1.5, 3.0)
WARP_SHAPE, WARP_ALPHA, WARP_SIGMA, WARP_SEED = (9, 12, 37), 12.0, 2.0, 20261021
HALF_ULP_SHARE = 1e-3                                 # order 0: the share of outputs that may lie within 1 ulp of a half-integer


def warp_matrix():
    """A non-trivial [4, 4] matrix for WARP_SHAPE: a small rotation and scale about the centre and a fractional shift."""
    m = np.eye(4)
    M = rr._rotation(0.07, -0.05, 0.04) @ np.diag([1.05, 0.95, 1.02])
    c = (np.array(WARP_SHAPE) - 1) / 2.0
    m[:3, :3], m[:3, 3] = M, (c - M @ c) + np.array([0.3137, -0.4213, 0.1871])
    return m


def near_half(coords):
    """Where any of the three coordinates lies within 1 ulp of a half-integer: floor(c + 0.5) may fall either way."""
    h = np.floor(coords) + 0.5
    return (np.abs(coords - h) <= np.spacing(np.abs(h))).any(0)
