"""GPU parity of the volume preprocessing (include/dm3d.h, "Volume preprocessing") against the float64 numpy restatement of
tests/resample_reference.py, never against the device itself.

The raw-ABI cases call dm3d_spline_filter, dm3d_affine_resample, dm3d_volume_normalize and dm3d_augment through ctypes with every
device buffer guarded (tests/guarded_buffers.py); the wrapper cases go through dm3d_amd.ops and dm3d_amd.data.  Every case runs twice
and the second run must be bitwise the first.

Bars.  The prefilter's float64 coefficients: 1e-12 absolute on data in [0, 1], the bound the host test holds the restatement to against
scipy (the kernel performs the restatement's operations in its order, so equality is expected and printed).  Interpolated values:
RESAMPLE_TOL = 4 x 5.94e-08 = 2.376e-07, four times the worst |f32 - f64| of the restatement over these inputs, the three stages of
the transform_image case among them (the kernel keeps float64 up to its one float32 store; tests/test_resample_host.py measures
5.9374e-08; on an MI355X the worst |gpu - f64| was 5.5e-08 and every value bitwise the rounded restatement).  Orders 0 and the exact
cases: ==.  transform_image end to end: the same RESAMPLE_TOL against the restatement with its float32 stores (measured 0).
normalize: min and max bitwise numpy's, values within 2 float32 ulp of the float64 evaluation.  augment: 2^-24 on values in [0, 1]."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_reference as rr
from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu
COEFF_BOUND = 1e-12


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _twice(fn):
    """fn() twice: the two results (arrays or tuples of arrays) must be bitwise equal; returns the first."""
    a, b = fn(), fn()
    for u, v in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        if u is not None:
            assert np.array_equal(np.ascontiguousarray(u).view(np.uint8), np.ascontiguousarray(v).view(np.uint8)), "a second run differs from the first"
    return a


def _raw_spline(dev, x):
    """dm3d_spline_filter of float32 [V, d, h, w] on guarded buffers: float64 [V, d, h, w]."""
    from dm3d_amd import _lib
    gx, out = Guarded(x, dev, IN), Guarded(np.full(x.shape, -5.0, np.float64), dev, OUT)
    d = _lib.SplineDesc()
    d.x, d.coeff = gx.ptr, out.ptr
    d.volumes, d.d, d.h, d.w = x.shape
    _lib.check(_lib.lib().dm3d_spline_filter(C.byref(d), None), "spline_filter")
    torch.cuda.synchronize()
    gx.unchanged()
    return out.get()


def _raw_resample(dev, src, mats, offs, oshape, order, cval):
    """dm3d_affine_resample of [V, d, h, w] (float32 data or float64 coefficients) on guarded buffers: float32 [V, *oshape]."""
    from dm3d_amd import _lib
    V = src.shape[0]
    table = np.concatenate([np.asarray(mats, np.float64).reshape(V, 9), np.asarray(offs, np.float64).reshape(V, 3)], 1)
    gs, gt = Guarded(src, dev, IN), Guarded(table, dev, IN)
    out = Guarded(np.full((V,) + tuple(oshape), 77.0, np.float32), dev, OUT)
    d = _lib.ResampleDesc()
    d.src, d.table, d.out, d.in_f64 = gs.ptr, gt.ptr, out.ptr, int(src.dtype == np.float64)
    d.volumes, d.id, d.ih, d.iw = src.shape
    d.od, d.oh, d.ow = oshape
    d.order, d.cval = order, cval
    _lib.check(_lib.lib().dm3d_affine_resample(C.byref(d), None), "affine_resample")
    torch.cuda.synchronize()
    gs.unchanged(), gt.unchanged()
    return out.get()


def _raw_transform(dev, x, mats, offs, oshape, order, cval):
    """The prefilter (order 3) and the resample, both raw."""
    return _raw_resample(dev, _raw_spline(dev, x) if order == 3 else x, mats, offs, oshape, order, cval)


def _close(got, ref, bar, what):
    assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: worst |gpu - f64| {err:.3e} (bar {bar:.3e}), bitwise the rounded restatement: {np.array_equal(got, rr.f32(ref))}")
    assert err <= bar, (what, err, bar)


# ---- prefilter ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", rr.PREFILTER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_prefilter(dev, shape):
    """Lines of 1 (left unfiltered, as scipy leaves them), 2, 3, 17 and tile + 1 on every axis; line counts that fill no whole tile."""
    x = rr.volumes(shape, 2)
    got = _twice(lambda: _raw_spline(dev, x))
    ref = rr.spline_filter(x)
    err = float(np.abs(got - ref).max())
    print(f"prefilter {shape}: worst |gpu - restatement| {err:.3e}, bitwise: {np.array_equal(got, ref)}")
    assert np.isfinite(got).all() and err <= COEFF_BOUND


@pytest.mark.parametrize("shape", [(33, 1, 70), (1, 70, 33), (70, 33, 1)], ids=lambda s: "x".join(map(str, s)))
def test_prefilter_line_tiler(dev, shape):
    """What the shared line-pass tiler (csrc/dm3d_volume.h) can get wrong, through ops.spline_filter on two volumes: line counts that are no
    multiple of 32 (33, 70), more than one tile per group (70 > 64), an axis of extent 1 (its h or d pass is skipped, its w pass copies)
    and a group stride (two volumes)."""
    from dm3d_amd import ops
    x = rr.volumes(shape, 2)
    got = _twice(lambda: ops.spline_filter(torch.from_numpy(x).to(dev)).cpu().numpy())
    err = float(np.abs(got - rr.spline_filter(x)).max())
    print(f"prefilter tiler {shape}: worst |gpu - restatement| {err:.3e}")
    assert got.shape == x.shape and got.dtype == np.float64 and np.isfinite(got).all() and err <= COEFF_BOUND


def test_prefilter_wrapper_layouts(dev):
    from dm3d_amd import ops
    x = rr.volumes((5, 4, 6, 2), 2)                                             # NDHWC, C = 2: each channel a volume
    got = _twice(lambda: ops.spline_filter(torch.from_numpy(x).to(dev)).cpu().numpy())
    assert got.shape == x.shape and got.dtype == np.float64
    for c in range(2):
        assert np.abs(got[..., c] - rr.spline_filter(x[..., c])).max() <= COEFF_BOUND
    planar = ops.spline_filter(torch.from_numpy(np.ascontiguousarray(x[..., 0])).to(dev)).cpu().numpy()
    assert np.array_equal(planar, got[..., 0])


# ---- resample ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cval", rr.CVALS)
@pytest.mark.parametrize("order", [0, 1, 3])
def test_generic_affine(dev, order, cval):
    """(9, 12, 7) -> (10, 6, 13), three volumes under three full matrices (rotation, shear, non-unit scale, fractional offset)."""
    mats, offs = rr.generic_matrices()
    x = rr.volumes(rr.IN_SHAPE, 3)
    got = _twice(lambda: _raw_transform(dev, x, mats, offs, rr.OUT_SHAPE, order, cval))
    ref = np.stack([rr.affine_transform(x[b], mats[b], offs[b], rr.OUT_SHAPE, order, cval) for b in range(3)])
    outside = ref == float(np.float32(cval))
    assert np.array_equal(got == np.float32(cval), outside), "inside / outside decisions differ"
    if order == 0:
        assert np.array_equal(got, rr.f32(ref))
    else:
        _close(got, ref, rr.RESAMPLE_TOL, f"order {order} cval {cval}")


@pytest.mark.parametrize("order", [0, 1, 3])
def test_lines_of_one_and_two(dev, order):
    shape, m, off, oshape = rr.thin_case()
    x = rr.volumes(shape, 1)
    got = _twice(lambda: _raw_transform(dev, x, m[None], off[None], oshape, order, 0.0))
    ref = rr.affine_transform(x[0], m, off, oshape, order)[None]
    assert np.array_equal(got == 0.0, ref == 0.0)
    _close(got, ref, 0.0 if order == 0 else rr.RESAMPLE_TOL, f"thin volume, order {order}")


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("case", rr.exact_cases(), ids=lambda c: c[0])
def test_exact_cases(dev, case, order):
    """Identity, integer shift, diag(2), diag(0.5): coordinates exactly on 0 and n - 1 are inside, the next one is cval; compared with ==."""
    from dm3d_amd import ops
    name, ishape, m, off, oshape = case
    x = rr.volumes(ishape, 2)
    cval = rr.CVALS[1]
    got = _twice(lambda: _raw_resample(dev, x, np.stack([np.diag(m)] * 2), np.stack([off] * 2), oshape, order, cval))
    ref = np.stack([rr.affine_transform(x[b], m, off, oshape, order, cval) for b in range(2)])
    assert np.array_equal(got, rr.f32(ref)), name
    if name in ("shift", "diag0.5"):
        assert (got == np.float32(cval)).any()
    wrapped = ops.affine_transform(torch.from_numpy(x).to(dev), m, off, oshape, order=order, cval=cval).cpu().numpy()     # the 3-vector form
    assert np.array_equal(wrapped, got)


def test_ndhwc_two_channels(dev):
    from dm3d_amd import ops
    mats, offs = rr.generic_matrices()
    x = rr.volumes(rr.IN_SHAPE + (2,), 2, rr.SEED + 1)
    t = torch.from_numpy(x).to(dev)
    got = _twice(lambda: ops.affine_transform(t, mats[:2], offs[:2], rr.OUT_SHAPE).cpu().numpy())
    assert got.shape == (2,) + rr.OUT_SHAPE + (2,)
    ref = np.stack([np.stack([rr.affine_transform(x[b, ..., c], mats[b], offs[b], rr.OUT_SHAPE, 3) for c in range(2)], -1) for b in range(2)])
    _close(got, ref, rr.RESAMPLE_TOL, "NDHWC, C = 2")
    # prefilter=False reads x as the coefficients; a [4, 4] homogeneous matrix carries its offset
    hom = np.eye(4)
    hom[:3, :3], hom[:3, 3] = mats[0], offs[0]
    raw = ops.affine_transform(t[:1], hom, output_shape=rr.OUT_SHAPE, prefilter=False).cpu().numpy()
    ref = np.stack([rr.affine_transform(x[0, ..., c], mats[0], offs[0], rr.OUT_SHAPE, 3, prefilter=False) for c in range(2)], -1)[None]
    _close(raw, ref, rr.RESAMPLE_TOL, "prefilter=False")


def test_transform_image_end_to_end(dev):
    from dm3d_amd import data
    x = rr.volumes(rr.TI_SHAPE, 2)
    t = torch.from_numpy(x).to(dev)

    def run():
        out, a2 = data.transform_image(t, rr.ti_affine(), rr.TI_VOXSIZE, scale=rr.TI_SCALE, init_shape=rr.TI_INIT)
        return out.cpu().numpy(), a2

    got, a2 = _twice(run)
    refs = [rr.transform_image(x[b], rr.ti_affine(), rr.TI_VOXSIZE, rr.TI_SCALE, rr.TI_INIT) for b in range(2)]
    assert np.array_equal(a2, refs[0][1]) and got.shape == (2, 8, 8, 8)
    _close(got, np.stack([r[0] for r in refs]), rr.RESAMPLE_TOL, "transform_image")
    single, _ = data.transform_image(t[0], rr.ti_affine(), rr.TI_VOXSIZE, scale=rr.TI_SCALE, init_shape=rr.TI_INIT)       # one [D,H,W] volume
    assert np.array_equal(single.cpu().numpy(), got[0])
    image, mask, context = data.preprocess(t, rr.ti_affine(), rr.TI_VOXSIZE, mask=torch.ones_like(t), init_shape=rr.TI_INIT)
    assert image.shape == mask.shape == (2, 8, 8, 8, 1) and context.shape == (2, 1, 1) and context.dtype == torch.int64
    assert not mask.any() and not context.any() and float(image.min()) == 0.0 and float(image.max()) == 1.0
    want = np.stack([rr.normalize(got[b])[2] for b in range(2)])                # normalize's bar: 2 float32 ulp of the float64 evaluation
    ulp = np.spacing(np.abs(rr.f32(want))).astype(np.float64)
    assert (np.abs(image[..., 0].cpu().numpy().astype(np.float64) - want) <= 2.0 * ulp).all()


# ---- normalize ---------------------------------------------------------------------------------------------------------------------------
def _raw_normalize(dev, x):
    from dm3d_amd import _lib
    B, n = x.shape[0], int(np.prod(x.shape[1:]))
    gx, out = Guarded(x, dev, IN), Guarded(np.full(x.shape, 9.0, np.float32), dev, OUT)
    partials = Guarded(np.zeros((B, _lib.NORM_PARTIAL_BLOCKS, 2), np.float32), dev, OUT)
    minmax, flag = Guarded(np.full((B, 2), 9.0, np.float32), dev, OUT), Guarded(np.full(B, 9, np.int32), dev, OUT)
    d = _lib.NormalizeDesc()
    d.x, d.out, d.volumes, d.n, d.partials, d.minmax, d.flag = gx.ptr, out.ptr, B, n, partials.ptr, minmax.ptr, flag.ptr
    _lib.check(_lib.lib().dm3d_volume_normalize(C.byref(d), None), "volume_normalize")
    torch.cuda.synchronize()
    gx.unchanged(), partials.get()
    return out.get(), minmax.get(), flag.get()


@pytest.mark.parametrize("shape", [(5, 6, 7), (64, 64, 65)], ids=["small", "strided"])
def test_normalize(dev, shape):
    """Negatives present; the second shape exceeds 256 blocks of 1024, so every lane strides.  The last volume is constant."""
    from dm3d_amd import data
    rng = np.random.default_rng(rr.SEED)
    x = (rng.standard_normal((3,) + shape) * 3.0).astype(np.float32)
    x[2] = -1.25
    assert (x[:2] < 0).any()
    out, minmax, flag = _twice(lambda: _raw_normalize(dev, x))
    assert flag.tolist() == [0, 0, 1] and not out[2].any() and minmax[2].tolist() == [1.25, 1.25]
    for b in range(2):
        mn, mx, ref = rr.normalize(x[b])
        assert minmax[b, 0].tobytes() == mn.tobytes() and minmax[b, 1].tobytes() == mx.tobytes()
        ulp = np.spacing(np.abs(rr.f32(ref)).astype(np.float32)).astype(np.float64)
        worst = float((np.abs(out[b].astype(np.float64) - ref) / ulp).max())
        print(f"normalize {shape} volume {b}: worst error {worst:.2f} float32 ulp")
        assert worst <= 2.0 and out[b].min() == 0.0 and out[b].max() == 1.0
    t = torch.from_numpy(x).to(dev)
    assert np.array_equal(data.normalize(t[:2]).cpu().numpy(), out[:2])
    with pytest.raises(ValueError, match=r"volume\(s\) \[2\] are constant"):
        data.normalize(t)
    assert np.array_equal(data.normalize(t, check=False).cpu().numpy(), out)


# ---- augment -----------------------------------------------------------------------------------------------------------------------------
def _raw_augment(dev, x, mask, flip, brightness, contrast, draw=0, seed=0):
    from dm3d_amd import _lib
    B = x.shape[0]
    gx, gm = Guarded(x, dev, IN), Guarded(mask, dev, IN)
    out, mout = Guarded(np.full(x.shape, 9.0, np.float32), dev, OUT), Guarded(np.full(mask.shape, 9.0, np.float32), dev, OUT)
    tables = [Guarded(np.ascontiguousarray(t), dev, OUT if draw else IN) for t in (flip, brightness, contrast)]
    partials = Guarded(np.zeros((B, _lib.AUG_PARTIAL_BLOCKS), np.float64), dev, OUT)
    d = _lib.AugmentDesc()
    d.x, d.out, d.mask, d.mask_out = gx.ptr, out.ptr, gm.ptr, mout.ptr
    d.batch, d.d, d.h, d.w, d.c = x.shape
    d.cm = mask.shape[4]
    d.flip, d.brightness, d.contrast = (t.ptr for t in tables)
    d.draw, d.seed, d.flip_chance, d.brightness_lo, d.brightness_hi, d.contrast_lo, d.contrast_hi = draw, seed, 0.6, 0.9, 1.1, 0.9, 1.1
    d.partials = partials.ptr
    _lib.check(_lib.lib().dm3d_augment(C.byref(d), None), "augment")
    torch.cuda.synchronize()
    gx.unchanged(), gm.unchanged(), partials.get()
    if not draw:
        [t.unchanged() for t in tables]
    return (out.get(), mout.get()) + tuple(t.get() for t in tables)


def _check_augment(got, x, mask, what):
    out, mout, flip, b, c = got
    for i in range(x.shape[0]):
        ref, mref = rr.augment(x[i], mask[i], flip[i], b[i], c[i])
        err = float(np.abs(out[i].astype(np.float64) - ref).max())
        assert err <= rr.AUGMENT_TOL, (what, i, err)
        assert np.array_equal(mout[i], mref), (what, i)
    print(f"augment {what}: within {rr.AUGMENT_TOL:.2e}")


@pytest.mark.parametrize("shape", [(5, 6, 7, 1), (65, 64, 64, 1), (4, 3, 5, 2)], ids=["small", "strided", "two-channel"])
def test_augment_explicit(dev, shape):
    B = 4 if shape[0] < 65 else 2
    x = rr.volumes(shape, B) * 1.2                                              # some values clip at 1 after the brightness
    mask = (rr.volumes(shape[:3] + (2,), B, rr.SEED + 2) > 0.5).astype(np.float32)
    flip = np.array([0, 1, 1, 0], np.int32)[:B]
    b, c = np.array([0.9, 1.1, 1.037, 0.95], np.float32)[:B], np.array([0.91, 1.1, -0.5, 1.0], np.float32)[:B]
    got = _twice(lambda: _raw_augment(dev, x, mask, flip, b, c))
    _check_augment(got, x, mask, f"explicit {shape}")
    assert not np.array_equal(got[0][1], got[0][1][::-1])                      # the flipped sample is not symmetric: the flip is visible


def test_augment_seeded(dev):
    from dm3d_amd import data
    B, shape = 6, (5, 6, 7, 1)
    x = rr.volumes(shape, B)
    mask = (rr.volumes(shape, B, rr.SEED + 2) > 0.5).astype(np.float32)
    junk_i, junk_f = np.full(B, 9, np.int32), np.full(B, 9.0, np.float32)
    got = _twice(lambda: _raw_augment(dev, x, mask, junk_i, junk_f, junk_f, draw=7, seed=rr.SEED))
    flip, b, c = rr.augment_draw(rr.SEED, B)
    assert np.array_equal(got[2], flip) and got[3].tobytes() == b.tobytes() and got[4].tobytes() == c.tobytes()
    assert 0 < flip.sum() < B
    _check_augment(got, x, mask, "seeded")
    ti, tm = torch.from_numpy(x).to(dev), torch.from_numpy(mask).to(dev)
    res = data.augment(ti, tm, seed=rr.SEED)
    assert np.array_equal(res.images.cpu().numpy(), got[0]) and np.array_equal(res.masks.cpu().numpy(), got[1])
    assert np.array_equal(res.flip.cpu().numpy(), flip) and np.array_equal(res.brightness.cpu().numpy(), b)
    other = data.augment(ti, tm, seed=rr.SEED + 1)
    assert not np.array_equal(other.brightness.cpu().numpy(), b)
    # an explicit table overrides its draw and leaves the other draws as they were
    keep = data.augment(ti, seed=rr.SEED, flip=torch.zeros(B, dtype=torch.int32, device=dev))
    assert keep.masks is None and not keep.flip.any() and np.array_equal(keep.contrast.cpu().numpy(), c)
    big = rr.augment_draw(1 << 63, 3)
    hi = data.augment(ti[:3], seed=1 << 63)                                     # both key words count
    assert np.array_equal(hi.flip.cpu().numpy(), big[0]) and np.array_equal(hi.contrast.cpu().numpy(), big[2])
