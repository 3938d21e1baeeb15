"""GPU parity of the spatial augmentation (include/dm3d.h, "Spatial augmentation") against the numpy restatement of
tests/deform_reference.py, never against the device itself.

The raw-ABI cases call dm3d_gaussian_filter, dm3d_uniform_field and dm3d_warp through ctypes with every device buffer guarded
(tests/guarded_buffers.py); the wrapper cases go through dm3d_amd.ops and dm3d_amd.data.

Bars.  The Gaussian filter and the elastic field: bitwise the restatement, which tests/test_deform_host.py holds to scipy bit for bit
(the kernel performs the restatement's float64 operations in its order and stores float32 after every axis).  Warped values: four times
the float32 rounding gap of the restatement on the case at hand (resample_reference.f32_gap, the bar tests/test_gpu_resample.py holds
affine_transform to: the kernel keeps float64 up to its one float32 store).  Outside voxels: cval exactly.  Order 0: ==, except where a
reference coordinate lies within 1 ulp of a half-integer; at most 0.1 % of the outputs may be left out so, asserted from the reference.
Shapes: (5, 9, 37), (1, 6, 70) and (3, 3, 3) leave partial 16-wide bricks, cross a wave, leave a partial group of 32 lines (H W = 333)
and, at sigma = 3 (radius 12), have a radius longer than every axis."""
import ctypes as C

import numpy as np
import pytest
import torch

import deform_reference as dr
import resample_reference as rr
from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu
SHAPE_IDS = ["x".join(map(str, s)) for s in dr.TAIL_SHAPES]


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def warp_case():
    """The volume, the reference field at alpha = 12, sigma = 2 on (9, 12, 37) and the matrix, computed once and left unchanged."""
    x = rr.volumes(dr.WARP_SHAPE, 2)
    field = dr.elastic_field(dr.WARP_SHAPE, 2, dr.WARP_ALPHA, dr.WARP_SIGMA, dr.WARP_SEED)
    for a in (x, field):
        a.setflags(write=False)
    return x, field, dr.warp_matrix()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), f"{what}: {int((a != b).sum())} of {a.size} values differ"


def _close(got, ref, what):
    """|gpu - f64| within four times the restatement's own float32 rounding gap; cval voxels are exact and checked by the caller."""
    bar = 4.0 * rr.f32_gap(ref)
    assert got.dtype == np.float32 and got.shape == ref.shape and np.isfinite(got).all(), what
    err = float(np.abs(got.astype(np.float64) - ref).max())
    print(f"{what}: worst |gpu - f64| {err:.3e} (bar {bar:.3e}), bitwise the rounded restatement: {np.array_equal(got, rr.f32(ref))}")
    assert err <= bar, (what, err, bar)


# ---- raw entries on guarded buffers ------------------------------------------------------------------------------------------------------
def _raw_gauss(dev, x, sigma, mode, cval, gain=None, in_place=False):
    from dm3d_amd import _lib, ops
    radii, table = ops._gauss_table(sigma, 4.0)
    d = _lib.GaussDesc()
    if in_place:
        out = Guarded(x, dev, OUT)
        d.x = d.out = out.ptr
    else:
        gx, out = Guarded(x, dev, IN), Guarded(np.full(x.shape, 77.0, np.float32), dev, OUT)
        d.x, d.out = gx.ptr, out.ptr
    d.weights = table.ctypes.data
    d.volumes, d.d, d.h, d.w = x.shape
    d.rd, d.rh, d.rw = radii
    d.mode, d.cval = _lib.GAUSS_MODES[mode], cval
    if gain is not None:
        d.gains, (d.gain0, d.gain1, d.gain2) = 3, gain
    _lib.check(_lib.lib().dm3d_gaussian_filter(C.byref(d), None), "gaussian_filter")
    torch.cuda.synchronize()
    if not in_place:
        gx.unchanged()
    return out.get()


def _raw_uniform(dev, n, seed, draw):
    from dm3d_amd import _lib
    out = Guarded(np.full(n, 77.0, np.float32), dev, OUT)
    d = _lib.FieldDesc()
    d.out, d.n, d.seed, d.draw = out.ptr, n, seed, draw
    _lib.check(_lib.lib().dm3d_uniform_field(C.byref(d), None), "uniform_field")
    torch.cuda.synchronize()
    return out.get()


def _raw_warp(dev, src, table, field, oshape, order, cval, per_field=1):
    from dm3d_amd import _lib
    V = src.shape[0]
    gs, gt = Guarded(src, dev, IN), Guarded(np.ascontiguousarray(table, np.float64), dev, IN)
    gf = None if field is None else Guarded(field, dev, IN)
    out = Guarded(np.full((V,) + tuple(oshape), 77.0, np.float32), dev, OUT)
    d = _lib.WarpDesc()
    d.src, d.table, d.field, d.out = gs.ptr, gt.ptr, (None if gf is None else gf.ptr), out.ptr
    d.in_f64, d.field_f64 = int(src.dtype == np.float64), int(field is not None and field.dtype == np.float64)
    d.volumes, d.id, d.ih, d.iw = src.shape
    d.vols_per_field = per_field
    d.od, d.oh, d.ow = oshape
    d.order, d.cval = order, cval
    _lib.check(_lib.lib().dm3d_warp(C.byref(d), None), "warp")
    torch.cuda.synchronize()
    gs.unchanged(), gt.unchanged()
    if gf is not None:
        gf.unchanged()
    return out.get()


# ---- the Gaussian filter -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", dr.MODES)
@pytest.mark.parametrize("shape", dr.TAIL_SHAPES, ids=SHAPE_IDS)
def test_gaussian_filter_is_the_restatement_bitwise(dev, shape, mode):
    """Two volumes on guarded buffers: the three sigmas, a per-axis sigma with one 0, cval != 0; a second run equals the first; in place."""
    x = rr.volumes(shape, 2)
    for sigma, cval in [(s, 0.0) for s in dr.SIGMAS] + [((1.5, 0.0, 0.7), 0.0), (1.5, -0.375)]:
        ref = np.stack([dr.gaussian_filter(x[b], sigma, mode, cval) for b in range(2)])
        got = _raw_gauss(dev, x, sigma, mode, cval)
        _same(got, ref, f"gaussian {shape} {mode} sigma {sigma} cval {cval}")
        _same(_raw_gauss(dev, x, sigma, mode, cval), got, "a second run")
    _same(_raw_gauss(dev, x, 1.5, mode, -0.375, in_place=True), ref, "in place")


def test_gaussian_filter_wrapper_layouts(dev):
    from dm3d_amd import ops
    x = rr.volumes(dr.TAIL_SHAPES[0] + (2,), 2)                                 # NDHWC, C = 2: each channel a volume
    got = ops.gaussian_filter(torch.from_numpy(x).to(dev), (0.7, 1.5, 3.0), mode="mirror").cpu().numpy()
    assert got.shape == x.shape
    for b in range(2):
        for c in range(2):
            _same(got[b, ..., c], dr.gaussian_filter(x[b, ..., c], (0.7, 1.5, 3.0), "mirror"), f"NDHWC item {b} channel {c}")
    planar = np.ascontiguousarray(x[..., 0])
    t = torch.from_numpy(planar).to(dev)
    _same(ops.gaussian_filter(t, 1.5, "constant", 0.25).cpu().numpy(), np.stack([dr.gaussian_filter(v, 1.5, "constant", 0.25) for v in planar]), "[B,D,H,W]")
    _same(ops.gaussian_filter(t, 0.0).cpu().numpy(), planar, "every axis left out: a copy")
    assert np.array_equal(t.cpu().numpy(), planar)                              # the input is left alone


# ---- the elastic field -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", dr.TAIL_SHAPES, ids=SHAPE_IDS)
def test_elastic_field_draws_and_smoothing(dev, shape):
    from dm3d_amd import ops
    seed, n = 0x0123456789ABCDEF, 2 * 3 * int(np.prod(shape))
    raw = _raw_uniform(dev, n, seed, 0)                                         # n = 1110, 2520, 162: not every Philox block is whole
    _same(raw, dr.uniform_field(n, seed), f"uniform field of {n}")
    draws = ops.elastic_field(shape, 2, 1.0, 0.0, seed, device=dev).cpu().numpy()
    _same(draws.reshape(-1), raw, "elastic_field at sigma 0, alpha 1")
    assert draws.min() >= -1.0 and draws.max() <= 1.0 and abs(float(draws.mean())) < 0.2
    for alpha, sigma in ((12.0, 2.0), ((3.0, 0.0, 7.5), (1.5, 0.0, 0.7))):
        got = ops.elastic_field(shape, 2, alpha, sigma, seed, device=dev).cpu().numpy()
        _same(got, dr.elastic_field(shape, 2, alpha, sigma, seed), f"elastic field {shape} alpha {alpha} sigma {sigma}")
        _same(ops.elastic_field(shape, 2, alpha, sigma, seed, device=dev).cpu().numpy(), got, "a second run")
    other = ops.elastic_field(shape, 2, 1.0, 0.0, seed, draw=1, device=dev).cpu().numpy()
    _same(other, dr.uniform_field(n, seed, 1).reshape(other.shape), "draw 1")
    assert not np.array_equal(other, draws)
    # the smoothed, scaled field on guarded buffers, in place as ops.elastic_field runs it
    u = dr.uniform_field(n, seed).reshape((6,) + tuple(shape))
    _same(_raw_gauss(dev, u, 2.0, "constant", 0.0, gain=(12.0, 0.5, -3.0), in_place=True).reshape((2, 3) + tuple(shape)),
          dr.elastic_field(shape, 2, (12.0, 0.5, -3.0), 2.0, seed), "guarded field")


# ---- the warp ----------------------------------------------------------------------------------------------------------------------------
def _check_warp(got, x, field, matrix, order, cval, what):
    """One volume against the restatement: outside voxels are cval exactly, order 0 is == off the half-integers, the rest within the bar."""
    coords = dr.warp_coordinates(matrix, 0.0, field)
    inside = rr.inside_mask(coords, x.shape)
    assert 0.5 <= inside.mean() <= 0.99, (what, float(inside.mean()))
    ref = dr.warp(x, field, matrix, order=order, cval=cval)
    assert (got[~inside] == np.float32(cval)).all() and (ref[~inside] == float(np.float32(cval))).all(), what
    if order == 0:
        skip = dr.near_half(coords)
        assert skip.mean() <= dr.HALF_ULP_SHARE
        assert np.array_equal(got[~skip], rr.f32(ref)[~skip]), what
    else:
        _close(got, ref, what)


@pytest.mark.parametrize("with_matrix", [False, True], ids=["identity", "matrix"])
@pytest.mark.parametrize("f64", [False, True], ids=["field32", "field64"])
@pytest.mark.parametrize("order", [0, 1, 3])
def test_warp(dev, warp_case, order, f64, with_matrix):
    """(9, 12, 37), two volumes with a field each, through ops.warp; cval != 0."""
    from dm3d_amd import ops
    x, field, m = warp_case
    field = field.astype(np.float64) if f64 else field
    matrix = m if with_matrix else None
    cval = -0.375
    got = ops.warp(torch.tensor(x, device=dev), torch.tensor(field, device=dev), matrix, order=order, cval=cval).cpu().numpy()
    for b in range(2):
        _check_warp(got[b], x[b], field[b], matrix, order, cval, f"warp order {order} volume {b}")


@pytest.mark.parametrize("order", [0, 1, 3])
def test_warp_raw_on_guarded_buffers(dev, warp_case, order):
    """dm3d_warp itself on the tail shape (5, 9, 37) -> output (3, 6, 35): four volumes, two to a field, no write outside the output."""
    from dm3d_amd import _lib  # noqa: F401  (the library is loaded by the fixture's require_device)
    shape, oshape, OFFSET = dr.TAIL_SHAPES[0], (3, 6, 35), (1.0, 1.5, 3.25)
    x = rr.volumes(shape, 4)
    field = dr.elastic_field(oshape, 2, 6.0, 1.5, dr.WARP_SEED + 1)
    tables = np.concatenate([np.eye(3).reshape(1, 9).repeat(4, 0), np.array([OFFSET]).repeat(4, 0)], 1)
    src = rr.spline_filter(x) if order == 3 else x
    got = _raw_warp(dev, src, tables, field, oshape, order, 0.5, per_field=2)
    for v in range(4):
        ref = dr.warp(x[v], field[v // 2], np.eye(3), OFFSET, order, 0.5)
        coords = dr.warp_coordinates(np.eye(3), OFFSET, field[v // 2])
        inside = rr.inside_mask(coords, shape)
        assert 0.5 <= inside.mean() <= 0.99 and (got[v][~inside] == 0.5).all()
        if order == 0:
            skip = dr.near_half(coords)
            assert skip.mean() <= dr.HALF_ULP_SHARE and np.array_equal(got[v][~skip], rr.f32(ref)[~skip])
        else:
            _close(got[v], ref, f"raw warp order {order} volume {v}")
    none = _raw_warp(dev, src, tables, None, oshape, order, 0.5)                  # no field: dm3d_affine_resample's values
    from test_gpu_resample import _raw_resample
    _same(none, _raw_resample(dev, src, tables[:, :9].reshape(4, 3, 3), tables[:, 9:], oshape, order, 0.5), "no field")


@pytest.mark.parametrize("order", [0, 1, 3])
def test_map_coordinates_equals_warp(dev, warp_case, order):
    from dm3d_amd import ops
    x, field, _ = warp_case
    t, u = torch.tensor(x, device=dev), torch.tensor(field, device=dev)
    grid = np.stack(np.meshgrid(*(np.arange(s, dtype=np.float64) for s in dr.WARP_SHAPE), indexing="ij"))
    coords = torch.from_numpy(grid[None] + field.astype(np.float64)).to(dev)
    a, b = ops.map_coordinates(t, coords, order=order, cval=0.25).cpu().numpy(), ops.warp(t, u, order=order, cval=0.25).cpu().numpy()
    _same(a, b, f"map_coordinates order {order}")
    assert 0.5 <= (a != np.float32(0.25)).mean() <= 0.99


def test_channels_share_a_field(dev, warp_case):
    from dm3d_amd import ops
    _, field, m = warp_case
    x = rr.volumes(dr.WARP_SHAPE + (2,), 2, rr.SEED + 1)
    t, u = torch.from_numpy(x).to(dev), torch.tensor(field, device=dev)
    for order in (0, 1, 3):
        both = ops.warp(t, u, m, order=order).cpu().numpy()
        assert both.shape == x.shape
        for c in range(2):
            _same(both[..., c:c + 1], ops.warp(t[..., c:c + 1].contiguous(), u, m, order=order).cpu().numpy(), f"order {order} channel {c}")
    shared = ops.warp(t, u[:1].contiguous(), m, order=1).cpu().numpy()            # one field for the whole batch
    _same(shared[1], ops.warp(t[1:].contiguous(), u[:1].contiguous(), m[None], order=1).cpu().numpy()[0], "a [1,3,...] field serves every item")
    _same(shared[0], ops.warp(t, u, m, order=1).cpu().numpy()[0], "item 0 under field 0")


# ---- data --------------------------------------------------------------------------------------------------------------------------------
def test_elastic_deform(dev):
    from dm3d_amd import data
    shape = dr.WARP_SHAPE
    x = rr.volumes(shape + (2,), 2)
    mask = (rr.volumes(shape + (1,), 2, rr.SEED + 2) > 0.5).astype(np.float32)
    ti, tm = torch.from_numpy(x).to(dev), torch.from_numpy(mask).to(dev)
    res = data.elastic_deform(ti, tm, alpha=12.0, sigma=2.0, seed=dr.WARP_SEED, cval=0.0)
    field = res.field.cpu().numpy()
    _same(field, dr.elastic_field(shape, 2, 12.0, 2.0, dr.WARP_SEED), "the field")
    assert res.matrices is None and res.images.shape == x.shape and res.masks.shape == mask.shape
    got, gm = res.images.cpu().numpy(), res.masks.cpu().numpy()
    assert set(np.unique(gm)) <= {0.0, 1.0} and 0.1 < gm.mean() < 0.9                  # a binary mask stays binary at mask_order = 0
    for b in range(2):
        for c in range(2):
            _check_warp(got[b, ..., c], x[b, ..., c], field[b], None, 1, 0.0, f"elastic_deform item {b} channel {c}")
        _check_warp(gm[b, ..., 0], mask[b, ..., 0], field[b], None, 0, 0.0, f"mask {b}")
    # consistently: the image of the mask at order 0 is the mask that came back
    again = data.elastic_deform(tm, tm, alpha=12.0, sigma=2.0, seed=dr.WARP_SEED, order=0)
    _same(again.images.cpu().numpy(), gm, "image and mask under one field")
    _same(again.masks.cpu().numpy(), gm, "mask")
    for order in (0, 1):                                                        # alpha = 0: the identity returns the image bitwise
        still = data.elastic_deform(ti, tm, alpha=0.0, sigma=2.0, seed=1, order=order)
        _same(still.images.cpu().numpy(), x, f"alpha 0, order {order}")
        _same(still.masks.cpu().numpy(), mask, "alpha 0, mask")
        assert not still.field.any()


def test_spatial_augment(dev):
    from dm3d_amd import data
    shape = dr.WARP_SHAPE
    x = rr.volumes(shape + (1,), 2)
    mask = (rr.volumes(shape + (1,), 2, rr.SEED + 2) > 0.5).astype(np.float32)
    ti, tm = torch.from_numpy(x).to(dev), torch.from_numpy(mask).to(dev)
    seed, ranges = dr.WARP_SEED, dict(rotate_range=0.08, scale_range=0.05, translate_range=0.5)
    ela = data.elastic_deform(ti, tm, alpha=12.0, sigma=2.0, seed=seed)
    only_field = data.spatial_augment(ti, tm, seed=seed, elastic_alpha=12.0, elastic_sigma=2.0)
    _same(only_field.images.cpu().numpy(), ela.images.cpu().numpy(), "all ranges 0: elastic_deform")
    _same(only_field.masks.cpu().numpy(), ela.masks.cpu().numpy(), "all ranges 0: its mask")
    assert np.array_equal(only_field.matrices, np.broadcast_to(np.eye(4), (2, 4, 4)))
    aff = data.random_affine(ti, tm, seed=seed, **ranges)
    only_affine = data.spatial_augment(ti, tm, seed=seed, **ranges)
    _same(only_affine.images.cpu().numpy(), aff.images.cpu().numpy(), "elastic_alpha None: random_affine")
    _same(only_affine.masks.cpu().numpy(), aff.masks.cpu().numpy(), "elastic_alpha None: its mask")
    mats = dr.affine_matrices(shape, 2, seed, **ranges)
    assert only_affine.field is None and np.array_equal(aff.matrices, mats) and not np.array_equal(mats[0], mats[1])
    for b in range(2):                                                          # random_affine against the affine restatement
        _close(aff.images.cpu().numpy()[b, ..., 0], rr.affine_transform(x[b, ..., 0], mats[b], order=1), f"random_affine item {b}")
    both = data.spatial_augment(ti, tm, seed=seed, elastic_alpha=12.0, elastic_sigma=2.0, cval=-0.375, **ranges)
    field = both.field.cpu().numpy()
    _same(field, ela.field.cpu().numpy(), "one seed, one field")
    assert np.array_equal(both.matrices, mats)
    for b in range(2):
        _check_warp(both.images.cpu().numpy()[b, ..., 0], x[b, ..., 0], field[b], mats[b], 1, -0.375, f"spatial_augment item {b}")
        _check_warp(both.masks.cpu().numpy()[b, ..., 0], mask[b, ..., 0], field[b], mats[b], 0, -0.375, f"spatial_augment mask {b}")
