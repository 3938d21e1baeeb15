"""GPU parity of the connected-component entries (include/dm3d.h, dm3d_ccl_desc) against the numpy restatement of
tests/components_reference.py.

The raw-ABI cases call dm3d_components and dm3d_component_filter through ctypes with every device buffer guarded
(tests/guarded_buffers.py): labels, count, largest and the three filter modes must equal the restatement's, the input must be unchanged
and every guard intact.  All results are integers (or the floats 0 and 1), so every comparison is an equality, and a second run of
every case is bitwise the first."""
import ctypes as C

import numpy as np
import pytest
import torch

import components_reference as cr
from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu

PARAMS = [(case, conn) for case in cr.CASES for conn in cr.CONNECTIVITIES]
IDS = [f"{cr.case_id(case)}-c{conn}" for case, conn in PARAMS]


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _work_words(x, planes):
    from dm3d_amd import _lib
    B, D, H, W = x.shape[:4]
    nblk = -(-(D * H * W) // _lib.CCL_BLOCK_VOXELS)
    return planes * B * cr.NC * D * H * W + 1 + B * cr.NC * (3 * nblk + 2)


def _desc(_lib, gx, x, conn, work):
    d = _lib.CclDesc()
    d.x = gx.ptr
    d.batch, d.d, d.h, d.w = x.shape[:4]
    d.cx, d.x0c, d.nc = x.shape[4], cr.X0C, cr.NC
    d.threshold, d.connectivity = cr.THRESHOLD, conn
    d.work, d.work_elems = work.ptr, work.n
    return d


def _raw_components(dev, x, conn):
    """dm3d_components on guarded buffers: labels int32 [B, nc, D, H, W], count int32 [B, nc], largest int64 [B, nc, 2]."""
    from dm3d_amd import _lib
    shape = (x.shape[0], cr.NC) + x.shape[1:4]
    gx = Guarded(x, dev, IN)
    labels = Guarded(np.full(shape, -5, np.int32), dev, OUT)
    count = Guarded(np.full(shape[:2], -7, np.int32), dev, OUT)
    largest = Guarded(np.full(shape[:2] + (2,), -9, np.int64), dev, OUT)
    work = Guarded(np.zeros(_work_words(x, 2), np.int32), dev, OUT)
    d = _desc(_lib, gx, x, conn, work)
    d.labels, d.count, d.largest = labels.ptr, count.ptr, largest.ptr
    _lib.check(_lib.lib().dm3d_components(C.byref(d), None), "components")
    torch.cuda.synchronize()
    gx.unchanged(), work.get()
    return labels.get(), count.get(), largest.get()


def _raw_filter(dev, x, conn, mode, min_size=0):
    """dm3d_component_filter on guarded buffers: float32 [B, D, H, W, nc]."""
    from dm3d_amd import _lib
    gx = Guarded(x, dev, IN)
    out = Guarded(np.full(x.shape[:4] + (cr.NC,), -3.0, np.float32), dev, OUT)
    work = Guarded(np.zeros(_work_words(x, 3), np.int32), dev, OUT)
    d = _desc(_lib, gx, x, conn, work)
    d.mode, d.min_size, d.out = mode, min_size, out.ptr
    _lib.check(_lib.lib().dm3d_component_filter(C.byref(d), None), "component_filter")
    torch.cuda.synchronize()
    gx.unchanged(), work.get()
    return out.get()


@pytest.mark.parametrize("case,conn", PARAMS, ids=IDS)
def test_labels_count_and_largest_equal_the_restatement(dev, case, conn):
    x, ref = cr.make_case(case), cr.reference(case, conn)
    labels, count, largest = _raw_components(dev, x, conn)
    assert labels.dtype == np.int32 and count.dtype == np.int32 and largest.dtype == np.int64
    assert np.array_equal(count, ref["count"]), (count.tolist(), ref["count"].tolist())
    assert np.array_equal(largest, ref["largest"]), (largest.tolist(), ref["largest"].tolist())
    assert np.array_equal(labels, ref["labels"]), f"{int((labels != ref['labels']).sum())} of {labels.size} labels differ"
    again = _raw_components(dev, x, conn)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (labels, count, largest)))


@pytest.mark.parametrize("case,conn", PARAMS, ids=IDS)
def test_filters_equal_the_restatement(dev, case, conn):
    from dm3d_amd import _lib
    x, ref = cr.make_case(case), cr.reference(case, conn)
    modes = [("largest", _lib.CCL_LARGEST, 0), ("fill_holes", _lib.CCL_FILL_HOLES, 0)]
    modes += [(("min_size", n), _lib.CCL_MIN_SIZE, n) for n in cr.MIN_SIZES]
    for key, mode, n in modes:
        got, want = _raw_filter(dev, x, conn, mode, n), cr.ndhwc(ref["filters"][key])
        assert got.dtype == np.float32 and np.array_equal(got, want), f"{key}: {int((got != want).sum())} of {want.size} voxels differ"
        assert _raw_filter(dev, x, conn, mode, n).tobytes() == got.tobytes(), key


def _host_clean(x, first, count, **kw):
    m = cr.masks(x, first, count)
    return cr.ndhwc(np.stack([np.stack([cr.clean(m[b, c], **kw) for c in range(m.shape[1])]) for b in range(m.shape[0])]))


def test_wrappers(dev):
    from dm3d_amd import data, metrics, ops
    case, conn = ((17, 33, 65), "blobs"), 18
    xn, ref = cr.make_case(case), cr.reference(case, conn)
    x = torch.from_numpy(xn.copy()).to(dev)
    window = (cr.X0C, cr.NC)
    comp = ops.connected_components(x, cr.THRESHOLD, channels=window, connectivity=conn)
    assert comp.labels.dtype == torch.int32 and comp.labels.shape == (2, 17, 33, 65, 2) and comp.labels.is_cuda
    assert comp.count.dtype == torch.int32 and comp.count.shape == (2, 2) and comp.largest.dtype == torch.int64 and comp.largest.shape == (2, 2, 2)
    assert np.array_equal(comp.labels.permute(0, 4, 1, 2, 3).cpu().numpy(), ref["labels"])
    assert np.array_equal(comp.count.cpu().numpy(), ref["count"]) and np.array_equal(comp.largest.cpu().numpy(), ref["largest"])
    stats = metrics.component_stats(x, cr.THRESHOLD, channels=window, connectivity=conn)
    assert stats["components"].dtype == torch.int32 and np.array_equal(stats["components"].cpu().numpy(), ref["count"])
    total = ref["m"].reshape(2, 2, -1).sum(-1).astype(np.float64)
    assert stats["largest_fraction"].dtype == torch.float64
    assert np.array_equal(stats["largest_fraction"].cpu().numpy(), ref["largest"][..., 1].astype(np.float64) / total)
    # single stages, then all three in the documented order
    for kw, key in ((dict(keep="largest"), "largest"), (dict(min_size=5), ("min_size", 5)), (dict(fill_holes=True), "fill_holes")):
        got = ops.component_filter(x, cr.THRESHOLD, channels=window, connectivity=conn, **kw)
        assert got.dtype == torch.float32 and got.shape == (2, 17, 33, 65, 2) and got.is_contiguous()
        assert np.array_equal(got.cpu().numpy(), cr.ndhwc(ref["filters"][key])), key
    got = ops.component_filter(x, cr.THRESHOLD, channels=window, connectivity=conn, keep="largest", min_size=5, fill_holes=True)
    assert np.array_equal(got.cpu().numpy(), _host_clean(xn, *window, min_size=5, connectivity=conn))
    # clean_mask on the holes group (shell, tunnel, diagonal cavity, NaN background) and on the edges group (full, empty, single)
    for group in ("holes", "edges", "touch"):
        hn = cr.make_case(((17, 33, 65), group))
        hx = torch.from_numpy(np.ascontiguousarray(hn[..., cr.X0C:cr.X0C + cr.NC])).to(dev)
        for kw in (dict(), dict(min_size=2, connectivity=26), dict(keep_largest=False), dict(fill_holes=False, connectivity=18)):
            got = data.clean_mask(hx, **kw)
            want = _host_clean(hn, *window, keep_largest_=kw.get("keep_largest", True), fill=kw.get("fill_holes", True),
                               min_size=kw.get("min_size"), connectivity=kw.get("connectivity", 6))
            assert got.shape == hx.shape and np.array_equal(got.cpu().numpy(), want), (group, kw)
    # mask_metrics of the cleaned tensor equals mask_metrics of the host-cleaned one, bitwise
    yn = cr.make_case(((17, 33, 65), "holes"))
    y = torch.from_numpy(np.ascontiguousarray(yn[..., cr.X0C:cr.X0C + cr.NC])).to(dev)
    truth = torch.from_numpy(_host_clean(yn, *window, keep_largest_=False)).to(dev)
    a = metrics.mask_metrics(truth, data.clean_mask(y))
    b = metrics.mask_metrics(truth, torch.from_numpy(_host_clean(yn, *window)).to(dev))
    for k in ("dice", "iou", "hd", "hd_percentile", "assd"):
        assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), k


def test_an_empty_mask_has_no_fraction(dev):
    from dm3d_amd import metrics
    xn = cr.make_case(((5, 7, 9), "edges"))                                     # full, empty, single, speckle
    x = torch.from_numpy(xn.copy()).to(dev)
    ref = cr.reference(((5, 7, 9), "edges"), 6)
    stats = metrics.component_stats(x, channels=(cr.X0C, cr.NC))
    frac = stats["largest_fraction"].cpu().numpy()
    assert np.array_equal(stats["components"].cpu().numpy(), ref["count"])
    assert frac[0, 0] == 1.0 and np.isnan(frac[0, 1]) and frac[1, 0] == 1.0 and 0.0 < frac[1, 1] < 1.0
