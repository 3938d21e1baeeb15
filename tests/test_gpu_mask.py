"""GPU parity of the mask-channel scores (include/dm3d.h, dm3d_mask_desc) against the numpy restatement of tests/mask_reference.py.

The raw-ABI cases call dm3d_mask_overlap, dm3d_edt and dm3d_surface_distance through ctypes with every device buffer guarded
(tests/guarded_buffers.py): counts, surface masks and squared distance maps must equal the restatement's, every guard must be intact.
hd, hd_percentile and assd start from the same integers on both sides, so their bar is relative, (n + 4) * 2^-52 with n the surface
voxels summed (each sqrt and each add contributes at most one rounding; all terms are non-negative); the test takes n per (volume,
channel) from the reference.  A second run of every case is bitwise the first."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import mask_reference as mk
from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _bytes(n):
    """A guarded buffer takes 4-byte words: n bytes rounded up to whole words of zeros."""
    return np.zeros(-(-n // 4), np.int32)


def _as_bool(words, shape):
    flat = words.view(np.uint8)
    n = int(np.prod(shape))
    assert not flat[n:].any() and set(np.unique(flat[:n]).tolist()) <= {0, 1}
    return flat[:n].reshape(shape).astype(bool)


def _desc(_lib, gx, gy, x, y, window):
    cx0, cy0, nc = window
    d = _lib.MaskDesc()
    d.x, d.y = gx.ptr, (None if gy is None else gy.ptr)
    d.batch, d.d, d.h, d.w = x.shape[:4]
    d.cx, d.cy, d.x0c, d.y0c, d.nc = x.shape[4], (0 if y is None else y.shape[4]), cx0, cy0, nc
    d.threshold = mk.THRESHOLD
    return d


def _raw_overlap(dev, x, y):
    """dm3d_mask_overlap on guarded buffers: counts int64 [B, nc, 3], the two surface masks bool [B, nc, D, H, W]."""
    from dm3d_amd import _lib
    shape = (x.shape[0], mk.NC) + x.shape[1:4]
    gx, gy = Guarded(x, dev, IN), Guarded(y, dev, IN)
    counts = Guarded(np.full((x.shape[0], mk.NC, 3), -7, np.int64), dev, OUT)
    sx, sy = (Guarded(_bytes(int(np.prod(shape))), dev, OUT) for _ in range(2))
    d = _desc(_lib, gx, gy, x, y, (mk.X0C, mk.Y0C, mk.NC))
    d.counts, d.surf_x, d.surf_y = counts.ptr, sx.ptr, sy.ptr
    _lib.check(_lib.lib().dm3d_mask_overlap(C.byref(d), None), "mask_overlap")
    torch.cuda.synchronize()
    gx.unchanged(), gy.unchanged()
    with_surfaces = counts.get(), _as_bool(sx.get(), shape), _as_bool(sy.get(), shape)
    d.surf_x = d.surf_y = None                                                 # the counts alone
    _lib.check(_lib.lib().dm3d_mask_overlap(C.byref(d), None), "mask_overlap")
    assert np.array_equal(counts.get(), with_surfaces[0])
    return with_surfaces


def _raw_edt(dev, t, first, of):
    """dm3d_edt of one tensor's window (first, NC) on guarded buffers: int32 [B, nc, D, H, W]."""
    from dm3d_amd import _lib
    shape = (t.shape[0], mk.NC) + t.shape[1:4]
    n = int(np.prod(shape))
    gt = Guarded(t, dev, IN)
    masks, out = Guarded(_bytes(n), dev, OUT), Guarded(np.full(shape, -5, np.int32), dev, OUT)
    d = _desc(_lib, gt, None, t, None, (first, 0, mk.NC))
    d.of, d.map, d.masks, d.masks_elems = of, out.ptr, masks.ptr, n
    _lib.check(_lib.lib().dm3d_edt(C.byref(d), None), "edt")
    torch.cuda.synchronize()
    gt.unchanged(), masks.get()
    return out.get()


def _raw_surface_distance(dev, x, y, percentile):
    """dm3d_surface_distance on guarded buffers: out float64 [B, nc, 5] and the counts it leaves on the way."""
    from dm3d_amd import _lib
    B, D, H, W = x.shape[:4]
    vox = B * mk.NC * D * H * W
    bins = (D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 + 1
    gx, gy = Guarded(x, dev, IN), Guarded(y, dev, IN)
    out = Guarded(np.full((B, mk.NC, 5), -3.0, np.float64), dev, OUT)
    counts = Guarded(np.full((B, mk.NC, 3), -7, np.int64), dev, OUT)
    masks = Guarded(_bytes(2 * vox), dev, OUT)
    work = Guarded(np.zeros(vox + 2 * B * mk.NC * (bins + 1), np.int32), dev, OUT)
    d = _desc(_lib, gx, gy, x, y, (mk.X0C, mk.Y0C, mk.NC))
    d.percentile, d.out, d.counts = percentile, out.ptr, counts.ptr
    d.masks, d.masks_elems, d.work, d.work_elems = masks.ptr, 2 * vox, work.ptr, work.n
    _lib.check(_lib.lib().dm3d_surface_distance(C.byref(d), None), "surface_distance")
    torch.cuda.synchronize()
    gx.unchanged(), gy.unchanged(), masks.get(), work.get()
    return out.get(), counts.get()


def _check_distances(got, stats, what):
    """got float64 [B, nc, 5] against the reference's dicts: the three distances within the bar, the surface counts equal."""
    for b in range(got.shape[0]):
        for c in range(got.shape[1]):
            s = stats[b][c]
            assert got[b, c, 3] == s["surface_x"] and got[b, c, 4] == s["surface_y"], (what, b, c, got[b, c], s)
            for k, key in enumerate(("hd", "hd_percentile", "assd")):
                g, r = float(got[b, c, k]), s[key]
                rel = abs(g - r) / abs(r) if r and not math.isnan(r) else 0.0
                print(f"{what} [{b},{c}] {key}: got {g!r} ref {r!r} rel {rel:.2e} (bar {mk.bound(s['n']):.2e}, n {s['n']})")
                assert mk.within(g, r, s["n"]), (what, b, c, key, g, r, s["n"])


@pytest.mark.parametrize("case", mk.CASES, ids=mk.case_id)
def test_counts_and_surfaces_equal_the_restatement(dev, case):
    x, y = mk.make_case(case)
    ref = mk.reference(case)
    counts, sx, sy = _raw_overlap(dev, x, y)
    assert counts.dtype == np.int64 and np.array_equal(counts, ref["counts"]), (counts.tolist(), ref["counts"].tolist())
    assert np.array_equal(sx, ref["surf_x"]), f"{int((sx != ref['surf_x']).sum())} voxels of x's surface differ"
    assert np.array_equal(sy, ref["surf_y"]), f"{int((sy != ref['surf_y']).sum())} voxels of y's surface differ"


@pytest.mark.parametrize("case", mk.CASES, ids=mk.case_id)
def test_squared_distance_maps_equal_the_restatement(dev, case):
    from dm3d_amd import _lib
    x, y = mk.make_case(case)
    ref = mk.reference(case)
    for name, t, first, want in (("x", x, mk.X0C, ref["map_x"]), ("y", y, mk.Y0C, ref["map_y"])):
        got = _raw_edt(dev, t, first, _lib.EDT_SURFACE)
        assert got.dtype == np.int32 and np.array_equal(got, want), f"{name}: {int((got != want).sum())} of {want.size} voxels differ"
    # the map of the mask itself: 0 inside it
    got = _raw_edt(dev, y, mk.Y0C, _lib.EDT_FOREGROUND)
    want = np.stack([np.stack([mk.sq_distance_map(ref["my"][b, c]) for c in range(mk.NC)]) for b in range(mk.BATCH)])
    assert np.array_equal(got, want), f"foreground: {int((got != want).sum())} of {want.size} voxels differ"


@pytest.mark.parametrize("case", mk.CASES, ids=mk.case_id)
def test_surface_distances_meet_the_restatement_and_repeat_bitwise(dev, case):
    x, y = mk.make_case(case)
    ref = mk.reference(case)
    for p in mk.PERCENTILES:
        got, counts = _raw_surface_distance(dev, x, y, p)
        assert np.array_equal(counts, ref["counts"])
        _check_distances(got, ref["stats"][p], f"{mk.case_id(case)} p{p:g}")
        again, counts2 = _raw_surface_distance(dev, x, y, p)
        assert again.tobytes() == got.tobytes() and counts2.tobytes() == counts.tobytes()


@pytest.mark.parametrize("shape", [(33, 1, 70), (1, 70, 33), (70, 33, 1)], ids=lambda s: "x".join(map(str, s)))
def test_distance_transform_line_tiler(dev, shape):
    """What the shared line-pass tiler (csrc/dm3d_volume.h) can get wrong, through ops.distance_transform on two volumes of two channels
    with a window of one: column counts that are no multiple of 32 (33, 70), more than one tile per group (70 > 64), an axis of extent
    1 (its pass still runs: the d pass writes INT32_MAX) and a group stride (batch * nc = 2).  Exact: int32 against the brute force."""
    from dm3d_amd import ops
    rng = np.random.default_rng([11] + list(shape))
    x = rng.random((2,) + shape + (2,)).astype(np.float32)
    x[..., 1] = np.stack([mk.values_of(mk.mask_of("balls", shape, seed=b), rng) for b in range(2)])
    m = mk.masks(x, 1, 1)
    t = torch.from_numpy(x).to(dev)
    for of, feat in (("surface", mk.surface), ("foreground", lambda v: v)):
        got = ops.distance_transform(t, mk.THRESHOLD, channels=(1, 1), of=of)
        again = ops.distance_transform(t, mk.THRESHOLD, channels=(1, 1), of=of)
        want = np.stack([mk.sq_distance_map(feat(m[b, 0])) for b in range(2)])[..., None]
        assert got.dtype == torch.int32 and got.shape == (2,) + shape + (1,) and torch.equal(got, again)
        assert np.array_equal(got.cpu().numpy(), want), f"{of}: {int((got.cpu().numpy() != want).sum())} of {want.size} voxels differ"


def test_the_interpolation_is_exercised():
    """About the inputs, on the CPU side: at both percentiles some (volume, channel) has its two ranks on different squared distances."""
    for p in mk.PERCENTILES:
        assert any(s["split"] for case in mk.CASES for row in mk.reference(case)["stats"][p] for s in row), p


def test_wrappers(dev):
    from dm3d_amd import metrics, ops
    case = ((5, 7, 9), "edges")                                                  # one full pair, two half-empty ones, one empty one
    xn, yn = mk.make_case(case)
    ref = mk.reference(case)
    x, y = torch.from_numpy(xn.copy()).to(dev), torch.from_numpy(yn.copy()).to(dev)
    kw = dict(x_channels=(mk.X0C, mk.NC), y_channels=(mk.Y0C, mk.NC))
    counts = ops.mask_overlap(x, y, **kw)
    assert all(t.dtype == torch.int64 and t.is_cuda and t.shape == (2, 2) for t in counts)
    assert np.array_equal(torch.stack(list(counts), -1).cpu().numpy(), ref["counts"])
    dist = ops.surface_distances(x, y, mk.THRESHOLD, 95.0, **kw)
    assert all(t.dtype == torch.float64 and t.is_cuda and t.shape == (2, 2) for t in dist)
    _check_distances(torch.stack(list(dist), -1).cpu().numpy(), ref["stats"][95.0], "ops.surface_distances")
    dt = ops.distance_transform(x, channels=kw["x_channels"])
    assert dt.dtype == torch.int32 and dt.shape == (2, 5, 7, 9, 2)
    assert np.array_equal(dt.permute(0, 4, 1, 2, 3).cpu().numpy(), ref["map_x"])
    fg = ops.distance_transform(y, channels=kw["y_channels"], of="foreground")
    assert bool(((fg == 0) == (y > mk.THRESHOLD)).all())
    # mask_metrics equals its parts, bitwise
    m = metrics.mask_metrics(x, y, **kw)
    dice, iou = metrics.dice(x, y, **kw), metrics.iou(x, y, **kw)
    rd, ri = mk.dice_iou(ref["counts"])
    for got, part, want in ((m["dice"], dice, rd), (m["iou"], iou, ri)):
        assert got.dtype == torch.float64 and got.cpu().numpy().tobytes() == part.cpu().numpy().tobytes()
        assert np.array_equal(got.cpu().numpy(), want, equal_nan=True)
    for k, t in dist._asdict().items():
        assert m[k].cpu().numpy().tobytes() == t.cpu().numpy().tobytes(), k
    assert all(torch.equal(a, b) for a, b in zip(m["counts"], counts))
    assert metrics.hausdorff(x, y, **kw).cpu().numpy().tobytes() == dist.hd_percentile.cpu().numpy().tobytes()
    assert metrics.hausdorff(x, y, percentile=None, **kw).cpu().numpy().tobytes() == dist.hd.cpu().numpy().tobytes()
    # the edges group: Dice is NaN where the truth is empty, and the running mean skips it
    assert torch.isnan(dice).sum() == 2 and torch.isnan(dist.hd).sum() == 3
    mean, plain = metrics.NanMean("mask_dice"), metrics.Mean("mask_dice")
    mean.update_state(dice), plain.update_state(dice)
    assert mean.result().is_cuda and float(mean.result()) == float(np.nanmean(rd)) and int(mean.count) == 2 and math.isnan(float(plain.result()))
    with pytest.raises(ValueError, match="same number must be compared"):
        ops.mask_overlap(x, y)
    with pytest.raises(ValueError, match="threshold must be finite"):
        ops.mask_overlap(x, y, float("nan"), **kw)


def _model(dev):
    from dm3d_amd.networks.vqvae3d_monai import VQVAE
    return VQVAE(2, 2, (16, 32), 1, (16, 32), downsample_parameters=((2, 4, 1, "same"),) * 2,
                 upsample_parameters=((2, 4, 1, "same", 0),) * 2, num_embeddings=64, embedding_dim=8, device=dev, seed=3, input_size=16)


def test_evaluate_scores_the_mask_half(dev):
    """A tiny 2-in / 2-out VQVAE: mask_evaluate(batches) gives the restatement's numbers for the reconstruction model(x) returns;
    evaluate(batches) returns exactly METRIC_KEYS with the same values.  (evaluate keeps the signature tests/test_metrics_host.py pins,
    so the mask scores have an entry of their own, not a keyword.)"""
    vq = _model(dev)
    rng = np.random.default_rng(5)
    # synthetic weights put the mask channel of the reconstruction anywhere: move the last layer's bias of that channel so that its median
    # over a probe batch sits on the threshold, and the reconstructed masks are neither empty nor full
    probe = torch.from_numpy(rng.random((1, 16, 16, 16, 2)).astype(np.float32)).to(dev)
    state = {k: v.copy() for k, v in vq.state.items()}
    state["dec.up1.bias"][1] += 0.5 - float(vq(probe)[0][..., 1].median())
    vq.load_state_dict(state)
    batches = []
    for n in (2, 1):
        img = rng.random((n, 16, 16, 16, 1)).astype(np.float32)
        mask = np.stack([mk.mask_of("balls", (16, 16, 16), seed=10 * n + i) for i in range(n)])[..., None].astype(np.float32)
        batches.append((torch.from_numpy(img), torch.from_numpy(mask), None))
    batches[1][1].zero_()                                                      # an empty truth: its Dice is NaN and is skipped
    per = {k: [] for k in vq.MASK_METRIC_KEYS}
    bars = {k: 0.0 for k in vq.MASK_METRIC_KEYS}
    for img, mask, _ in batches:
        recon, _ = vq(torch.cat([img, mask], -1).to(dev).contiguous())
        rn = recon.cpu().numpy()
        mx, my = mk.masks(mask.numpy(), 0, 1), mk.masks(rn, 1, 1)
        dice, iou = mk.dice_iou(mk.overlap_counts(mx, my))
        for b in range(img.shape[0]):
            s = mk.surface_stats(mx[b, 0], my[b, 0], 95.0)
            per["mask_dice"].append(dice[b, 0]), per["mask_iou"].append(iou[b, 0])
            per["mask_hd95"].append(s["hd_percentile"]), per["mask_assd"].append(s["assd"])
            bars["mask_hd95"] = bars["mask_assd"] = max(bars["mask_assd"], mk.bound(s["n"]))
    assert 0.0 < per["mask_dice"][0] < 1.0 and per["mask_hd95"][0] > 0.0 and per["mask_assd"][1] > 0.0, per   # a reconstruction that says something
    got = vq.mask_evaluate(batches)
    assert tuple(got) == vq.METRIC_KEYS + vq.MASK_METRIC_KEYS and all(isinstance(v, float) for v in got.values())
    for k in vq.MASK_METRIC_KEYS:
        vals = [v for v in per[k] if not math.isnan(v)]
        want = math.fsum(vals) / len(vals) if vals else 0.0
        # the mean of m values adds m roundings and one division to the per-value bar (0 for the overlap scores, exact ratios of counts)
        bar = bars[k] + (len(vals) + 2) * 2.0 ** -52
        print(f"{k}: got {got[k]!r} want {want!r} over {len(vals)} of {len(per[k])} values (bar {bar:.2e})")
        assert abs(got[k] - want) <= bar * abs(want), (k, got[k], want)
    assert math.isnan(per["mask_dice"][2]) and not math.isnan(per["mask_dice"][0])
    plain = vq.evaluate(batches)
    assert tuple(plain) == vq.METRIC_KEYS and all(plain[k] == got[k] for k in vq.METRIC_KEYS)
    assert set(vq.test_step(batches[0])) == set(vq.METRIC_KEYS) and set(vq.mask_test_step(batches[0])) == set(got)
