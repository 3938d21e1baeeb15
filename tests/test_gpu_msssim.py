"""GPU parity of the 3-D multi-scale SSIM (include/dm3d.h, dm3d_ms_ssim_desc) against the float64 restatement of
tests/msssim_reference.py, and of the pair table behind metrics.pairwise_ms_ssim / sample_diversity.

The raw-ABI cases call dm3d_ms_ssim through ctypes with every device buffer guarded (tests/guarded_buffers.py): a halo or pooling read
past an input turns the score into NaN, a store past the output, a partials slot or the pooled scratch trips a sentinel.

The bar (msssim_reference.py derives it; tests/test_msssim_host.py holds it to what the restatement measures on the CPU):
    MSSSIM_TOL = 4 * 8.88e-7 = 3.55e-6    four times the worst |f32 - f64| of the restatement over these inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import msssim_reference as ms
from guarded_buffers import IN, OUT, Guarded

pytestmark = pytest.mark.gpu

TOL = ms.MSSSIM_TOL


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    return torch.device("cuda:0")


def _raw(dev, x, y, channels, filter_size, power, max_val, xi=None, yi=None):
    """dm3d_ms_ssim on guarded buffers: out [P] as numpy, after every guard was checked.  max_val: float32 [P]."""
    from dm3d_amd import _lib
    cx, x0c, cy, y0c, nc = channels
    nx, ny = x.shape[0], y.shape[0]
    dd, h, w = x.shape[1:4]
    P = len(max_val)
    f, m = filter_size, len(power)
    td, th, tw = _lib.MSSSIM_TILE
    tiles = sum(-(-((dd >> j) - f + 1) // td) * -(-((h >> j) - f + 1) // th) * -(-((w >> j) - f + 1) // tw) for j in range(m))
    pooled = sum((dd >> j) * (h >> j) * (w >> j) for j in range(1, m))
    gx, gy = Guarded(x, dev, IN), Guarded(y, dev, IN)
    gl = Guarded(np.asarray(max_val, np.float32), dev, IN)
    tables = [None if t is None else Guarded(np.asarray(t, np.int32), dev, IN) for t in (xi, yi)]
    part = Guarded(np.zeros(2 * P * nc * tiles, np.float64), dev, OUT)
    scratch = Guarded(np.zeros(max(1, (nx + ny) * nc * pooled), np.float32), dev, OUT)
    out = Guarded(np.zeros(P, np.float32), dev, OUT)
    d = _lib.MsSsimDesc()
    d.x, d.y, d.pairs, d.nx, d.ny, d.d, d.h, d.w = gx.ptr, gy.ptr, P, nx, ny, dd, h, w
    d.x_index, d.y_index = (None if t is None else t.ptr for t in tables)
    d.cx, d.cy, d.x0c, d.y0c, d.nc = cx, cy, x0c, y0c, nc
    d.filter_size, d.filter_sigma, d.scales = f, 1.5, m
    for j, wj in enumerate(power):
        d.power_factors[j] = wj
    d.max_val, d.out = gl.ptr, out.ptr
    d.partials, d.partials_elems = part.ptr, part.n // 2
    d.scratch, d.scratch_elems = (scratch.ptr, pooled * (nx + ny) * nc) if m > 1 else (None, 0)
    _lib.check(_lib.lib().dm3d_ms_ssim(C.byref(d), None), "ms_ssim")
    torch.cuda.synchronize()
    for g in [gx, gy, gl] + [t for t in tables if t is not None]:
        g.unchanged()
    part.get(), scratch.get()
    return out.get()


def _case_max_val(case, yc):
    """float32 [B]: the case's values, or what dm3d_pair_stats leaves as y_range: one float32 subtraction of the volume's max and min."""
    mv = ms.case_max_val(case)
    b = yc.shape[0]
    if mv is None:
        flat = yc.reshape(b, -1)
        return flat.max(axis=1) - flat.min(axis=1)
    return np.broadcast_to(np.asarray(mv, np.float32), (b,)).copy()


def _run_case(dev, case):
    shape, ch, f = case[0], case[1], case[2]
    x, y = ms.make_pair(shape, ch)
    _, yc = ms.compared(x, y, ch)
    return _raw(dev, x, y, ch, f, ms.case_power(case), _case_max_val(case, yc))


@pytest.mark.parametrize("case", ms.CASES, ids=ms.case_id)
def test_kernels_match_the_float64_restatement(dev, case):
    got = _run_case(dev, case)
    ref, per = ms.reference(case)
    assert np.isfinite(got).all(), "non-finite score (a read outside an input's extent?)"
    err = float(np.abs(got - ref).max())
    print(f"{ms.case_id(case)}: {err:.3e} (bar {TOL:.2e})  ms-ssim {ref}  lowest term {min(float(min(cs.min(), s.min())) for cs, s in per):.3f}")
    assert got.shape == ref.shape and got.dtype == np.float32
    assert err <= TOL


@pytest.mark.parametrize("case", [ms.CASES[4], ms.CASES[7], ms.CASES[-1]], ids=ms.case_id)
def test_runs_repeat_bitwise(dev, case):
    assert _run_case(dev, case).tobytes() == _run_case(dev, case).tobytes()


def test_pair_table_reads_volumes_in_place(dev):
    """Three volumes of x against two of y through both tables, a max_val per row; a row whose entry is out of range reads nothing and
    scores NaN."""
    t = ms.PAIR_TABLE
    ch, power, L, xi, yi = t["channels"], t["power"], t["max_val"], t["x_index"], t["y_index"]
    x, y = ms.pair_table_inputs()
    got = _raw(dev, x, y, ch, 3, power, L, xi, yi)
    ref = ms.ms_ssim(*ms.pair_table_rows(), L, power, 3)
    err = float(np.abs(got - ref).max())
    print(f"pair table: {err:.3e} (bar {TOL:.2e})  ms-ssim {ref}")
    assert err <= TOL
    bad = _raw(dev, x, y, ch, 3, power, L, [2, 3, 1, -1], [0, 1, 2, 0])
    assert np.isnan(bad[1:]).all() and bad[0].tobytes() == got[0].tobytes()


def test_wrappers_pairs_and_diversity(dev):
    from dm3d_amd import metrics, ops
    # ops on torch tensors gives what the raw entry gives; max_val None is max(y) - min(y) per volume and differs from a given one
    case = ms.CASES[6]                                                       # 2x16x16x16, 7 taps, a window that starts past channel 0
    shape, ch, f = case[0], case[1], case[2]
    x, y = (torch.from_numpy(a).to(dev) for a in ms.make_pair(shape, ch))
    kw = dict(power_factors=ms.case_power(case), filter_size=f, x_channels=(ch[1], ch[4]), y_channels=(ch[3], ch[4]))
    raw = _run_case(dev, case)
    auto = ops.ms_ssim(x, y, **kw)
    assert auto.is_cuda and auto.dtype == torch.float32 and auto.shape == (2,) and auto.cpu().numpy().tobytes() == raw.tobytes()
    assert torch.equal(auto, ops.ms_ssim(x, y, stats=ops.pair_stats(x, y, x_channels=kw["x_channels"], y_channels=kw["y_channels"]), **kw))
    fixed = metrics.ms_ssim(x, y, 1.0, **kw)
    assert torch.equal(fixed, ops.ms_ssim(x, y, torch.ones(2, device=dev), **kw)) and not torch.equal(fixed, auto)
    with pytest.raises(ValueError, match="at most 2 scales fit"):
        ops.ms_ssim(x, y, 1.0, **{**kw, "power_factors": ms.POWER_FACTORS[:3]})
    with pytest.raises(ValueError, match="max_val=None"):
        ops.ms_ssim(x, y, pairs=torch.zeros(1, 2, dtype=torch.int64, device=dev), **kw)

    # four volumes: the six pairs in lexicographic order, each bitwise what the two volumes give on their own
    kw = dict(power_factors=ms.BATCH["power"], filter_size=ms.BATCH["filter_size"])
    v = torch.from_numpy(ms.batch_volumes(4)).to(dev)
    L = ms.BATCH["max_val"]
    pw = metrics.pairwise_ms_ssim(v, L, **kw)
    order = [(i, j) for i in range(4) for j in range(i + 1, 4)]
    assert pw.shape == (6,) and pw.dtype == torch.float32 and pw.is_cuda
    for k, (i, j) in enumerate(order):
        assert torch.equal(pw[k:k + 1], ops.ms_ssim(v[i:i + 1], v[j:j + 1], L, **kw)), (i, j)
    ref = ms.ms_ssim(*ms.batch_rows(4), L, kw["power_factors"], 3)
    err = float(np.abs(pw.cpu().numpy() - ref).max())
    print(f"pairwise: {err:.3e} (bar {TOL:.2e})  ms-ssim {ref}")
    assert err <= TOL and len(set(pw.tolist())) == 6
    per_pair = torch.linspace(0.9, 1.3, 6, device=dev)
    assert torch.equal(metrics.pairwise_ms_ssim(v, per_pair, **kw)[2:3], ops.ms_ssim(v[0:1], v[3:4], per_pair[2:3], **kw))
    div = metrics.sample_diversity(v, L, **kw)
    assert div.dim() == 0 and div.dtype == torch.float64 and div.is_cuda and torch.equal(div, pw.double().mean())
    same = v[:1].expand(3, -1, -1, -1, -1).contiguous()
    assert float((metrics.pairwise_ms_ssim(same, L, **kw) - 1).abs().max()) <= TOL
    assert abs(float(metrics.sample_diversity(same, L, **kw)) - 1) <= TOL
