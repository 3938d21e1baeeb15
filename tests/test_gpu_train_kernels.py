"""GPU parity of every training and normalisation entry of the C ABI, one kernel at a time, called through ctypes as a host would
(no Trainer in between) and compared with the float64 restatements of oracle/ref_kernels.py.

Each entry gets a hand-written list of edge cases (channel tails, rows that leave threads or blocks idle, grid caps, NULL optional
pointers, leading dimensions larger than the matrices) and a seeded random sweep.  Every output buffer sits between sentinel words
that must survive the call, and every "+=" output starts from random non-zero values.

Tolerances (max |err| / max |ref|): contractions and reductions 2e-5 (LAYER_TOL of test_gpu_train.py), LayerNorm-type row kernels
3e-6, elementwise 1e-6, data movement and q_sample bitwise, the float64 loss n * 2^-53.  A float32 reduction can only be held to its
bar where float32 itself stays inside it: each reduction test first asserts that a sequential float32 evaluation on the CPU
(np.cumsum; a float32 contraction for dm3d_wgrad) is within half the bar of float64, and the inputs are sized accordingly.
The worst error per entry is printed at the end of the module (docs/EXPERIMENTS.md records a run)."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import ref_kernels as rk

pytestmark = pytest.mark.gpu

LAYER_TOL, ROW_TOL, ELEM_TOL = 2e-5, 3e-6, 1e-6
NONE, RELU, SILU = 0, 1, 2
PAD = 64                                 # sentinel elements on each side of a buffer (a multiple of 4: pointers stay 16-byte aligned)
SENTINEL = -123456.0
WORST = {}


@pytest.fixture(scope="module")
def dev():
    from dm3d_amd import _lib
    _lib.require_device()
    torch.cuda.set_device(0)
    yield torch.device("cuda:0")
    for name in sorted(WORST):
        print(f"worst error {name}: {WORST[name]:.2e}")


class Buf:
    """A device buffer holding `arr` between two runs of sentinel elements."""

    def __init__(self, arr, dev):
        a = np.ascontiguousarray(arr)
        self.shape, self.n = a.shape, a.size
        self.t = torch.full((self.n + 2 * PAD,), SENTINEL, dtype=torch.from_numpy(a.reshape(-1)[:1].copy()).dtype, device=dev)
        self.t[PAD:PAD + self.n] = torch.from_numpy(a.reshape(-1)).to(dev)
        self.ptr = self.t.data_ptr() + PAD * self.t.element_size()
        assert self.ptr % 16 == 0

    def get(self):
        torch.cuda.synchronize()
        assert bool((self.t[:PAD] == SENTINEL).all()) and bool((self.t[PAD + self.n:] == SENTINEL).all()), "sentinel padding overwritten"
        return self.t[PAD:PAD + self.n].cpu().numpy().reshape(self.shape)


def _call(name, *args):
    from dm3d_amd import _lib
    _lib.check(getattr(_lib.lib(), name)(*args, None), name)


def _err(name, got, ref, scale=None):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    e = float(np.abs(got - ref).max() / max(float(np.abs(ref).max()) if scale is None else scale, 1e-30))
    WORST[name] = max(WORST.get(name, 0.0), e)
    print(f"{name}: {e:.2e}")
    return e


def _f32(rng, *shape, mean=0.0, std=1.0):
    return (rng.standard_normal(shape) * std + mean).astype(np.float32)


def _t64(a):
    return torch.from_numpy(np.asarray(a, np.float64))


def _cumsum32(a):
    """Column sums of a float32 matrix by sequential float32 addition."""
    return np.cumsum(np.asarray(a, np.float32), axis=0, dtype=np.float32)[-1]


def _rows_with_an_idle_block(c, rows_per_thread, cap):
    """A row count for which the last slab of the reduction kernels is empty: the grid is clamp(rows / (par * rows_per_thread), 1, cap)
    blocks of ceil(rows / grid) rows each, par = 256 / min(c / 4, 256).  Narrow tensors have no such count within the 20 000 rows a
    float32 sum can be held to the bar for (it takes about (par * rows_per_thread)^2 rows): they get two slabs with a ragged second one."""
    unit = 256 // min(c // 4, 256) * rows_per_thread
    for rows in range(2, 20000):
        grid = min(max(rows // unit, 1), cap)
        if (grid - 1) * -(-rows // grid) >= rows:
            return rows
    return min(2 * unit + 1, 20000)


CHANNELS = [4, 20, 36, 100, 256, 1028, 2048]


def _row_counts(c, rows_per_thread, cap):
    return [1, 7, _rows_with_an_idle_block(c, rows_per_thread, cap), min(3000, 1_000_000 // c)]


# ---- dm3d_wgrad ----------------------------------------------------------------------------------------------------------------------
WGRAD_CASES = [
    # name, batch, (d, h, w), cin, cout, ksize
    ("k3_c4_c4", 2, (3, 4, 5), 4, 4, 3),
    ("k3_c12_c36", 2, (3, 4, 5), 12, 36, 3),                    # cin % 8 == 4: the second float4 of the last piece is masked
    ("k3_c36_c12", 2, (3, 4, 5), 36, 12, 3),                    # cout <= 32: one whole wave masked
    ("k3_c68_c100", 2, (3, 4, 5), 68, 100, 3),
    ("k3_c100_c68", 1, (4, 3, 5), 100, 68, 3),
    ("k3_c132_c132", 1, (3, 3, 3), 132, 132, 3),
    ("k3_c4_c132", 2, (2, 3, 4), 4, 132, 3),
    ("k3_c132_c4", 2, (2, 3, 4), 132, 4, 3),
    ("k3_d1", 2, (1, 5, 6), 12, 20, 3),
    ("k3_h1", 2, (5, 1, 6), 12, 20, 3),
    ("k3_w1", 2, (5, 6, 1), 12, 20, 3),
    ("k3_single_voxel", 3, (1, 1, 1), 36, 12, 3),
    ("k3_line", 2, (1, 1, 7), 20, 36, 3),
    ("k3_chunk_straddles_samples", 3, (3, 3, 5), 20, 12, 3),    # 45 voxels per sample: 32-voxel chunks span two samples
    ("k3_straddle_wide", 4, (2, 3, 7), 68, 36, 3),              # 42 voxels per sample
    ("k3_uneven_k_slices", 2, (6, 9, 11), 12, 12, 3),           # 38 chunks in 9 K slices
    ("k3_many_k_slices", 2, (15, 15, 15), 36, 20, 3),           # 211 chunks in 52 K slices
    ("k1_flat_rows", 3, (5, 1, 7), 68, 36, 1),
    ("k1_flat_rows_big", 2, (10, 10, 25), 132, 100, 1),
    ("k1_one_row", 1, (1, 1, 1), 4, 4, 1),
]


def _random_wgrad_cases(n, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for i in range(n):
        ks = int(rng.choice([1, 3, 3]))
        size = tuple(int(v) for v in rng.integers(1, 7, 3))
        cin, cout = (int(v) * 4 for v in rng.integers(1, 36, 2))
        cases.append((f"rand{i}_k{ks}_{size[0]}x{size[1]}x{size[2]}_{cin}to{cout}", int(rng.integers(1, 4)), size, cin, cout, ks))
    return cases


WGRAD_ALL = WGRAD_CASES + _random_wgrad_cases(12, 20260201)


@pytest.mark.parametrize("case", WGRAD_ALL, ids=[c[0] for c in WGRAD_ALL])
def test_wgrad(dev, case):
    from dm3d_amd import _lib
    name, B, (D, H, W), cin, cout, ks = case
    rng = np.random.default_rng(sum(map(ord, name)))
    a, g = _f32(rng, B, D, H, W, cin), _f32(rng, B, D, H, W, cout)
    pre = _f32(rng, ks ** 3, cin, cout)
    ref = rk.wgrad(_t64(a), _t64(g), ks).numpy()
    f32 = rk.wgrad(torch.from_numpy(a), torch.from_numpy(g), ks).numpy()
    assert np.abs(f32 - ref).max() / np.abs(ref).max() < LAYER_TOL / 2          # float32 itself is inside half the bar
    da, dg, dw = Buf(a, dev), Buf(g, dev), Buf(pre, dev)
    d = _lib.WgradDesc()
    d.a, d.g, d.dw = da.ptr, dg.ptr, dw.ptr
    d.batch, d.in_d, d.in_h, d.in_w, d.cin, d.cout, d.ksize = B, D, H, W, cin, cout, ks
    _lib.check(_lib.lib().dm3d_wgrad(C.byref(d), None), "wgrad")
    assert _err("dm3d_wgrad", dw.get() - pre.astype(np.float64), ref) < LAYER_TOL


def test_wgrad_per_item_output_with_strides(dev):
    """`batch` independent contractions, every operand with a stride larger than its matrix; the gaps of dw stay as they were."""
    from dm3d_amd import _lib
    rng = np.random.default_rng(5)
    for batch, rows, cin, cout in ((3, 50, 36, 20), (3, 1, 4, 68), (2, 200, 100, 132)):
        sa, sg, sdw = rows * cin + 16, rows * cout + 12, cin * cout + 7
        a, g, pre = _f32(rng, batch, sa), _f32(rng, batch, sg), _f32(rng, batch, sdw)
        da, dg, dw = Buf(a, dev), Buf(g, dev), Buf(pre, dev)
        d = _lib.WgradDesc()
        d.a, d.g, d.dw = da.ptr, dg.ptr, dw.ptr
        d.batch, d.in_d, d.in_h, d.in_w, d.cin, d.cout, d.ksize = batch, rows, 1, 1, cin, cout, 1
        d.per_item_output, d.stride_a, d.stride_g, d.stride_dw = 1, sa, sg, sdw
        _lib.check(_lib.lib().dm3d_wgrad(C.byref(d), None), "wgrad")
        got = dw.get()
        for b in range(batch):
            am, gm = a[b, :rows * cin].reshape(rows, cin), g[b, :rows * cout].reshape(rows, cout)
            ref = _t64(am).T @ _t64(gm)
            assert np.abs(am.T @ gm - ref.numpy()).max() / np.abs(ref.numpy()).max() < LAYER_TOL / 2
            delta = got[b, :cin * cout].astype(np.float64) - pre[b, :cin * cout]
            assert _err("dm3d_wgrad", delta.reshape(cin, cout), ref.numpy()) < LAYER_TOL
            assert np.array_equal(got[b, cin * cout:], pre[b, cin * cout:])


# ---- dm3d_colsum ---------------------------------------------------------------------------------------------------------------------
COLSUM_CASES = [(c, rows, groups) for c in CHANNELS
                for rows, groups in zip(_row_counts(c, 8, 256), itertools.cycle([1, 3, 2]))]


@pytest.mark.parametrize("c,rows,groups", COLSUM_CASES)
def test_colsum(dev, c, rows, groups):
    rng = np.random.default_rng(c * 7 + rows)
    ld = c if groups == 1 else c + 8
    x, pre = _f32(rng, groups * rows, c, mean=0.2), _f32(rng, groups, ld)
    ref = rk.colsum(_t64(x), groups).numpy()
    f32 = np.stack([_cumsum32(x[i * rows:(i + 1) * rows]) for i in range(groups)])
    assert np.abs(f32 - ref).max() / np.abs(ref).max() < LAYER_TOL / 2
    dx, out = Buf(x, dev), Buf(pre, dev)
    _call("dm3d_colsum", dx.ptr, groups, rows, c, out.ptr, ld)
    got = out.get()
    assert _err("dm3d_colsum", got[:, :c].astype(np.float64) - pre[:, :c], ref) < LAYER_TOL
    assert np.array_equal(got[:, c:], pre[:, c:])                    # the columns between groups


# ---- dm3d_bn_act_bwd -----------------------------------------------------------------------------------------------------------------
def _bn_cases():
    cases, variant = [], itertools.count()
    for c in CHANNELS:
        for rows in _row_counts(c, 8, 512):
            v = next(variant)
            two = c >= 8 and v % 2 == 0
            # (dx1 wanted, dx2 wanted, dgamma wanted)
            want = [(1, 1, 1), (0, 1, 1), (1, 0, 1), (0, 0, 1), (1, 1, 0), (0, 0, 0)][v % 6]
            cases.append((c, rows, two, v % 3, want))
    cases += [(20, 50, True, SILU, (0, 1, 1)), (20, 50, True, RELU, (1, 0, 0)), (36, 9, False, NONE, (0, 0, 1)), (100, 640, True, SILU, (1, 1, 1))]
    return cases


@pytest.mark.parametrize("c,rows,two,act,want", _bn_cases())
def test_bn_act_bwd(dev, c, rows, two, act, want):
    rng = np.random.default_rng(c * 11 + rows + act)
    c1 = 4 * max(c // 12, 1) if two else c                           # an uneven split: the boundary is not a power of two
    c2 = c - c1
    x, g = _f32(rng, rows, c, mean=0.3, std=1.5), _f32(rng, rows, c)
    mean, rstd = _f32(rng, c, mean=0.3, std=0.1), (rng.random(c) + 0.5).astype(np.float32)
    gamma, beta = _f32(rng, c, mean=1.0, std=0.2), _f32(rng, c, std=0.3)
    scale = (gamma * rstd).astype(np.float32)
    shift = (beta - mean * scale).astype(np.float32)
    dx_ref, dgamma_ref, dbeta_ref, red_ref = (t.numpy() for t in rk.bn_act_bwd(*(_t64(v) for v in (g, x, scale, shift, mean, rstd)), act))
    # float32 on the CPU, sequential sums
    du32 = (torch.from_numpy(g) * rk.act_grad(torch.from_numpy(x) * torch.from_numpy(scale) + torch.from_numpy(shift), act)).numpy()
    xh32 = (x - mean) * rstd
    assert np.abs(_cumsum32(du32) - red_ref[:, 0]).max() / np.abs(red_ref[:, 0]).max() < LAYER_TOL / 2
    assert np.abs(_cumsum32(du32 * xh32) - red_ref[:, 1]).max() / np.abs(red_ref[:, 1]).max() < LAYER_TOL / 2
    x1, x2 = np.ascontiguousarray(x[:, :c1]), np.ascontiguousarray(x[:, c1:])
    pre1, pre2, pre_g, pre_b = _f32(rng, rows, c1), _f32(rng, rows, max(c2, 1)), _f32(rng, c), _f32(rng, c)
    bufs = {k: Buf(v, dev) for k, v in dict(g=g, x1=x1, x2=x2 if two else np.zeros(4, np.float32), scale=scale, shift=shift, mean=mean, rstd=rstd,
                                            dx1=pre1, dx2=pre2, dgamma=pre_g, dbeta=pre_b).items()}
    red = Buf(np.zeros((c, 2), np.float64), dev)
    w1, w2, wg = want
    w2 = w2 and two
    _call("dm3d_bn_act_bwd", bufs["g"].ptr, bufs["x1"].ptr, c1, bufs["x2"].ptr if two else None, c2, rows, bufs["scale"].ptr, bufs["shift"].ptr,
          bufs["mean"].ptr, bufs["rstd"].ptr, act, red.ptr, bufs["dx1"].ptr if w1 else None, bufs["dx2"].ptr if w2 else None,
          bufs["dgamma"].ptr if wg else None, bufs["dbeta"].ptr if wg else None)
    got_red = red.get()
    assert _err("dm3d_bn_act_bwd red", got_red[:, 0], red_ref[:, 0]) < LAYER_TOL
    assert _err("dm3d_bn_act_bwd red", got_red[:, 1], red_ref[:, 1]) < LAYER_TOL
    for key, wanted, pre, ref in (("dx1", w1, pre1, dx_ref[:, :c1]), ("dx2", w2, pre2, dx_ref[:, c1:]), ("dgamma", wg, pre_g, dgamma_ref),
                                  ("dbeta", wg, pre_b, dbeta_ref)):
        got = bufs[key].get()
        if wanted:
            whole = dx_ref if key.startswith("dx") else ref          # dx1 | dx2 are the two halves of one tensor
            assert _err(f"dm3d_bn_act_bwd {key}", got.astype(np.float64) - pre, ref, scale=float(np.abs(whole).max())) < LAYER_TOL
        else:
            assert np.array_equal(got, pre), f"{key} was not wanted"
    for key in ("g", "x1", "scale", "shift", "mean", "rstd"):
        bufs[key].get()                                              # inputs' padding


# ---- dm3d_batchnorm_finalize -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [
    dict(name="moving_unbiased", batch=2, voxels=37, c=20, moving=True, unbiased=1),
    dict(name="moving_biased", batch=2, voxels=37, c=20, moving=True, unbiased=0),
    dict(name="no_moving", batch=3, voxels=5, c=300, moving=False, unbiased=1),
    dict(name="one_value", batch=1, voxels=1, c=8, moving=True, unbiased=1),
    dict(name="constant_input", batch=2, voxels=50, c=12, moving=True, unbiased=1, constant=3.0),
], ids=lambda c: c["name"])
def test_batchnorm_finalize(dev, case):
    rng = np.random.default_rng(3)
    B, V, c, eps, mom = case["batch"], case["voxels"], case["c"], 1e-3, 0.9
    x = np.full((B, V, c), case["constant"], np.float32) if "constant" in case else _f32(rng, B, V, c, mean=0.4, std=1.3)
    acc_h = rk.moments_acc(_t64(x))
    gamma, beta, mm, mv = _f32(rng, c, mean=1, std=0.2), _f32(rng, c), _f32(rng, c), np.abs(_f32(rng, c)) + 0.1
    ref = rk.batchnorm_finalize(acc_h, V, eps, _t64(gamma), _t64(beta), _t64(mm) if case["moving"] else None, _t64(mv), mom, case["unbiased"])
    acc = Buf(acc_h.numpy(), dev)
    outs = [Buf(_f32(rng, c), dev) for _ in range(4)]
    bg, bb, bmm, bmv = Buf(gamma, dev), Buf(beta, dev), Buf(mm, dev), Buf(mv, dev)
    _call("dm3d_batchnorm_finalize", acc.ptr, B, V, c, eps, bg.ptr, bb.ptr, *(o.ptr for o in outs), bmm.ptr if case["moving"] else None,
          bmv.ptr if case["moving"] else None, mom, case["unbiased"])
    for o, r, what in zip(outs, ref, ("scale", "shift", "mean", "rstd")):
        assert _err(f"dm3d_batchnorm_finalize {what}", o.get(), r.numpy()) < LAYER_TOL
    if case["moving"]:
        assert _err("dm3d_batchnorm_finalize moving", bmm.get(), ref[4].numpy()) < LAYER_TOL
        assert _err("dm3d_batchnorm_finalize moving", bmv.get(), ref[5].numpy()) < LAYER_TOL
    else:
        assert np.array_equal(bmm.get(), mm) and np.array_equal(bmv.get(), mv)
    if "constant" in case:                                           # variance clamps at 0: rstd = eps^-1/2
        assert np.allclose(outs[3].get(), eps ** -0.5, rtol=1e-6, atol=0)
    if B * V == 1:                                                   # no Bessel factor: the variance fed to the moving average is 0
        assert np.allclose(bmv.get(), mv * np.float32(mom), rtol=1e-6, atol=0)
    assert not acc.get().any(), "acc must be zero again"
    bg.get(), bb.get()


# ---- GroupNormalization: stats -> finalize, partials -> finalize2 ------------------------------------------------------------------------
GN_CASES = [
    # batch, voxels, c1, c2, groups
    (2, 1, 4, 0, 1), (2, 7, 4, 0, 4),
    (2, 7, 20, 0, 4), (3, 321, 12, 8, 20), (2, 70, 20, 12, 4),          # group widths 5 and 8; 20 | 12: group 2 straddles the inputs
    (2, 70, 36, 0, 4), (1, 70, 36, 0, 36), (2, 200, 16, 20, 1),
    (2, 3000, 100, 0, 4), (1, 999, 60, 40, 1),                            # width 25: 47 slots x 25 channels > 1024 pairs per group
    (2, _rows_with_an_idle_block(256, 16, 64), 256, 0, 64), (1, 3000, 128, 128, 4),
    (2, _rows_with_an_idle_block(1028, 16, 64), 1028, 0, 4), (2, 1, 1028, 0, 1), (1, 500, 1028, 0, 4),
    (2, 7, 2048, 0, 64), (1, 400, 1024, 1024, 1), (1, 65, 2048, 0, 64),
]


def _random_gn_cases(n, seed):
    rng = np.random.default_rng(seed)
    cases = []
    for _ in range(n):
        c1, c2 = int(rng.integers(1, 40)) * 4, int(rng.integers(0, 20)) * 4
        divs = [g for g in range(1, 65) if (c1 + c2) % g == 0]
        cases.append((int(rng.integers(1, 4)), int(rng.integers(1, 700)), c1, c2, int(rng.choice(divs))))
    return cases


@pytest.mark.parametrize("B,V,c1,c2,groups", GN_CASES + _random_gn_cases(10, 20260202))
def test_groupnorm_chains(dev, B, V, c1, c2, groups):
    from dm3d_amd import _lib
    rng = np.random.default_rng(B * 131 + V + c1)
    c, eps = c1 + c2, 1e-3
    x = _f32(rng, B, V, c, mean=0.3, std=1.2)
    gamma, beta = _f32(rng, c, mean=1, std=0.3), _f32(rng, c, std=0.5)
    ref = [t.numpy() for t in rk.groupnorm_scale_shift(_t64(x), groups, eps, _t64(gamma), _t64(beta))]
    # float32 sequential moments on the CPU, finished in float64 like the kernels do
    acc32 = np.stack([np.stack([_cumsum32(x[b]), _cumsum32(x[b] * x[b])], -1) for b in range(B)])
    m = acc32.reshape(B, groups, c // groups, 2).astype(np.float64).sum(2) / (V * (c // groups))
    rstd = 1 / np.sqrt(np.maximum(m[..., 1] - m[..., 0] ** 2, 0) + eps)
    sc32 = gamma * np.repeat(rstd, c // groups, 1)
    assert np.abs(sc32 - ref[0]).max() / np.abs(ref[0]).max() < LAYER_TOL / 2
    assert np.abs(beta - np.repeat(m[..., 0], c // groups, 1) * sc32 - ref[1]).max() / np.abs(ref[1]).max() < LAYER_TOL / 2

    x1, x2 = np.ascontiguousarray(x[..., :c1]), np.ascontiguousarray(x[..., c1:])
    b1, b2 = Buf(x1, dev), (Buf(x2, dev) if c2 else None)
    bg, bb = Buf(gamma, dev), Buf(beta, dev)
    acc = Buf(np.zeros((B, c, 2), np.float64), dev)
    _call("dm3d_groupnorm_stats", b1.ptr, B, V, c1, acc.ptr, c, 0)
    if c2:
        _call("dm3d_groupnorm_stats", b2.ptr, B, V, c2, acc.ptr, c, c1)
    moments = acc.get().copy()
    mref = rk.moments_acc(_t64(x)).numpy()
    assert _err("dm3d_groupnorm_stats", moments[..., 0], mref[..., 0]) < LAYER_TOL
    assert _err("dm3d_groupnorm_stats", moments[..., 1], mref[..., 1]) < LAYER_TOL
    scale, shift = Buf(_f32(rng, B, c), dev), Buf(_f32(rng, B, c), dev)
    _call("dm3d_groupnorm_finalize", acc.ptr, B, V, c, groups, eps, bg.ptr, bb.ptr, scale.ptr, shift.ptr)
    chain1 = scale.get().copy(), shift.get().copy()
    assert _err("dm3d_groupnorm_finalize scale", chain1[0], ref[0]) < LAYER_TOL
    assert _err("dm3d_groupnorm_finalize shift", chain1[1], ref[1]) < LAYER_TOL
    assert not acc.get().any(), "acc must be zero again"

    slots = -(-V // 64)
    lib = _lib.lib()
    assert lib.dm3d_groupnorm_partials_bytes(B, V, c1) == B * slots * c1 * 8
    p1 = Buf(_f32(rng, B, slots, c1, 2), dev)
    p2 = Buf(_f32(rng, B, slots, c2, 2), dev) if c2 else None
    _call("dm3d_groupnorm_partials", b1.ptr, B, V, c1, p1.ptr)
    if c2:
        _call("dm3d_groupnorm_partials", b2.ptr, B, V, c2, p2.ptr)
    pref = rk.groupnorm_partials(_t64(x1)).numpy()
    assert _err("dm3d_groupnorm_partials", p1.get(), pref) < LAYER_TOL
    scale2, shift2 = Buf(_f32(rng, B, c), dev), Buf(_f32(rng, B, c), dev)
    _call("dm3d_groupnorm_finalize2", p1.ptr, c1, p2.ptr if c2 else None, c2, B, V, groups, eps, bg.ptr, bb.ptr, scale2.ptr, shift2.ptr)
    assert _err("dm3d_groupnorm_finalize2 scale", scale2.get(), ref[0]) < LAYER_TOL
    assert _err("dm3d_groupnorm_finalize2 shift", shift2.get(), ref[1]) < LAYER_TOL
    assert _err("groupnorm chains against each other", scale2.get(), chain1[0]) < LAYER_TOL
    assert _err("groupnorm chains against each other", shift2.get(), chain1[1], scale=float(np.abs(ref[1]).max())) < LAYER_TOL
    b1.get(), bg.get(), bb.get()


# ---- dm3d_affine_act_batched, dm3d_affine_act_cat ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,rows,c,act", [(3, 7, 20, SILU), (2, 1, 4, RELU), (2, 1031, 36, SILU), (4, 65, 1028, NONE), (2, 300, 100, RELU),
                                           (1, 2 ** 17 + 3, 8, SILU)])     # the last: past the 256-block cap of one sample
def test_affine_act_batched(dev, B, rows, c, act):
    rng = np.random.default_rng(rows + c)
    x, scale, shift = _f32(rng, B, rows, c, std=2), _f32(rng, B, c, mean=1, std=0.5), _f32(rng, B, c)
    assert B == 1 or not np.array_equal(scale[0], scale[1])
    ref = rk.affine_act_batched(_t64(x), _t64(scale), _t64(shift), act).numpy()
    bx, bs, bh, y = Buf(x, dev), Buf(scale, dev), Buf(shift, dev), Buf(_f32(rng, B, rows, c), dev)
    _call("dm3d_affine_act_batched", bx.ptr, y.ptr, B, rows, c, bs.ptr, bh.ptr, act)
    assert _err("dm3d_affine_act_batched", y.get(), ref) < ELEM_TOL
    assert np.array_equal(bx.get(), x)


@pytest.mark.parametrize("rows,c1,c2,act,affine", [(7, 20, 0, SILU, True), (1031, 12, 24, RELU, True), (65, 1028, 4, NONE, True), (3, 4, 2044, SILU, True),
                                                   (1031, 12, 24, NONE, False), (77, 36, 0, NONE, False), (5, 4, 4, RELU, False),
                                                   (2 ** 18 + 5, 8, 12, SILU, True)])      # the last: past the 4096-block cap
def test_affine_act_cat(dev, rows, c1, c2, act, affine):
    rng = np.random.default_rng(rows + c1)
    c = c1 + c2
    x1, x2 = _f32(rng, rows, c1, std=2), _f32(rng, rows, max(c2, 1), std=2)
    scale, shift = _f32(rng, c, mean=1, std=0.5), _f32(rng, c)
    b1, b2, bs, bh, y = Buf(x1, dev), Buf(x2, dev), Buf(scale, dev), Buf(shift, dev), Buf(_f32(rng, rows, c), dev)
    _call("dm3d_affine_act_cat", b1.ptr, c1, b2.ptr if c2 else None, c2, rows, bs.ptr if affine else None, bh.ptr if affine else None, act, y.ptr)
    cat = np.concatenate([x1, x2], 1) if c2 else x1
    if not affine and act == NONE:
        assert np.array_equal(y.get(), cat)                          # scale NULL: a bitwise copy / concatenation
        WORST.setdefault("dm3d_affine_act_cat (scale NULL, bitwise)", 0.0)
        return
    ref = rk.affine_act_cat(_t64(cat), None, _t64(scale) if affine else None, _t64(shift) if affine else None, act).numpy()
    assert _err("dm3d_affine_act_cat", y.get(), ref) < ELEM_TOL


# ---- dm3d_layernorm_bwd, dm3d_softmax_bwd -----------------------------------------------------------------------------------------------
LN_CASES = [(rows, c) for c in (4, 36, 256, 260, 1024) for rows in (1, 3, 5)] + [(4099, 4), (4099, 36), (4099, 256), (4099, 260), (4100, 1024)]


def _random_ln_cases(n, seed):
    rng = np.random.default_rng(seed)
    return [(int(rng.integers(1, 600)), int(rng.integers(1, 257)) * 4) for _ in range(n)]


@pytest.mark.parametrize("rows,c", LN_CASES + _random_ln_cases(8, 20260203))
def test_layernorm_bwd(dev, rows, c):
    rng = np.random.default_rng(rows * 3 + c)
    x, dy, gamma = _f32(rng, rows, c, mean=0.5, std=2), _f32(rng, rows, c), _f32(rng, c, mean=1, std=0.3)
    pre_x, pre_g, pre_b = _f32(rng, rows, c), _f32(rng, c), _f32(rng, c)
    ref = [t.numpy() for t in rk.layernorm_bwd(_t64(x), _t64(gamma), _t64(dy), 1e-3)]
    bx, bdy, bg, dx, dg, db = (Buf(v, dev) for v in (x, dy, gamma, pre_x, pre_g, pre_b))
    _call("dm3d_layernorm_bwd", bx.ptr, rows, c, 1e-3, bg.ptr, bdy.ptr, dx.ptr, dg.ptr, db.ptr)
    assert _err("dm3d_layernorm_bwd dx", dx.get().astype(np.float64) - pre_x, ref[0]) < ROW_TOL
    assert _err("dm3d_layernorm_bwd dgamma", dg.get().astype(np.float64) - pre_g, ref[1]) < ROW_TOL
    assert _err("dm3d_layernorm_bwd dbeta", db.get().astype(np.float64) - pre_b, ref[2]) < ROW_TOL
    assert np.array_equal(bx.get(), x) and np.array_equal(bdy.get(), dy)


@pytest.mark.parametrize("rows,cols,ld", [(7, 1, 1), (1, 7, 7), (13, 7, 12), (5, 64, 64), (6, 64, 70), (13, 100, 100), (3, 100, 133), (7, 512, 512),
                                          (2, 512, 516), (1030, 65, 67), (9, 1000, 1001)])
def test_softmax_bwd(dev, rows, cols, ld):
    rng = np.random.default_rng(rows + cols + ld)
    scale = 0.125
    logits = _f32(rng, rows, cols, std=3)
    p = torch.softmax(torch.from_numpy(logits) * scale, -1).numpy()
    pm, dpm = _f32(rng, rows, ld), _f32(rng, rows, ld)
    pm[:, :cols] = p
    ref = rk.softmax_bwd(_t64(pm[:, :cols]), _t64(dpm[:, :cols]), scale).numpy()
    bp, bdp = Buf(pm, dev), Buf(dpm, dev)
    _call("dm3d_softmax_bwd", bp.ptr, bdp.ptr, rows, cols, ld, scale)
    got = bdp.get()
    assert _err("dm3d_softmax_bwd", got[:, :cols], ref, scale=float(np.abs(ref).max()) or 1.0) < ROW_TOL
    assert np.array_equal(got[:, cols:], dpm[:, cols:]) and np.array_equal(bp.get(), pm)


# ---- elementwise: dm3d_act_bwd, dm3d_axpy, dm3d_fill, dm3d_adam, dm3d_mse_loss_grad ------------------------------------------------------
CAP4 = 4096 * 256                        # float4s one pass of the 4096-block elementwise grids covers


@pytest.mark.parametrize("n,act,alias", [(4, SILU, False), (1028, RELU, False), (1028, SILU, True), (40, NONE, True), (4 * 257, SILU, False),
                                          (4 * (CAP4 + 301), SILU, True)])
def test_act_bwd(dev, n, act, alias):
    rng = np.random.default_rng(n % 1000 + act)
    ref_in, dy = _f32(rng, n, std=3), _f32(rng, n)
    if act == RELU:
        ref_in[:8] = [0.0, -0.0, 1e-30, -1e-30, 1, -1, 0, 2]
    ref = rk.act_bwd(_t64(ref_in), _t64(dy), act).numpy()
    br, bdy = Buf(ref_in, dev), Buf(dy, dev)
    bdx = bdy if alias else Buf(_f32(rng, n), dev)
    _call("dm3d_act_bwd", br.ptr, bdy.ptr, bdx.ptr, n // 4 * 4, act)
    assert _err("dm3d_act_bwd", bdx.get(), ref) < ELEM_TOL
    assert np.array_equal(br.get(), ref_in) and (alias or np.array_equal(bdy.get(), dy))


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 6, 7, 1023, 1025, 4 * 256 + 2, 4 * (CAP4 + 77) + 3])
def test_axpy_and_fill(dev, n):
    rng = np.random.default_rng(n % 1000)
    dst, src, alpha = _f32(rng, n), _f32(rng, n), np.float32(-0.37)
    bd, bs = Buf(dst, dev), Buf(src, dev)
    _call("dm3d_axpy", bd.ptr, bs.ptr, n, float(alpha))
    assert _err("dm3d_axpy", bd.get(), dst.astype(np.float64) + float(alpha) * src.astype(np.float64)) < ELEM_TOL
    assert np.array_equal(bs.get(), src)
    _call("dm3d_fill", bd.ptr, n, 2.5)
    assert np.array_equal(bd.get(), np.full(n, 2.5, np.float32))
    WORST.setdefault("dm3d_fill (bitwise)", 0.0)


@pytest.mark.parametrize("n", [1, 3, 5, 1001, 4096 * 256 + 1001])      # the last: past the cap of the per-element grid
def test_adam_three_steps(dev, n):
    rng = np.random.default_rng(n % 1000)
    b1, b2, eps, lr = np.float32(0.9), np.float32(0.999), np.float32(1e-7), 0.5
    w0 = _f32(rng, n, std=0.1)
    bw, bm, bv = Buf(w0, dev), Buf(np.zeros(n, np.float32), dev), Buf(np.zeros(n, np.float32), dev)
    w, m, v = _t64(w0), torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for t in range(1, 4):
        g = _f32(rng, n)
        lr_t = np.float32(lr * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t))
        bg = Buf(g, dev)
        _call("dm3d_adam", bw.ptr, bg.ptr, bm.ptr, bv.ptr, n, float(lr_t), float(b1), float(b2), float(eps))
        w, m, v = rk.adam(w, _t64(g), m, v, float(lr_t), float(b1), float(b2), float(eps))
        assert _err("dm3d_adam m", bm.get(), m.numpy()) < ELEM_TOL
        assert _err("dm3d_adam v", bv.get(), v.numpy()) < ELEM_TOL
        assert _err("dm3d_adam step", bw.get().astype(np.float64) - w0, (w - _t64(w0)).numpy()) < ELEM_TOL
        assert np.array_equal(bg.get(), g)


@pytest.mark.parametrize("n,with_dpred", [(4, True), (1028, True), (1028, False), (4 * (1024 * 256 + 99), True), (4 * (1024 * 256 + 99), False)])
def test_mse_loss_grad(dev, n, with_dpred):
    rng = np.random.default_rng(n % 1000)
    pred, noise, inv, loss0 = _f32(rng, n), _f32(rng, n), 1.0 / 4096.0 / 3.0, 0.7071
    d = (pred - noise).astype(np.float32)                            # the float32 difference the kernel forms
    ref_loss = loss0 + float(np.sum(d.astype(np.float64) ** 2)) * inv
    bp, bn, bl, bd = Buf(pred, dev), Buf(noise, dev), Buf(np.array([loss0]), dev), Buf(_f32(rng, n), dev)
    before = bd.get().copy()
    _call("dm3d_mse_loss_grad", bp.ptr, bn.ptr, n, inv, bl.ptr, bd.ptr if with_dpred else None)
    rel = abs(float(bl.get()[0]) - ref_loss) / ref_loss
    WORST["dm3d_mse_loss_grad loss"] = max(WORST.get("dm3d_mse_loss_grad loss", 0.0), rel)
    print(f"dm3d_mse_loss_grad loss: {rel:.2e} (bound {n * 2.0 ** -53:.2e})")
    assert rel <= n * 2.0 ** -53
    if with_dpred:
        assert _err("dm3d_mse_loss_grad dpred", bd.get(), 2 * (pred.astype(np.float64) - noise) * inv) < ELEM_TOL
    else:
        assert np.array_equal(bd.get(), before)


# ---- data movement: bitwise ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,cols,ld_src,ld_dst,batch", [(1, 1, 1, 1, 1), (32, 32, 32, 32, 1), (33, 31, 31, 33, 2), (5, 70, 75, 9, 3), (100, 3, 3, 100, 1),
                                                           (65, 64, 64, 70, 2), (31, 97, 100, 40, 2)])
def test_transpose(dev, rows, cols, ld_src, ld_dst, batch):
    rng = np.random.default_rng(rows + cols)
    ss, sd = rows * ld_src + 5, cols * ld_dst + 3                   # batch strides larger than the matrices
    src, pre = _f32(rng, batch, ss), _f32(rng, batch, sd)
    bs, bd = Buf(src, dev), Buf(pre, dev)
    _call("dm3d_transpose", bs.ptr, rows, cols, ld_src, ss, bd.ptr, ld_dst, sd, batch)
    exp = pre.copy()
    for b in range(batch):
        m = src[b, :rows * ld_src].reshape(rows, ld_src)[:, :cols]
        exp[b, :cols * ld_dst].reshape(cols, ld_dst)[:, :rows] = m.T
    assert np.array_equal(bd.get(), exp) and np.array_equal(bs.get(), src)
    WORST.setdefault("dm3d_transpose (bitwise)", 0.0)


@pytest.mark.parametrize("rows,c,ld_src,src_off,ld_dst,dst_off,acc", [(1, 4, 4, 0, 4, 0, 0), (7, 20, 36, 8, 24, 4, 0), (7, 20, 36, 8, 24, 4, 1),
                                                                    (1031, 12, 12, 0, 40, 28, 1), (130, 1028, 1032, 4, 1028, 0, 0),
                                                                    (2 ** 18 + 3, 16, 20, 4, 16, 0, 1)])
def test_copy_cols(dev, rows, c, ld_src, src_off, ld_dst, dst_off, acc):
    rng = np.random.default_rng(rows + c)
    src, pre = _f32(rng, rows, ld_src), _f32(rng, rows, ld_dst)
    bs, bd = Buf(src, dev), Buf(pre, dev)
    _call("dm3d_copy_cols", bs.ptr, ld_src, src_off, bd.ptr, ld_dst, dst_off, rows, c, acc)
    exp = pre.copy()
    win = src[:, src_off:src_off + c]
    exp[:, dst_off:dst_off + c] = win + pre[:, dst_off:dst_off + c] if acc else win
    assert np.array_equal(bd.get(), exp)
    WORST.setdefault("dm3d_copy_cols (bitwise)", 0.0)


@pytest.mark.parametrize("B,size,c", [(1, (1, 1, 1), 4), (2, (1, 3, 2), 12), (2, (3, 1, 5), 20), (3, (2, 5, 1), 36), (1, (4, 3, 5), 100), (2, (5, 6, 7), 8),
                                      (1, (33, 32, 32), 16)])           # the last: the upsampled side is past the 4096-block cap
def test_upsample2_and_sumpool2_add(dev, B, size, c):
    rng = np.random.default_rng(sum(size) + c)
    D, H, W = size
    x, y = _f32(rng, B, D, H, W, c), _f32(rng, B, 2 * D, 2 * H, 2 * W, c)
    bx, up = Buf(x, dev), Buf(_f32(rng, B, 2 * D, 2 * H, 2 * W, c), dev)
    _call("dm3d_upsample2", bx.ptr, up.ptr, B, D, H, W, c)
    assert np.array_equal(up.get(), rk.upsample2(x))
    by, pooled = Buf(y, dev), Buf(x, dev)                            # accumulates into non-zero values
    _call("dm3d_sumpool2_add", by.ptr, pooled.ptr, B, D, H, W, c)
    assert np.array_equal(pooled.get(), rk.sumpool2_add(x, y))       # float32, the children added one at a time in index order
    assert np.array_equal(bx.get(), x) and np.array_equal(by.get(), y)
    WORST.setdefault("dm3d_upsample2 / dm3d_sumpool2_add (bitwise)", 0.0)


DILATE_CASES = [(2, inp, off, 8) for inp in ((5, 7, 6), (4, 4, 4), (1, 3, 1)) for off in itertools.product((0, 1), repeat=3)] + \
               [(1, (9, 1, 5), (1, 0, 1), 36), (3, (2, 2, 3), (0, 1, 0), 4)]


@pytest.mark.parametrize("B,inp,off,c", DILATE_CASES)
def test_dilate2(dev, B, inp, off, c):
    rng = np.random.default_rng(sum(inp) + sum(off))
    out = tuple(-(-n // 2) for n in inp)                             # the extent of a stride-2 "same" convolution's output
    src = _f32(rng, B, *out, c)
    src[src == 0] = 1
    bs, bd = Buf(src, dev), Buf(_f32(rng, B, *inp, c), dev)
    _call("dm3d_dilate2", bs.ptr, bd.ptr, B, *out, *inp, *off, c)
    assert np.array_equal(bd.get(), rk.dilate2(src, inp, off)) and np.array_equal(bs.get(), src)
    WORST.setdefault("dm3d_dilate2 (bitwise)", 0.0)


@pytest.mark.parametrize("taps,cin,cout", [(1, 4, 4), (1, 33, 7), (27, 5, 3), (27, 36, 68), (8, 1, 9), (27, 200, 200)])
def test_flip_transpose(dev, taps, cin, cout):
    rng = np.random.default_rng(taps + cin)
    w = _f32(rng, taps, cin, cout)
    bw, bo = Buf(w, dev), Buf(_f32(rng, taps, cout, cin), dev)
    _call("dm3d_flip_transpose", bw.ptr, taps, cin, cout, bo.ptr)
    assert np.array_equal(bo.get(), rk.flip_transpose(w)) and np.array_equal(bw.get(), w)
    WORST.setdefault("dm3d_flip_transpose (bitwise)", 0.0)


@pytest.mark.parametrize("B,per", [(1, 4), (3, 1028), (2, 4 * 257), (4, 36), (2, 4 * (256 * 256 + 9))])     # the last: past the 256-block cap
def test_q_sample(dev, B, per):
    rng = np.random.default_rng(per % 1000)
    T = 7
    lat, noise = _f32(rng, B, per), _f32(rng, B, per)
    sqab, sq1ab = rng.random(T).astype(np.float32), rng.random(T).astype(np.float32)
    t = np.array([-3, T + 5, 2, T - 1][:B], np.int32)                # out-of-range timesteps are clamped to the table
    bl, bn, bt, ba, bs = Buf(lat, dev), Buf(noise, dev), Buf(t, dev), Buf(sqab, dev), Buf(sq1ab, dev)
    out = Buf(_f32(rng, B, per), dev)
    _call("dm3d_q_sample", bl.ptr, bn.ptr, bt.ptr, ba.ptr, bs.ptr, T, out.ptr, B, per)
    assert np.array_equal(out.get(), rk.q_sample_f32(lat, noise, t, sqab, sq1ab))
    WORST.setdefault("dm3d_q_sample (bitwise)", 0.0)


# ---- indexed rows, counters, the range guard ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,c,table_rows", [(6, 5, 4), (40, 3, 7), (300, 20, 11), (64, 129, 5)])
def test_scatter_add_rows(dev, rows, c, table_rows):
    rng = np.random.default_rng(rows + c)
    src, table = _f32(rng, rows, c), _f32(rng, table_rows, c)
    idx = rng.integers(0, table_rows, rows).astype(np.int32)         # far more rows than table rows: duplicates
    idx[:4] = [-1, table_rows, 2 ** 31 - 1, -2 ** 31]                # ignored
    idx[4:6] = 1
    bs, bi, bt = Buf(src, dev), Buf(idx, dev), Buf(table, dev)
    _call("dm3d_scatter_add_rows", bs.ptr, bi.ptr, rows, c, bt.ptr, table_rows)
    ref = rk.scatter_add_rows(_t64(table), idx, _t64(src)).numpy()
    assert _err("dm3d_scatter_add_rows", bt.get(), ref) < ELEM_TOL * max(1, rows // table_rows)    # float atomics: one rounding per added row
    assert np.array_equal(bi.get(), idx)


@pytest.mark.parametrize("rows,c,table_rows", [(5, 4, 3), (70, 36, 9), (1000, 260, 2)])
def test_gather_rows(dev, rows, c, table_rows):
    rng = np.random.default_rng(rows + c)
    table = _f32(rng, table_rows, c)
    idx = rng.integers(0, table_rows, rows).astype(np.int32)
    idx[:4] = [-1, table_rows, 2 ** 31 - 1, -2 ** 31]                # clamped to the first / last row
    bt, bi, out = Buf(table, dev), Buf(idx, dev), Buf(_f32(rng, rows, c), dev)
    _call("dm3d_gather_rows", bt.ptr, table_rows, bi.ptr, out.ptr, rows, c)
    assert np.array_equal(out.get(), rk.gather_rows(table, idx))
    WORST.setdefault("dm3d_gather_rows (bitwise)", 0.0)


def test_add_i32_saturates_at_zero(dev):
    p = np.array([5, 1, 0, 3, 1000] * 30, np.int32)                  # 150 counters: three blocks of 64
    bp = Buf(p, dev)
    _call("dm3d_add_i32", bp.ptr, p.size, -1)
    assert np.array_equal(bp.get(), np.maximum(p - 1, 0))
    _call("dm3d_add_i32", bp.ptr, p.size - 1, -3)
    exp = np.maximum(np.maximum(p - 1, 0) - 3, 0)
    exp[-1] = p[-1] - 1                                              # outside n
    assert np.array_equal(bp.get(), exp)
    _call("dm3d_add_i32", bp.ptr, p.size, 2)
    assert np.array_equal(bp.get(), exp + 2)
    WORST.setdefault("dm3d_add_i32 (exact)", 0.0)


def test_range_check(dev):
    rng = np.random.default_rng(0)
    limit = np.float32(100.0)
    n = 4 * (2048 * 256 + 53)                                        # past the 2048-block cap
    base = np.clip(_f32(rng, n, std=20), -99, 99)

    def flag_after(x, n_=None, start=0):
        bx, bf = Buf(x, dev), Buf(np.array([start], np.int32), dev)
        _call("dm3d_range_check", bx.ptr, x.size if n_ is None else n_, float(limit), bf.ptr)
        return int(bf.get()[0])

    assert flag_after(base) == 0
    assert flag_after(base, start=1) == 1                            # a set flag is not cleared
    edge = base.copy()
    edge[[0, 77, -1]] = [limit, -limit, limit]
    assert flag_after(edge) == 0                                     # |x| == limit is inside the range
    for bad in (np.nan, np.inf, -np.inf, np.nextafter(limit, np.float32(np.inf)), -np.float32(101)):
        x = base.copy()
        x[-1] = bad                                                  # the only offender: the very last element
        assert flag_after(x) == 1, bad
        small = base[:8].copy()
        small[5] = bad
        assert flag_after(small) == 1, bad
        assert flag_after(small, n_=4) == 0                          # beyond n: not looked at
    WORST.setdefault("dm3d_range_check (exact)", 0.0)
