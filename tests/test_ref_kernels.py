"""CPU tier of the kernel-by-kernel training tests.

1. oracle/ref_kernels.py against itself: every closed-form backward equals torch.autograd on the float64 forward to 1e-12 relative,
   and upsample2 / sumpool2 are adjoint.  These are the references tests/test_gpu_train_kernels.py holds the HIP kernels against.
2. Every training and normalisation entry of the C ABI refuses each documented bad argument with DM3D_EINVAL and a message, before
   any launch (fake aligned non-null pointers: nothing is ever dereferenced, so no GPU is needed).
3. The sampler restatements of oracle/ref_kernels.py against independent statements: the paper forms in lambda / h of the GPU sampler
   tests, np.quantile, the textbook guidance formula, autograd; and their float32 order within 1e-6 of their float64 one.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import ref_kernels as rk

TOL = 1e-12


def _rel(a, ref):
    a, ref = torch.as_tensor(a).double(), torch.as_tensor(ref).double()
    assert a.shape == ref.shape, (a.shape, ref.shape)
    return float((a - ref).abs().max() / ref.abs().max().clamp_min(1e-300))


def _rnd(seed, *shape):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


@pytest.mark.parametrize("kind", [rk.ACT_NONE, rk.ACT_RELU, rk.ACT_SILU])
def test_act_bwd_closed_form_is_autograd(kind):
    u, dy = _rnd(0, 37, 12) * 3, _rnd(1, 37, 12)
    assert _rel(rk.act_bwd(u, dy, kind), rk.act_bwd_autograd(u, dy, kind)) < TOL


@pytest.mark.parametrize("kind", [rk.ACT_NONE, rk.ACT_RELU, rk.ACT_SILU])
def test_bn_act_bwd_closed_form_is_autograd(kind):
    x, g = _rnd(2, 3 * 35, 20) * 1.5 + 0.3, _rnd(3, 3 * 35, 20)
    gamma, beta, eps = _rnd(4, 20) * 0.2 + 1, _rnd(5, 20) * 0.3, 1e-3
    scale, shift, mean, rstd = rk.batchnorm_finalize(rk.moments_acc(x.reshape(3, 35, 20)), 35, eps, gamma, beta)
    assert _rel(rk.affine_act_cat(x[:, :12], x[:, 12:], scale, shift, kind), rk.bn_act_fwd(x, gamma, beta, eps, kind)) < TOL
    dx, dgamma, dbeta, red = rk.bn_act_bwd(g, x, scale, shift, mean, rstd, kind)
    rx, rg, rb = rk.bn_act_bwd_autograd(g, x, gamma, beta, eps, kind)
    assert _rel(dx, rx) < TOL and _rel(dgamma, rg) < TOL and _rel(dbeta, rb) < TOL
    assert torch.equal(red[:, 0], dbeta) and torch.equal(red[:, 1], dgamma)


def test_batchnorm_finalize_moving_averages_and_edges():
    x = _rnd(6, 2, 9, 8) + 0.5
    gamma, beta = _rnd(7, 8), _rnd(8, 8)
    mm, mv = _rnd(9, 8), _rnd(10, 8).abs()
    flat = x.reshape(-1, 8)
    for unbiased in (0, 1):
        scale, shift, mean, rstd, nmm, nmv = rk.batchnorm_finalize(rk.moments_acc(x), 9, 1e-3, gamma, beta, mm, mv, 0.99, unbiased)
        assert _rel(mean, flat.mean(0)) < TOL and _rel(rstd, 1 / torch.sqrt(flat.var(0, unbiased=False) + 1e-3)) < TOL
        assert _rel(nmm, 0.99 * mm + 0.01 * flat.mean(0)) < TOL
        assert _rel(nmv, 0.99 * mv + 0.01 * flat.var(0, unbiased=bool(unbiased))) < 1e-11
    one = _rnd(11, 1, 1, 4)                                         # batch*voxels == 1: no Bessel factor, variance 0
    out = rk.batchnorm_finalize(rk.moments_acc(one), 1, 1e-3, torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64),
                                torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64), 0.5, 1)
    assert torch.isfinite(out[5]).all() and _rel(out[3], torch.full((4,), 1e-3 ** -0.5, dtype=torch.float64)) < 1e-9


@pytest.mark.parametrize("groups", [1, 4, 5, 20])
def test_groupnorm_scale_shift_is_group_norm(groups):
    x = _rnd(12, 3, 70, 20) * 2 + 0.4
    gamma, beta = _rnd(13, 20), _rnd(14, 20)
    scale, shift = rk.groupnorm_scale_shift(x, groups, 1e-3, gamma, beta)
    ref = torch.nn.functional.group_norm(x.permute(0, 2, 1), groups, gamma, beta, 1e-3).permute(0, 2, 1)
    assert _rel(rk.affine_act_batched(x, scale, shift, rk.ACT_NONE), ref) < 1e-11
    part = rk.groupnorm_partials(x)                                 # 70 voxels: two slots, the second of 6
    assert part.shape == (3, 2, 20, 2) and _rel(part.sum(1), rk.moments_acc(x)) < TOL


@pytest.mark.parametrize("ksize,size", [(3, (3, 4, 5)), (3, (1, 4, 1)), (1, (2, 3, 2))])
def test_wgrad_closed_form_is_autograd(ksize, size):
    a, g = _rnd(15, 2, *size, 8), _rnd(16, 2, *size, 12)
    assert _rel(rk.wgrad(a, g, ksize), rk.wgrad_autograd(a, g, ksize)) < TOL


def test_colsum_and_flip_transpose_are_the_gradients_they_stand_for():
    x = _rnd(17, 3 * 11, 8)
    assert _rel(rk.colsum(x, 3), rk.colsum_autograd(x, 3)) < TOL
    for k in (1, 3):
        w, xin, g = _rnd(18, k, k, k, 4, 8), _rnd(19, 2, 3, 4, 5, 4), _rnd(20, 2, 3, 4, 5, 8)
        wf = torch.from_numpy(rk.flip_transpose(w.reshape(k ** 3, 4, 8).numpy())).reshape(k, k, k, 8, 4)
        assert _rel(rk._conv_same(g, wf), rk.conv_dgrad_autograd(xin, w, g)) < TOL


@pytest.mark.parametrize("rows,c", [(1, 4), (5, 36), (3, 260)])
def test_layernorm_bwd_closed_form_is_autograd(rows, c):
    x, dy, gamma = _rnd(21, rows, c) * 2 + 0.5, _rnd(22, rows, c), _rnd(23, c) * 0.3 + 1
    for a, r in zip(rk.layernorm_bwd(x, gamma, dy, 1e-3), rk.layernorm_bwd_autograd(x, gamma, dy, 1e-3)):
        assert _rel(a, r) < TOL


@pytest.mark.parametrize("cols", [1, 7, 100])
def test_softmax_bwd_closed_form_is_autograd(cols):
    logits, dp = _rnd(24, 6, cols) * 3, _rnd(25, 6, cols)
    p, ref = rk.softmax_bwd_autograd(logits, dp, 0.25)
    got = rk.softmax_bwd(p, dp, 0.25)
    assert float((got - ref).abs().max()) <= TOL * max(float(ref.abs().max()), 1.0)     # cols == 1: both are exactly 0


def test_upsample2_and_sumpool2_are_adjoint():
    x, y = _rnd(26, 2, 3, 1, 5, 4), _rnd(27, 2, 6, 2, 10, 4)
    pooled = rk.sumpool2_add(torch.zeros_like(x), y)
    lhs, rhs = float((rk.upsample2(x) * y).sum()), float((x * pooled).sum())
    assert abs(lhs - rhs) <= TOL * abs(lhs)
    assert _rel(pooled, rk.sumpool2_autograd(y)) < TOL
    assert np.array_equal(rk.upsample2(x.numpy()), rk.upsample2(x).numpy())


def test_dilate2_scatter_gather_q_sample_references():
    src = np.arange(2 * 3 * 2 * 3 * 4, dtype=np.float32).reshape(2, 3, 2, 3, 4) + 1
    d = rk.dilate2(src, (5, 4, 6), (1, 0, 1))                       # z: 2*2+1 = 5 falls outside an extent of 5
    assert d.shape == (2, 5, 4, 6, 4) and np.array_equal(d[:, 1:5:2, 0:4:2, 1:6:2], src[:, :2])
    assert np.count_nonzero(d) == src[:, :2].size
    table, s = _rnd(28, 5, 3), _rnd(29, 4, 3)
    idx = np.array([2, 2, -1, 5])
    out = rk.scatter_add_rows(table, idx, s)
    assert torch.equal(out[2], table[2] + s[0] + s[1]) and torch.equal(out[[0, 1, 3, 4]], table[[0, 1, 3, 4]])
    assert np.array_equal(rk.gather_rows(table.numpy(), idx), table.numpy()[[2, 2, 0, 4]])
    lat, z = np.ones((3, 8), np.float32), np.full((3, 8), 2, np.float32)
    q = rk.q_sample_f32(lat, z, np.array([-4, 1, 9]), np.array([.5, .25], np.float32), np.array([.1, .2], np.float32))
    assert q.dtype == np.float32 and np.array_equal(q[:, 0], np.float32([.5, .25, .25]) + np.float32(2) * np.float32([.1, .2, .2]))


def test_mse_and_adam_references():
    pred, noise = _rnd(30, 64), _rnd(31, 64)
    l, gr = rk.mse_loss_grad(pred, noise, 1 / 48.0)
    rl, rg = rk.mse_loss_grad_autograd(pred, noise, 1 / 48.0)
    assert abs(float(l - rl)) <= TOL * float(rl) and _rel(gr, rg) < TOL
    w, g = _rnd(32, 50), _rnd(33, 50)
    wt = w.clone().requires_grad_(True)
    opt = torch.optim.Adam([wt], lr=1e-2, betas=(0.9, 0.999), eps=0.0)
    m = v = torch.zeros_like(w)
    for t in range(1, 4):
        wt.grad = g * t
        opt.step()
        w, m, v = rk.adam(w, g * t, m, v, 1e-2 * np.sqrt(1 - 0.999 ** t) / (1 - 0.9 ** t), 0.9, 0.999, 0.0)
        assert _rel(w, wt.detach()) < 1e-11


# ---- argument validation ------------------------------------------------------------------------------------------------------------
P, U = 0x1000, 0x1004            # a fake 16-byte aligned device pointer and a misaligned one: refused calls never dereference them

# entry -> ordered (name, valid value); names starting with "*" are required pointers, "^" pointers the kernels read as float4 (must
# be aligned), "?" optional pointers that must be aligned when given
ENTRIES = {
    "dm3d_colsum": [("^x", P), ("groups", 2), ("rows", 8), ("c", 8), ("*out", P), ("ld_out", 8)],
    "dm3d_bn_act_bwd": [("^g", P), ("^x1", P), ("c1", 8), ("?x2", P), ("c2", 4), ("rows", 8), ("^scale", P), ("^shift", P), ("^mean", P),
                        ("^rstd", P), ("act", 2), ("*red", P), ("?dx1", P), ("?dx2", P), ("dgamma", P), ("dbeta", P)],
    "dm3d_batchnorm_finalize": [("*acc", P), ("batch", 2), ("voxels", 8), ("c", 8), ("eps", 1e-3), ("*gamma", P), ("*beta", P), ("*scale", P),
                                ("*shift", P), ("*mean_out", P), ("*rstd_out", P), ("moving_mean", P), ("moving_var", P), ("momentum", 0.99),
                                ("unbiased", 1)],
    "dm3d_affine_act_cat": [("^x1", P), ("c1", 8), ("?x2", P), ("c2", 4), ("rows", 8), ("?scale", P), ("?shift", P), ("act", 2), ("^y", P)],
    "dm3d_flip_transpose": [("*w", P), ("taps", 27), ("cin", 4), ("cout", 8), ("*out", 0x2000)],
    "dm3d_layernorm_bwd": [("^x", P), ("rows", 8), ("c", 8), ("eps", 1e-3), ("^gamma", P), ("^dy", P), ("^dx", P), ("*dgamma", P), ("*dbeta", P)],
    "dm3d_softmax_bwd": [("*p", P), ("*dp", P), ("rows", 8), ("cols", 8), ("ld", 8), ("scale", 1.0)],
    "dm3d_act_bwd": [("^ref", P), ("^dy", P), ("^dx", P), ("n", 8), ("act", 2)],
    "dm3d_axpy": [("^dst", P), ("^src", P), ("n", 8), ("alpha", 1.0)],
    "dm3d_fill": [("^dst", P), ("n", 8), ("value", 1.0)],
    "dm3d_transpose": [("*src", P), ("rows", 8), ("cols", 8), ("ld_src", 8), ("stride_src", 64), ("*dst", P), ("ld_dst", 8), ("stride_dst", 64),
                       ("batch", 2)],
    "dm3d_copy_cols": [("^src", P), ("ld_src", 16), ("src_off", 4), ("^dst", P), ("ld_dst", 16), ("dst_off", 4), ("rows", 8), ("c", 8),
                       ("accumulate", 1)],
    "dm3d_upsample2": [("^src", P), ("^dst", P), ("batch", 2), ("d", 2), ("h", 2), ("w", 2), ("c", 8)],
    "dm3d_sumpool2_add": [("^src", P), ("^dst", P), ("batch", 2), ("d", 2), ("h", 2), ("w", 2), ("c", 8)],
    "dm3d_dilate2": [("^src", P), ("^dst", P), ("batch", 2), ("od", 2), ("oh", 2), ("ow", 2), ("id", 4), ("ih", 4), ("iw", 4), ("offz", 0),
                     ("offy", 1), ("offx", 0), ("c", 8)],
    "dm3d_scatter_add_rows": [("*src", P), ("*idx", P), ("rows", 8), ("c", 8), ("*table", P), ("table_rows", 8)],
    "dm3d_q_sample": [("^latents", P), ("^noise", P), ("*t", P), ("*sqab", P), ("*sq1ab", P), ("timesteps", 8), ("^out", P), ("batch", 2),
                      ("per_sample", 8)],
    "dm3d_mse_loss_grad": [("^pred", P), ("^noise", P), ("n", 8), ("inv", 0.5), ("*loss", P), ("?dpred", P)],
    "dm3d_adam": [("*w", P), ("*g", P), ("*m", P), ("*v", P), ("n", 8), ("lr_t", 1e-3), ("b1", 0.9), ("b2", 0.999), ("eps", 1e-7)],
    "dm3d_groupnorm_stats": [("^x", P), ("batch", 2), ("voxels", 8), ("c", 8), ("*acc", P), ("c_total", 16), ("chan_off", 4)],
    "dm3d_groupnorm_finalize": [("*acc", P), ("batch", 2), ("voxels", 8), ("c_total", 8), ("groups", 4), ("eps", 1e-3), ("*gamma", P), ("*beta", P),
                                ("*scale", P), ("*shift", P)],
    "dm3d_groupnorm_partials": [("*x", P), ("batch", 2), ("voxels", 8), ("c", 8), ("*part", P)],
    "dm3d_groupnorm_finalize2": [("*part1", P), ("c1", 8), ("part2", P), ("c2", 4), ("batch", 2), ("voxels", 8), ("groups", 4), ("eps", 1e-3),
                                 ("*gamma", P), ("*beta", P), ("*scale", P), ("*shift", P)],
    "dm3d_affine_act_batched": [("^x", P), ("^y", P), ("batch", 2), ("rows", 8), ("c", 8), ("^scale", P), ("^shift", P), ("act", 2)],
    "dm3d_range_check": [("^x", P), ("n", 8), ("limit", 1.0), ("*flag", P)],
    "dm3d_gather_rows": [("^table", P), ("table_rows", 8), ("*idx", P), ("^out", P), ("rows", 8), ("c", 8)],
    "dm3d_add_i32": [("*p", P), ("n", 8), ("delta", -1)],
}

# every other documented precondition: (entry, overrides of the valid call, what is wrong)
BAD = [
    ("dm3d_colsum", dict(c=6), "c % 4"), ("dm3d_colsum", dict(ld_out=4), "ld_out < c"), ("dm3d_colsum", dict(groups=0), "no groups"),
    ("dm3d_colsum", dict(groups=65536), "groups > 65535"), ("dm3d_colsum", dict(rows=0), "no rows"), ("dm3d_colsum", dict(c=0), "c == 0"),
    ("dm3d_bn_act_bwd", dict(c1=6), "c1 % 4"), ("dm3d_bn_act_bwd", dict(c2=6), "c2 % 4"), ("dm3d_bn_act_bwd", dict(x2=0), "c2 without x2"),
    ("dm3d_bn_act_bwd", dict(c2=0), "x2 without c2"), ("dm3d_bn_act_bwd", dict(rows=0), "no rows"), ("dm3d_bn_act_bwd", dict(act=3), "act"),
    ("dm3d_bn_act_bwd", dict(dbeta=0), "dgamma without dbeta"), ("dm3d_bn_act_bwd", dict(dgamma=0), "dbeta without dgamma"),
    ("dm3d_bn_act_bwd", dict(dbeta=0, dx1=0, dx2=0), "dgamma without dbeta, no dx"),
    ("dm3d_batchnorm_finalize", dict(moving_var=0), "moving_mean without moving_var"),
    ("dm3d_batchnorm_finalize", dict(moving_mean=0), "moving_var without moving_mean"),
    ("dm3d_batchnorm_finalize", dict(batch=0), "batch"), ("dm3d_batchnorm_finalize", dict(voxels=0), "voxels"),
    ("dm3d_batchnorm_finalize", dict(c=0), "c"),
    ("dm3d_affine_act_cat", dict(c1=6), "c1 % 4"), ("dm3d_affine_act_cat", dict(c2=6), "c2 % 4"), ("dm3d_affine_act_cat", dict(x2=0), "c2 without x2"),
    ("dm3d_affine_act_cat", dict(c2=0), "x2 without c2"), ("dm3d_affine_act_cat", dict(rows=0), "rows"), ("dm3d_affine_act_cat", dict(act=-1), "act"),
    ("dm3d_affine_act_cat", dict(shift=0), "scale without shift"), ("dm3d_affine_act_cat", dict(scale=0), "shift without scale"),
    ("dm3d_flip_transpose", dict(taps=0), "taps"), ("dm3d_flip_transpose", dict(cin=0), "cin"), ("dm3d_flip_transpose", dict(out=P), "in place"),
    ("dm3d_layernorm_bwd", dict(c=6), "c % 4"), ("dm3d_layernorm_bwd", dict(c=1028), "c > 1024"), ("dm3d_layernorm_bwd", dict(rows=0), "rows"),
    ("dm3d_softmax_bwd", dict(ld=4), "ld < cols"), ("dm3d_softmax_bwd", dict(rows=0), "rows"), ("dm3d_softmax_bwd", dict(cols=0), "cols"),
    ("dm3d_act_bwd", dict(n=6), "n % 4"), ("dm3d_act_bwd", dict(n=0), "n"), ("dm3d_act_bwd", dict(act=3), "act"),
    ("dm3d_axpy", dict(n=0), "n"), ("dm3d_fill", dict(n=0), "n"),
    ("dm3d_transpose", dict(ld_src=4), "ld_src < cols"), ("dm3d_transpose", dict(ld_dst=4), "ld_dst < rows"), ("dm3d_transpose", dict(rows=0), "rows"),
    ("dm3d_transpose", dict(cols=0), "cols"), ("dm3d_transpose", dict(batch=0), "batch"), ("dm3d_transpose", dict(batch=65536), "batch > 65535"),
    ("dm3d_copy_cols", dict(c=6), "c % 4"), ("dm3d_copy_cols", dict(src_off=2), "src_off % 4"), ("dm3d_copy_cols", dict(dst_off=2), "dst_off % 4"),
    ("dm3d_copy_cols", dict(ld_src=18), "ld_src % 4"), ("dm3d_copy_cols", dict(ld_dst=18), "ld_dst % 4"), ("dm3d_copy_cols", dict(ld_src=8), "ld_src < off + c"),
    ("dm3d_copy_cols", dict(ld_dst=8), "ld_dst < off + c"), ("dm3d_copy_cols", dict(src_off=-4), "src_off < 0"), ("dm3d_copy_cols", dict(rows=0), "rows"),
    ("dm3d_upsample2", dict(c=6), "c % 4"), ("dm3d_upsample2", dict(d=0), "d"), ("dm3d_upsample2", dict(batch=0), "batch"),
    ("dm3d_sumpool2_add", dict(c=6), "c % 4"), ("dm3d_sumpool2_add", dict(w=0), "w"), ("dm3d_sumpool2_add", dict(batch=0), "batch"),
    ("dm3d_dilate2", dict(c=6), "c % 4"), ("dm3d_dilate2", dict(offz=2), "offz"), ("dm3d_dilate2", dict(offy=-1), "offy"), ("dm3d_dilate2", dict(offx=2), "offx"),
    ("dm3d_dilate2", dict(offz=-1), "offz"), ("dm3d_dilate2", dict(offy=2), "offy"), ("dm3d_dilate2", dict(offx=-1), "offx"),
    ("dm3d_dilate2", dict(od=0), "od"), ("dm3d_dilate2", dict(id=0), "id"), ("dm3d_dilate2", dict(batch=0), "batch"),
    ("dm3d_scatter_add_rows", dict(rows=0), "rows"), ("dm3d_scatter_add_rows", dict(c=0), "c"), ("dm3d_scatter_add_rows", dict(table_rows=0), "table_rows"),
    ("dm3d_q_sample", dict(per_sample=6), "per_sample % 4"), ("dm3d_q_sample", dict(timesteps=0), "timesteps"), ("dm3d_q_sample", dict(batch=0), "batch"),
    ("dm3d_q_sample", dict(batch=65536), "batch > 65535"),
    ("dm3d_mse_loss_grad", dict(n=6), "n % 4"), ("dm3d_mse_loss_grad", dict(n=0), "n"),
    ("dm3d_adam", dict(n=0), "n"),
    ("dm3d_groupnorm_stats", dict(c=6), "c % 4"), ("dm3d_groupnorm_stats", dict(chan_off=2), "chan_off % 4"),
    ("dm3d_groupnorm_stats", dict(chan_off=12), "window outside c_total"), ("dm3d_groupnorm_stats", dict(chan_off=-4), "chan_off < 0"),
    ("dm3d_groupnorm_stats", dict(batch=0), "batch"), ("dm3d_groupnorm_stats", dict(voxels=0), "voxels"),
    ("dm3d_groupnorm_finalize", dict(groups=3), "groups does not divide c"), ("dm3d_groupnorm_finalize", dict(groups=0), "groups"),
    ("dm3d_groupnorm_finalize", dict(c_total=256, groups=128), "groups > 64"), ("dm3d_groupnorm_finalize", dict(c_total=0), "c_total"),
    ("dm3d_groupnorm_finalize", dict(batch=0), "batch"), ("dm3d_groupnorm_finalize", dict(voxels=0), "voxels"),
    ("dm3d_groupnorm_partials", dict(batch=0), "batch"), ("dm3d_groupnorm_partials", dict(voxels=0), "voxels"), ("dm3d_groupnorm_partials", dict(c=0), "c"),
    ("dm3d_groupnorm_finalize2", dict(groups=5), "groups does not divide c1 + c2"), ("dm3d_groupnorm_finalize2", dict(part2=0), "c2 without part2"),
    ("dm3d_groupnorm_finalize2", dict(c2=0), "part2 without c2"), ("dm3d_groupnorm_finalize2", dict(c1=0), "c1"),
    ("dm3d_groupnorm_finalize2", dict(groups=0), "groups"), ("dm3d_groupnorm_finalize2", dict(batch=0), "batch"),
    ("dm3d_affine_act_batched", dict(c=6), "c % 4"), ("dm3d_affine_act_batched", dict(act=3), "act"), ("dm3d_affine_act_batched", dict(batch=0), "batch"),
    ("dm3d_affine_act_batched", dict(rows=0), "rows"),
    ("dm3d_range_check", dict(n=6), "n % 4"), ("dm3d_range_check", dict(n=0), "n"),
    ("dm3d_gather_rows", dict(c=6), "c % 4"), ("dm3d_gather_rows", dict(table_rows=0), "table_rows"), ("dm3d_gather_rows", dict(rows=0), "rows"),
    ("dm3d_add_i32", dict(n=0), "n"),
]

WGRAD_OK = dict(a=P, g=P, dw=P, batch=2, in_d=2, in_h=2, in_w=2, cin=8, cout=8, ksize=3, per_item_output=0, stride_a=0, stride_g=0, stride_dw=0)
WGRAD_BAD = [
    (dict(a=0), "a null"), (dict(g=0), "g null"), (dict(dw=0), "dw null"), (dict(a=U), "a unaligned"), (dict(g=U), "g unaligned"),
    (dict(ksize=2), "ksize 2"), (dict(ksize=0), "ksize 0"), (dict(ksize=5), "ksize 5"), (dict(cin=6), "cin % 4"), (dict(cout=6), "cout % 4"),
    (dict(cin=0), "cin"), (dict(batch=0), "batch"), (dict(in_d=0), "in_d"), (dict(in_h=0), "in_h"), (dict(in_w=0), "in_w"),
    (dict(per_item_output=1, stride_a=64, stride_g=64, stride_dw=64), "per_item_output with ksize 3"),
    (dict(ksize=1, per_item_output=1, stride_a=66, stride_g=64, stride_dw=64), "per-item a not 16-byte aligned"),
    (dict(ksize=1, per_item_output=1, stride_a=64, stride_g=66, stride_dw=64), "per-item g not 16-byte aligned"),
]


def _bad_calls():
    calls = []
    for entry, params in ENTRIES.items():
        for name, _ in params:
            if name[0] in "*^":
                calls.append((entry, {name[1:]: 0}, f"{name[1:]} null"))
            if name[0] in "^?":
                calls.append((entry, {name[1:]: U}, f"{name[1:]} unaligned"))
    return calls + BAD


def test_training_entries_refuse_bad_arguments(built_library):
    """Every documented precondition of the training and normalisation entries is checked before anything is launched: DM3D_EINVAL
    and a message, with no GPU in the machine."""
    from dm3d_amd import _lib
    lib = _lib.lib()
    seen, failures = set(), []
    for entry, override, what in _bad_calls():
        params = ENTRIES[entry]
        names = [n.lstrip("*^?") for n, _ in params]
        assert set(override) <= set(names), (entry, override)
        assert len(params) + 1 == len(_lib.SIGNATURES[entry][1]), entry
        args = [override.get(n, v) for n, (_, v) in zip(names, params)]
        lib.dm3d_fill(None, 0, 0.0, None)                           # leaves a known message behind
        stale = lib.dm3d_last_error()
        rc = getattr(lib, entry)(*args, None)
        msg = lib.dm3d_last_error()
        if rc != -1 or not msg or msg == stale and entry != "dm3d_fill":
            failures.append(f"{entry}({what}): rc {rc}, message {msg!r}")
        seen.add(entry)
    for override, what in WGRAD_BAD:
        d = _lib.WgradDesc()
        for k, v in {**WGRAD_OK, **override}.items():
            setattr(d, k, v)
        rc = lib.dm3d_wgrad(C.byref(d), None)
        if rc != -1 or b"wgrad" not in lib.dm3d_last_error():
            failures.append(f"dm3d_wgrad({what}): rc {rc}, message {lib.dm3d_last_error()!r}")
    if lib.dm3d_wgrad(None, None) != -1:
        failures.append("dm3d_wgrad(NULL)")
    assert not failures, "\n".join(failures)
    assert seen == set(ENTRIES)
    assert lib.dm3d_groupnorm_partials_bytes(0, 8, 8) == 0 and lib.dm3d_groupnorm_partials_bytes(3, 65, 20) == 3 * 2 * 20 * 8


# ---- 3. the sampler restatements (oracle/ref_kernels.py, last section) against independent statements ----------------------------------
# The folded-row forms at order="f64" against the paper forms in lambda / h that the GPU sampler tests carry, with schedules' tables
# (handed over unrounded, in float64, so that the comparison is of the formulas alone); x0_bound against np.quantile; guide_update
# against the textbook lines; and order="f32" within 1e-6 of order="f64" on O(1) inputs.
T_S, SCHED = 1000, [0, 250, 500, 749, 999]
F64_TOL = 1e-11


def _ab():
    import dm3d_amd
    return np.asarray(dm3d_amd.Betas(T_S).alpha_bar, np.float64)


def _steps():
    """src, dst, prev of a 5-step chain, one row per step: the first step first order, the last one to clean."""
    src = SCHED[::-1]
    return src, src[1:] + [-1], [-1] + src[:-1]


def _xs(seed, B, n=64, k=4):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((B, n)) for _ in range(k)]


@pytest.mark.parametrize("clip", [True, False])
def test_dpm_update_f64_is_the_paper_form(clip):
    from dm3d_amd import schedules
    from chain_reference import dpm64
    ab = _ab()
    src, dst, prev = _steps()
    coef = np.zeros((5, 8))
    coef[:, :2] = schedules.ddim_coefficients(ab, src, dst)[:, :2]
    coef[:, 2:5] = schedules.dpm_coefficients(ab, src, dst, prev)
    coef[:, 5] = float(clip)
    x, e, h, _ = _xs(1, 5)
    res, x0 = rk.dpm_update(x, e, coef, np.arange(5), h, order="f64")
    for b in range(5):
        ref, ref0 = dpm64(torch.from_numpy(x[b]), torch.from_numpy(e[b]), ab, src[b], dst[b], prev[b] if dst[b] >= 0 else -1, torch.from_numpy(h[b]), clip)
        assert _rel(res[b], ref) < F64_TOL and _rel(x0[b], ref0) < F64_TOL, b
    assert coef[0, 4] == 0 and coef[1, 4] != 0 and coef[4, 4] == 0           # first order, second order, to clean
    # without a history the add of c_1*hist is skipped, whatever c_1 holds: the paper's first-order step on the rows that are first order
    first, _ = rk.dpm_update(x, e, coef, np.arange(5), None, order="f64")
    for b in (0, 4):
        ref, _ = dpm64(torch.from_numpy(x[b]), torch.from_numpy(e[b]), ab, src[b], dst[b], -1, None, clip)
        assert _rel(first[b], ref) < F64_TOL, b
    assert _rel(first, coef[:, 2:3] * x + coef[:, 3:4] * x0) < F64_TOL


@pytest.mark.parametrize("eta", [0.5, 1.0])
def test_dpm_sde_update_f64_is_the_paper_form(eta):
    from dm3d_amd import schedules
    from chain_reference import dpm64
    ab = _ab()
    src, dst, prev = _steps()
    coef = np.zeros((5, 8))
    coef[:, :2] = schedules.ddim_coefficients(ab, src, dst)[:, :2]
    rows = schedules.dpm_sde_coefficients(ab, src, dst, prev, 2, eta)
    coef[:, 2:5], coef[:, 6], coef[:, 5] = rows[:, :3], rows[:, 3], 1.0
    x, e, h, z = _xs(2, 5)
    res, x0 = rk.dpm_sde_update(x, e, coef, np.arange(5), h, z, order="f64")
    for b in range(5):
        ref, ref0 = dpm64(torch.from_numpy(x[b]), torch.from_numpy(e[b]), ab, src[b], dst[b], prev[b] if dst[b] >= 0 else -1,
                          torch.from_numpy(h[b]), eta=eta, z=torch.from_numpy(z[b]))
        assert _rel(res[b], ref) < F64_TOL and _rel(x0[b], ref0) < F64_TOL, b
    assert coef[0, 6] != 0 and coef[4, 6] == 0                               # the row to clean draws nothing
    # c_z = 0 everywhere: dpm_update's result
    ode = coef.copy()
    ode[:, 6] = 0
    a, b = rk.dpm_sde_update(x, e, ode, np.arange(5), h, z), rk.dpm_update(x, e, ode, np.arange(5), h)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[0].dtype == np.float32


@pytest.mark.parametrize("eta", [0.0, 0.7])
def test_ddim_update_f64_is_the_paper_form(eta):
    from dm3d_amd import schedules
    from chain_reference import ddim64
    ab = _ab()
    src, dst, _ = _steps()
    coef = np.zeros((5, 8))
    coef[:, :5] = schedules.ddim_coefficients(ab, src, dst, eta)
    coef[:, 5] = 1.0
    x, e, z, _ = _xs(3, 5)
    res = rk.ddim_update(x, e, coef, np.arange(5), z, order="f64")
    for b in range(5):
        ref = ddim64(torch.from_numpy(x[b]), torch.from_numpy(e[b]), ab[src[b]], ab[dst[b]] if dst[b] >= 0 else 1.0, eta, torch.from_numpy(z[b]))
        assert _rel(res[b], ref) < F64_TOL, b


@pytest.mark.parametrize("kind", ["v", "x0"])
def test_frame_rows_give_the_eps_frames_estimate(kind):
    """x0 and eps from a frame row of schedules.frame_table equal the eps-frame estimate of the eps that prediction stands for."""
    from dm3d_amd import schedules
    ab = _ab()
    t = np.array([3, 400, 998])
    a, s = np.sqrt(ab[t])[:, None], np.sqrt(1 - ab[t])[:, None]
    x0_true, z = _xs(4, 3, k=2)
    x = a * x0_true + s * z
    pred = a * z - s * x0_true if kind == "v" else x0_true
    frame = schedules.frame_table(ab.astype(np.float32), kind).astype(np.float64)
    coef = np.zeros((T_S, 8))
    coef[:, 0], coef[:, 1] = np.sqrt(ab), np.sqrt(1 - ab)
    x0, eps = rk.x0_estimate(x, pred, coef, t, frame, order="f64")
    assert np.abs(x0 - x0_true).max() < 1e-5 and np.abs(eps - z).max() < 1e-5       # (the table is rounded to float32)
    x0_e, _ = rk.x0_estimate(x, z, coef, t, None, order="f64")
    assert np.abs(x0_e - x0_true).max() < 1e-9


def test_x0_bound_is_the_linear_quantile():
    rng = np.random.default_rng(5)
    B, n = 4, 1004
    x, e = rng.standard_normal((B, n)) * 2, rng.standard_normal((B, n))
    coef = np.zeros((2, 8))
    coef[:, 0], coef[:, 1], coef[0, 5] = 0.8, 0.6, 1.0
    from dm3d_amd import schedules
    p = [1e-9, 0.37, 0.995, 1.0]
    rank, frac, smax = schedules.threshold_tables(B, n, p, 1e9)
    got = rk.x0_bound(x, e, coef, [0] * B, rank, frac, smax, order="f64")
    for b in range(B):
        q = float(np.quantile(np.abs((x[b] - 0.6 * e[b]) / 0.8), p[b], method="linear"))
        assert abs(got[b] - max(q, 1.0)) < 1e-6 * max(q, 1.0), (b, got[b], q)     # frac is a float32
    assert got[0] == 1.0 and got[3] > 3.0
    assert np.array_equal(rk.x0_bound(x, e, coef, [0, 1, 0, 5], rank, frac, np.full(B, 2.5, np.float32), order="f64") == 1.0, [True, True, False, True])
    assert rk.x0_bound(x, e, coef, [0] * B, rank, frac, np.full(B, 2.5, np.float32))[3] == np.float32(2.5)
    # a NaN sorts last: it reaches the bound only from the top rank
    x[1, 7] = np.nan
    top = rk.x0_bound(x, e, coef, [0] * B, [n - 1] * B, [0.0] * B, smax)
    assert np.isnan(top[1]) and np.isfinite(top[[0, 2, 3]]).all()
    assert np.isfinite(rk.x0_bound(x, e, coef, [0] * B, [n - 3] * B, [0.5] * B, smax)).all()


def test_guide_update_is_the_textbook_formula():
    ep, en = (v + 0.5 for v in _xs(6, 4, 1004, 2))
    w, phi = np.array([7.5, -1.0, 0.0, 1.0]), np.array([0.7, 0.0, 1.0, 0.3])
    g, f, out = rk.guide_update(ep, en, w, phi, order="f64")
    for b in range(4):
        gb = en[b] + w[b] * (ep[b] - en[b])
        fb = phi[b] * ep[b].std() / gb.std() + (1 - phi[b])
        assert np.abs(g[b] - gb).max() < 1e-12 and abs(f[b] - fb) < 1e-12 and np.abs(out[b] - fb * gb).max() < 1e-11
    assert np.array_equal(g[2], en[2]) and np.array_equal(g[3], ep[3]) and f[1] == 1.0 and np.array_equal(out[1], g[1])
    flat = np.full_like(en, 0.25)
    assert rk.guide_update(ep, flat, np.zeros(4), np.ones(4), order="f64")[1].tolist() == [1.0] * 4     # std(eps_g) == 0


def test_edit_pred_and_loss_restatements():
    x0, z, x, p = _xs(7, 3, 24)
    levels = np.array([[0.6, 0.8, 5, 0], [1.0, 0.0, -1, 0], [0.3, 0.9, 7, 0]])
    known = rk.edit_update(x0, levels, [0, 1, 9], z, order="f64")
    assert np.abs(known[0] - (0.6 * x0[0] + 0.8 * z[0])).max() < 1e-15 and np.array_equal(known[1], x0[1])
    assert np.abs(known[2] - (0.3 * x0[2] + 0.9 * z[2])).max() < 1e-15
    w = np.tile(np.array([0.0, 1.0, 0.25, 0.5]), (3, 1))                     # 4 voxels of 6 channels
    got = rk.edit_update(x0, levels, [0, 1, 2], z, 1, x, w, 6, order="f64").reshape(3, 4, 6)
    k3, x3 = known.reshape(3, 4, 6), x.reshape(3, 4, 6)
    assert np.array_equal(got[:, 0], x3[:, 0]) and np.array_equal(got[:, 1], k3[:, 1])
    assert np.abs(got[:, 2] - (0.25 * k3[:, 2] + 0.75 * x3[:, 2])).max() < 1e-15
    table = np.array([[0.5, 2.0], [-1.5, 0.25]])
    eps = rk.pred_to_eps(p, x, table, [-4, 1, 6], order="f64")
    assert np.abs(eps[0] - (0.5 * p[0] + 2.0 * x[0])).max() < 1e-15 and np.abs(eps[2] - (-1.5 * p[2] + 0.25 * x[2])).max() < 1e-15
    coef = np.array([[1, 0, 1, 0], [0.6, -0.8, 0.5, 0], [0, 1, 2.0, 0]], np.float64)
    inv = 1.0 / 48
    dpred, rows, loss = rk.objective_loss(p, z, x0, coef, inv, order="f64")
    pt, tgt = torch.from_numpy(p).requires_grad_(True), torch.from_numpy(coef[:, :1] * z + coef[:, 1:2] * x0)
    per = (torch.from_numpy(coef[:, 2]) * inv * ((pt - tgt) ** 2).sum(1))
    per.sum().backward()
    assert _rel(dpred, pt.grad) < TOL and _rel(rows, per.detach()) < TOL and abs(loss - float(per.detach().sum())) < 1e-12 * loss
    assert rk.objective_loss(p, z, x0, coef, inv, want_dpred=False)[0] is None


def test_f32_orders_stay_within_1e6_of_f64():
    rng = np.random.default_rng(8)
    B, n = 4, 1004
    x, e, h, z = (rng.standard_normal((B, n)).astype(np.float32) for _ in range(4))
    coef = (rng.uniform(0.5, 1.5, (B, 8)) * rng.choice([-1, 1], (B, 8))).astype(np.float32)
    coef[:, 0] = np.abs(coef[:, 0])
    coef[1, 5] = coef[2, 4] = coef[3, 6] = 0
    frame = rng.uniform(-1, 1, (B, 4)).astype(np.float32)
    pos, bound = np.arange(B), np.array([1.0, 1.3, 2.0, 1.1], np.float32)
    worst = 0.0
    for fr in (None, frame):
        for bd in (None, bound):
            pairs = [(rk.ddim_update(x, e, coef, pos, z, fr, bd, order=o),) + rk.dpm_update(x, e, coef, pos, h, fr, bd, order=o)
                     + rk.dpm_sde_update(x, e, coef, pos, h, z, fr, bd, order=o) for o in ("f32", "f64")]
            for a, b in zip(*pairs):
                assert a.dtype == np.float32 and b.dtype == np.float64
                worst = max(worst, float(np.abs(a - b).max() / max(1.0, np.abs(b).max())))
    levels = np.array([[0.6, 0.8, 5, 0], [1.0, 0.0, -1, 0], [0.3, 0.9, 7, 0], [0.9, 0.4, 2, 0]], np.float32)
    w = rng.choice([0.0, 1.0, 0.3, 0.6], (B, n // 4)).astype(np.float32)
    table = rng.uniform(-1.5, 1.5, (5, 2)).astype(np.float32)
    lc = np.array([[1, 0, 1, 0], [0.6, -0.8, 0.5, 0], [0, 1, 2.0, 0], [0.3, 0.9, 0.1, 0]], np.float32)
    scale, phi = np.array([2.5, 0, 1, -0.7], np.float32), np.array([0.7, 0.2, 0, 1.0], np.float32)
    for fn in (lambda o: rk.edit_update(x, levels, pos, z, 1, e, w, 4, order=o), lambda o: rk.pred_to_eps(x, e, table, pos, order=o),
               lambda o: rk.objective_loss(x, z, e, lc, 0.01, order=o)[0], lambda o: rk.guide_update(x, e, scale, phi, order=o)[2],
               lambda o: rk.guide_update(x, e, scale, phi, order=o)[1], lambda o: rk.objective_loss(x, z, e, lc, 0.01, order=o)[1],
               lambda o: rk.x0_bound(x, e, coef, pos, [0, n // 2, n - 2, n - 1], [0.3] * B, [1e9] * B, order=o)):
        a, b = np.asarray(fn("f32"), np.float64), np.asarray(fn("f64"), np.float64)
        worst = max(worst, float(np.abs(a - b).max() / max(1.0, np.abs(b).max())))
    print(f"f32 against f64 restatements: worst {worst:.2e}")
    assert worst < 1e-6
