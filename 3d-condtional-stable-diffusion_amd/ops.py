"""Immediate-mode wrappers over the C ABI (one call = one kernel launch on the current stream).

These mirror the stock Keras / TensorFlow ops the reference's hot path executes (include/dm3d.h cites each one).  They
validate shapes in Python (``ValueError``, like the reference's only explicit check, conditional_dm3d.py:343-346) and then
call the HIP kernels; there is no fallback implementation.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import NamedTuple, Optional

import torch

from . import _lib
from ._lib import ACT_NONE, ConvDesc, DdpmDesc, GemmDesc, check, lib


def _st() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]):
    return None if t is None else t.data_ptr()


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
        raise ValueError(f"{name} must be a contiguous float32 device tensor")
    return t


def pack_weights(kernel: torch.Tensor, in_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Keras Conv3D [kd,kh,kw,Cin,Cout] or Dense [in,out] kernel -> [taps][CoutPad][CinPad]."""
    _f32c(kernel, "kernel")
    if kernel.dim() not in (2, 5):
        raise ValueError("kernel must be [in,out] or [kd,kh,kw,cin,cout]")
    taps = 1 if kernel.dim() == 2 else kernel.shape[0] * kernel.shape[1] * kernel.shape[2]
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    out = torch.empty(lib().dm3d_packed_weight_elems(taps, cin, cout), dtype=torch.float32, device=kernel.device)
    check(lib().dm3d_pack_weights(kernel.data_ptr(), taps, cin, cout, _p(in_scale), out.data_ptr(), _st()), "pack_weights")
    return out


def h3_weight_exponent(*kernels) -> int:
    """Power-of-two pre-scale of the H3 weight images: the largest |w| of all given kernels (NumPy arrays or tensors) lands in
    [2^13, 2^14), so that hi stays finite and lo a normal float16.  Clamped to the +-100 the packers accept."""
    import math
    wmax = max(float(abs(k).max()) for k in kernels)
    if wmax == 0.0 or not math.isfinite(wmax):
        return 0
    return max(-100, min(100, 14 - math.frexp(wmax)[1]))           # frexp: wmax = m 2^e with m in [0.5, 1), i.e. floor(log2 wmax) = e - 1


def pack_weights_skip_h3p(kernel: torch.Tensor, w_exp: int) -> torch.Tensor:
    """Keras 1x1 kernel ([1,1,1,cin,cout] or [cin,cout]) -> image for conv3d(skip=...), packed with the main conv's w_exp."""
    _f32c(kernel, "kernel")
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    out = torch.empty(lib().dm3d_packed_weight_skip_h3p_bytes(cin, cout) // 2, dtype=torch.float16, device=kernel.device)
    check(lib().dm3d_pack_weights_skip_h3p(kernel.data_ptr(), cin, cout, w_exp, out.data_ptr(), _st()), "pack_weights_skip_h3p")
    return out


def pack_weights_skip_h3f(kernel: torch.Tensor, w_exp: int) -> torch.Tensor:
    """The same 1x1 kernel as MFMA operand fragments: conv3d(skip=(x1, x2, image, fragments)) lets the Winograd-x form serve the launch."""
    _f32c(kernel, "kernel")
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    out = torch.empty(lib().dm3d_packed_weight_skip_h3p_bytes(cin, cout) // 2, dtype=torch.float16, device=kernel.device)
    check(lib().dm3d_pack_weights_skip_h3f(kernel.data_ptr(), cin, cout, w_exp, out.data_ptr(), _st()), "pack_weights_skip_h3f")
    return out


def pack_weights_h3(kernel: torch.Tensor, in_scale: Optional[torch.Tensor] = None, stride: int = 1, w_exp: Optional[int] = None):
    """Keras kernel -> (float16 hi/lo image for the H3 conv kernels, w_exp).  max|w|*2^w_exp lands in [2^13, 2^14).
    ``stride`` is the stride of the conv that will read the image: it selects the layout (dm3d_conv_weight_layout)."""
    _f32c(kernel, "kernel")
    if kernel.dim() not in (2, 5):
        raise ValueError("kernel must be [in,out] or [kd,kh,kw,cin,cout]")
    taps = 1 if kernel.dim() == 2 else kernel.shape[0] * kernel.shape[1] * kernel.shape[2]
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    if w_exp is None:
        w_exp = h3_weight_exponent(kernel)
    ksize = {1: 1, 27: 3, 64: 4}.get(taps, 0)
    if ksize and lib().dm3d_conv_weight_layout(ksize, stride, 0, 0, cout) == _lib.WL_PAIR:
        out = torch.empty(lib().dm3d_packed_weight_h3p_bytes(taps, cin, cout) // 2, dtype=torch.float16, device=kernel.device)
        check(lib().dm3d_pack_weights_h3p(kernel.data_ptr(), taps, cin, cout, w_exp, _p(in_scale), out.data_ptr(), 0, _st()),
              "pack_weights_h3p")
        return out, w_exp
    out = torch.empty(lib().dm3d_packed_weight_h3_bytes(taps, cin, cout) // 2, dtype=torch.float16, device=kernel.device)
    check(lib().dm3d_pack_weights_h3(kernel.data_ptr(), taps, cin, cout, w_exp, _p(in_scale), out.data_ptr(), _st()),
          "pack_weights_h3")
    return out, w_exp


def pack_weights_h3w(kernel: torch.Tensor, w_exp: int, in_scale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Weight image of a k3 / stride-1 conv ([3,3,3,cin,cout]) for the Winograd-x form (conv3d(wpk_wino=...)): the x taps of every
    (dz, dy, cin, cout) become the four F(2,3) terms; packed with the w_exp of the conv's main image."""
    _f32c(kernel, "kernel")
    if kernel.dim() != 5 or tuple(kernel.shape[:3]) != (3, 3, 3):
        raise ValueError("kernel must be [3,3,3,cin,cout]")
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    out = torch.empty(lib().dm3d_packed_weight_h3w_bytes(cin, cout) // 2, dtype=torch.float16, device=kernel.device)
    check(lib().dm3d_pack_weights_h3w(kernel.data_ptr(), cin, cout, w_exp, _p(in_scale), out.data_ptr(), _st()), "pack_weights_h3w")
    return out


def pack_weights_up(kernel: torch.Tensor, h3: bool = False, w_exp: Optional[int] = None):
    """[3,3,3,Cin,Cout] kernel of an UpSample conv -> the 8 parity images dm3d_conv3d_ndhwc(upsample=1) expects.
    Returns wpk (fp32) or (wpk, w_exp) (h3; ``w_exp`` defaults to the exponent of the parity sums)."""
    _f32c(kernel, "kernel")
    if kernel.dim() != 5 or tuple(kernel.shape[:3]) != (3, 3, 3):
        raise ValueError("kernel must be [3,3,3,cin,cout]")
    cin, cout = kernel.shape[-2], kernel.shape[-1]
    if not h3:
        out = torch.empty(lib().dm3d_packed_weight_up_elems(cin, cout), dtype=torch.float32, device=kernel.device)
        check(lib().dm3d_pack_weights_up(kernel.data_ptr(), cin, cout, out.data_ptr(), _st()), "pack_weights_up")
        return out
    if w_exp is None:
        from .weights import upsample_parity_kernels
        w_exp = h3_weight_exponent(upsample_parity_kernels(kernel.cpu().numpy()))
    out = torch.empty(lib().dm3d_packed_weight_up_h3_bytes(cin, cout) // 2, dtype=torch.float16, device=kernel.device)
    check(lib().dm3d_pack_weights_up_h3(kernel.data_ptr(), cin, cout, w_exp, out.data_ptr(), _st()), "pack_weights_up_h3")
    return out, w_exp


def pack_weights_convt(kernel: torch.Tensor, h3: bool = False):
    """[4,4,4,Cout,Cin] kernel of Conv3DTranspose(k=4, strides=2, padding="same") -> the 8 parity images that
    dm3d_conv3d_ndhwc(transpose=1) expects.  Returns wpk (fp32) or (wpk, w_exp) (h3)."""
    _f32c(kernel, "kernel")
    if kernel.dim() != 5 or tuple(kernel.shape[:3]) != (4, 4, 4):
        raise ValueError("kernel must be [4,4,4,cout,cin]")
    cout, cin = kernel.shape[-2], kernel.shape[-1]
    if not h3:
        out = torch.empty(lib().dm3d_packed_weight_up_elems(cin, cout), dtype=torch.float32, device=kernel.device)
        check(lib().dm3d_pack_weights_convt(kernel.data_ptr(), cin, cout, out.data_ptr(), _st()), "pack_weights_convt")
        return out
    w_exp = h3_weight_exponent(kernel)
    out = torch.empty(lib().dm3d_packed_weight_up_h3_bytes(cin, cout) // 2, dtype=torch.float16, device=kernel.device)
    check(lib().dm3d_pack_weights_convt_h3(kernel.data_ptr(), cin, cout, w_exp, out.data_ptr(), _st()), "pack_weights_convt_h3")
    return out, w_exp


def conv3d(x1, wpk, cout, ksize, *, x2=None, bias=None, stride=1, upsample=False, pro_scale=None, pro_shift=None,
           vec=None, vec_idx=None, relu=False, res=None, precision=_lib.PREC_F32, w_exp=0, prelu_alpha=None,
           relu_out=False, transpose=False, skip=None, x1_h2_channels=None, out_h2=False, post=None, wpk_wino=None, gn_stats=None, split=True) -> torch.Tensor:
    """Conv3D(padding="same") on NDHWC with the fused prologue / concat / upsample / epilogue of dm3d_conv3d_ndhwc.
    ``skip=(sx1, sx2_or_None, skip_wpk[, skip_wpk_frag])``: also accumulate Conv3D(cout, 1) of the raw concat(sx1, sx2) (H3, k3, stride 1).
    ``post=(scale, shift)``: out = silu(out*scale[c] + shift[c]) at the very end; ``out_h2``: store DM3D_FMT_H2;
    ``x1_h2_channels=c``: x1 is a DM3D_FMT_H2 buffer of c logical channels (as written by ``out_h2``).
    ``split=False``: no split_counters, i.e. a small grid is not split along Cin (the A/B arm of the hand-over form)."""
    _f32c(x1, "x1")
    if x1.dim() != 5:
        raise ValueError("x1 must be [B,D,H,W,C]")
    B, D, H, W, c1 = x1.shape
    c2 = 0
    if x2 is not None:
        _f32c(x2, "x2")
        if x2.shape[:4] != x1.shape[:4]:
            raise ValueError("x2 must share x1's batch and spatial shape")
        c2 = x2.shape[4]
    up = 2 if upsample else 1
    od, oh, ow = (-(-D * up // stride), -(-H * up // stride), -(-W * up // stride))
    if transpose:
        od, oh, ow = 2 * D, 2 * H, 2 * W
    out = torch.empty(B, od, oh, ow, cout, dtype=torch.float32, device=x1.device)
    d = ConvDesc()
    d.x1, d.x2, d.c1, d.c2, d.batch = x1.data_ptr(), _p(x2), c1, c2, B
    d.in_d, d.in_h, d.in_w, d.upsample, d.ksize, d.stride = D, H, W, int(bool(upsample)), ksize, stride
    d.wpk, d.bias, d.pro_scale, d.pro_shift = wpk.data_ptr(), _p(bias), _p(pro_scale), _p(pro_shift)
    if vec is not None:
        d.vec, d.vec_idx, d.vec_ld = vec.data_ptr(), _p(vec_idx), vec.shape[-1]
    if res is not None and tuple(res.shape) != tuple(out.shape):
        raise ValueError("res must have the output's shape")
    d.relu, d.res, d.out, d.cout = int(bool(relu)), _p(res), out.data_ptr(), cout
    d.precision, d.w_exp = precision, w_exp
    if precision == _lib.PREC_H3:
        d.w_layout = lib().dm3d_conv_weight_layout(ksize, stride, int(bool(upsample)), int(bool(transpose)), cout)
    if prelu_alpha is not None and tuple(prelu_alpha.shape) != (od, oh, ow, cout):
        raise ValueError("prelu_alpha must be [out_d, out_h, out_w, cout]")
    d.prelu_alpha, d.relu_out, d.transpose = _p(prelu_alpha), int(bool(relu_out)), int(bool(transpose))
    if x1_h2_channels is not None:
        d.x1_fmt = _lib.FMT_H2
    if out_h2:
        d.out_fmt = _lib.FMT_H2
    if post is not None:
        d.post_scale, d.post_shift = post[0].data_ptr(), post[1].data_ptr()
    if wpk_wino is not None:
        d.wpk_wino = wpk_wino.data_ptr()
    if gn_stats is not None:               # float32 [B, ceil(voxels / 64), cout, 2]: partial (sum, sum of squares) of the output per (sample, channel)
        d.gn_stats = gn_stats.data_ptr()
    if skip is not None:
        sx1, sx2, swpk = skip[:3]
        if len(skip) > 3 and skip[3] is not None:
            d.skip_wpk_frag = skip[3].data_ptr()
        _f32c(sx1, "skip x1")
        d.skip_x1, d.skip_x2, d.skip_c1, d.skip_c2, d.skip_wpk = sx1.data_ptr(), _p(sx2), sx1.shape[-1], (sx2.shape[-1] if sx2 is not None else 0), swpk.data_ptr()
    # the Cin split of small grids (include/dm3d.h, split_counters): tickets (zero before, zero after) and the parts' workspace
    need, words = lib().dm3d_conv_scratch_bytes(C.byref(d)), lib().dm3d_conv_split_counter_words(C.byref(d))
    if need and split:
        scratch = torch.empty(need // 4, dtype=torch.float32, device=x1.device)     # stays alive until the launches are enqueued:
        d.scratch, d.scratch_bytes = scratch.data_ptr(), need                       # same stream, so the allocator cannot reuse it early
        counters = _split_counters(x1.device, words)
        d.split_counters, d.split_counter_words = counters.data_ptr(), counters.numel()
    check(lib().dm3d_conv3d_ndhwc(C.byref(d), _st()), "conv3d")
    return out


_COUNTERS = {}


def _split_counters(device, words: int) -> torch.Tensor:
    """One zeroed ticket buffer per device for the op-level calls (every launch leaves it zero; launches of a stream are ordered)."""
    buf = _COUNTERS.get(device)
    if buf is None or buf.numel() < words:
        buf = _COUNTERS[device] = torch.zeros(max(4096, words), dtype=torch.int32, device=device)
    return buf


def split_h2(src: torch.Tensor, exp2: int = 0) -> torch.Tensor:
    """float32 [rows, k] -> DM3D_FMT_H2 [rows, round_up(k,16)] (returned as a float32-typed buffer of the same byte size)."""
    _f32c(src, "src")
    rows, k = src.numel() // src.shape[-1], src.shape[-1]
    ld = -(-k // 16) * 16
    dst = torch.empty(rows, ld, dtype=torch.float32, device=src.device)
    check(lib().dm3d_split_h2(src.data_ptr(), rows, k, k, exp2, dst.data_ptr(), ld, _st()), "split_h2")
    return dst


def h2_to_f32(h2: torch.Tensor, k: int) -> torch.Tensor:
    """Host-side decoder of DM3D_FMT_H2 (tests only): [rows, ld] float32-typed buffer -> float32 hi + lo values."""
    rows, ld = h2.shape
    rec = h2.contiguous().view(torch.float16).reshape(rows, ld // 16, 4, 8).float()
    val = rec[:, :, 0:2, :] + rec[:, :, 2:4, :]
    return val.reshape(rows, ld)[:, :k]


def gemm_tn(a, b, *, m=None, n=None, k=None, lda=None, ldb=None, batch=1, stride_a=None, stride_b=None, alpha=1.0, bias=None,
            bias_along_m=False, act=ACT_NONE, res=None, out=None, precision=_lib.PREC_F32, a_fmt=_lib.FMT_F32,
            b_fmt=_lib.FMT_F32, out_fmt=_lib.FMT_F32) -> torch.Tensor:
    """out[b][m][n] = act(alpha * sum_k a[b][m][k] b[b][n][k] + bias) + res.  a: [batch?, m, k], b: [batch?, n, k]."""
    _f32c(a, "a"), _f32c(b, "b")
    m = a.shape[-2] if m is None else m
    k = a.shape[-1] if k is None else k
    n = b.shape[-2] if n is None else n
    lda = a.shape[-1] if lda is None else lda
    ldb = b.shape[-1] if ldb is None else ldb
    if stride_a is None:
        stride_a = a.shape[-2] * a.shape[-1] if (batch > 1 and a.dim() == 3 and a.shape[0] == batch) else 0
    if stride_b is None:
        stride_b = b.shape[-2] * b.shape[-1] if (batch > 1 and b.dim() == 3 and b.shape[0] == batch) else 0
    if out is None:
        out = torch.empty((batch, m, n) if batch > 1 else (m, n), dtype=torch.float32, device=a.device)
    d = GemmDesc()
    d.a, d.lda, d.stride_a = a.data_ptr(), lda, stride_a
    d.b, d.ldb, d.stride_b = b.data_ptr(), ldb, stride_b
    d.out, d.ldo, d.stride_o = out.data_ptr(), n, m * n
    d.m, d.n, d.k, d.batch, d.alpha = m, n, k, batch, alpha
    d.bias, d.bias_along_m, d.act = _p(bias), int(bool(bias_along_m)), act
    if res is not None:
        d.res, d.ldr, d.stride_r = res.data_ptr(), n, m * n
    d.precision, d.a_fmt, d.b_fmt, d.out_fmt = precision, a_fmt, b_fmt, out_fmt
    check(lib().dm3d_gemm_tn(C.byref(d), _st()), "gemm_tn")
    return out


def attention(q, k, vt, scale, *, res=None, precision=_lib.PREC_F32, fmt=_lib.FMT_F32) -> torch.Tensor:
    """softmax(q k^T * scale) v + res per sample through dm3d_attention.  q [B, Lq, C]; k [B or 1, Lk, C]; vt [B or 1, C, Lk]
    (the value tensor transposed); with fmt=FMT_H2 the three operands are DM3D_FMT_H2 buffers of those logical shapes."""
    B, Lq, Cc = q.shape
    Lk = k.shape[1]
    out = torch.empty(B, Lq, Cc, dtype=torch.float32, device=q.device)
    scratch = torch.empty(lib().dm3d_attention_workspace_bytes(B, Lq, Lk) // 4, dtype=torch.float32, device=q.device)
    d = _lib.AttentionDesc()
    d.q, d.ldq = q.data_ptr(), q.shape[-1]
    d.k, d.ldk, d.stride_k = k.data_ptr(), k.shape[-1], (Lk * k.shape[-1] if k.shape[0] == B and B > 1 else 0)
    d.vt, d.ldv, d.stride_vt = vt.data_ptr(), vt.shape[-1], (vt.shape[1] * vt.shape[-1] if vt.shape[0] == B and B > 1 else 0)
    d.out, d.ldo, d.res = out.data_ptr(), Cc, _p(res)
    d.batch, d.lq, d.lk, d.c, d.scale, d.precision, d.fmt = B, Lq, Lk, Cc, float(scale), precision, fmt
    check(lib().dm3d_attention(C.byref(d), scratch.data_ptr(), _st()), "attention")
    return out


def layernorm3(x, params, eps=1e-3):
    """params: up to three (gamma, beta) pairs -> list of outputs sharing one statistics pass."""
    _f32c(x, "x")
    c = x.shape[-1]
    rows = x.numel() // c
    outs = [torch.empty_like(x) for _ in params]
    args = []
    for i in range(3):
        if i < len(params):
            args += [params[i][0].data_ptr(), params[i][1].data_ptr(), outs[i].data_ptr()]
        else:
            args += [None, None, None]
    check(lib().dm3d_layernorm3(x.data_ptr(), rows, c, eps, *args, _st()), "layernorm3")
    return outs


def layernorm3_h2(x, params, eps=1e-3):
    _f32c(x, "x")
    c = x.shape[-1]
    rows = x.numel() // c
    outs = [torch.empty_like(x) for _ in params]
    args = []
    for i in range(3):
        if i < len(params):
            args += [params[i][0].data_ptr(), params[i][1].data_ptr(), outs[i].data_ptr()]
        else:
            args += [None, None, None]
    check(lib().dm3d_layernorm3_h2(x.data_ptr(), rows, c, eps, *args, _st()), "layernorm3_h2")
    return outs


def softmax_rows_h2_(s: torch.Tensor) -> torch.Tensor:
    _f32c(s, "s")
    cols = s.shape[-1]
    check(lib().dm3d_softmax_rows_h2(s.data_ptr(), s.numel() // cols, cols, cols, _st()), "softmax_rows_h2")
    return s


def softmax_rows_(s: torch.Tensor) -> torch.Tensor:
    _f32c(s, "s")
    cols = s.shape[-1]
    check(lib().dm3d_softmax_rows(s.data_ptr(), s.numel() // cols, cols, cols, _st()), "softmax_rows")
    return s


def affine_act(x, scale=None, shift=None, act=ACT_NONE) -> torch.Tensor:
    _f32c(x, "x")
    c = x.shape[-1]
    y = torch.empty_like(x)
    check(lib().dm3d_affine_act(x.data_ptr(), y.data_ptr(), x.numel() // c, c, _p(scale), _p(shift), act, _st()), "affine_act")
    return y


def randn(shape, seed: int, stream_id: int = 0, device="cuda") -> torch.Tensor:
    x = torch.empty(shape, dtype=torch.float32, device=device)
    check(lib().dm3d_randn(x.data_ptr(), x.numel(), seed, stream_id, _st()), "randn")
    return x


def vq_assign(z: torch.Tensor, codebook_t: torch.Tensor, esq: torch.Tensor) -> torch.Tensor:
    """Nearest-code indices (reference VectorQuantizer.get_code_indices): z [rows, D], codebook_t = E^T [K, D], esq [K]."""
    _f32c(z, "z"), _f32c(codebook_t, "codebook_t")
    rows, dd = z.shape
    k = codebook_t.shape[0]
    sim = gemm_tn(z, codebook_t)                         # exact float32 MFMA: z.E
    idx = torch.empty(rows, dtype=torch.int32, device=z.device)
    check(lib().dm3d_vq_assign(z.data_ptr(), rows, dd, sim.data_ptr(), k, esq.data_ptr(), idx.data_ptr(), _st()), "vq_assign")
    return idx


def gather_rows(table: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    _f32c(table, "table")
    out = torch.empty(idx.numel(), table.shape[1], dtype=torch.float32, device=table.device)
    check(lib().dm3d_gather_rows(table.data_ptr(), table.shape[0], idx.data_ptr(), out.data_ptr(), idx.numel(), table.shape[1],
                                 _st()), "gather_rows")
    return out


def pack_mlp_weights(w_h2: torch.Tensor, units: int, which: int) -> torch.Tensor:
    """DM3D_FMT_H2 weights of the MLP (which = 0: [4 units, units]; 1: [units, 4 units]) -> the operand-fragment image dm3d_mlp_fused reads."""
    out = torch.empty_like(w_h2)
    check(lib().dm3d_pack_mlp_weights(w_h2.data_ptr(), units, which, out.data_ptr(), _st()), "pack_mlp_weights")
    return out


def pack_front_weights(w_h2: torch.Tensor, n: int, units: int = 256) -> torch.Tensor:
    """DM3D_FMT_H2 weight rows W[n][units] (split_h2 of the [n, units] float32 weight) -> the operand-fragment image dm3d_attn_front reads."""
    out = torch.empty_like(w_h2)
    check(lib().dm3d_pack_front_weights(w_h2.data_ptr(), n, units, out.data_ptr(), _st()), "pack_front_weights")
    return out


def attn_front(x: torch.Tensor, w_in_t: torch.Tensor, b_in: torch.Tensor, w_qk_t: torch.Tensor, b_qk: torch.Tensor, w_v_t: torch.Tensor,
               b_v: torch.Tensor, norms, eps: float = 1e-3):
    """The front half of a CrossAttentionBlock in one launch (dm3d_attn_front; conditional_dm3d.py:186-193, 163-170): x [m, 256] float32,
    weights from pack_front_weights, norms = ((g1, b1), (g2, b2), (g3, b3)).  Returns y [m, 256] float32 and the DM3D_FMT_H2 buffers
    qk [m, 512], v_t [256, m], q2 [m, 256], n3 [m, 256] (decode with h2_to_f32)."""
    from ._lib import AttnFrontDesc
    _f32c(x, "x")
    m, u = x.shape
    dev = x.device
    y = torch.empty(m, u, dtype=torch.float32, device=dev)
    qk, v_t = torch.empty(m, 2 * u, dtype=torch.float32, device=dev), torch.empty(u, m, dtype=torch.float32, device=dev)
    q2, n3 = torch.empty(m, u, dtype=torch.float32, device=dev), torch.empty(m, u, dtype=torch.float32, device=dev)
    d = AttnFrontDesc()
    d.x, d.ldx = x.data_ptr(), u
    d.w_in, d.b_in, d.w_qk, d.b_qk, d.w_v, d.b_v = w_in_t.data_ptr(), b_in.data_ptr(), w_qk_t.data_ptr(), b_qk.data_ptr(), w_v_t.data_ptr(), b_v.data_ptr()
    (g1, b1), (g2, b2), (g3, b3) = norms
    d.g1, d.be1, d.g2, d.be2, d.g3, d.be3 = g1.data_ptr(), b1.data_ptr(), g2.data_ptr(), b2.data_ptr(), g3.data_ptr(), b3.data_ptr()
    d.eps = eps
    d.y, d.ldy, d.qk, d.ldqk, d.vt, d.ldvt, d.q2, d.ldq2, d.n3, d.ldn3 = y.data_ptr(), u, qk.data_ptr(), 2 * u, v_t.data_ptr(), m, q2.data_ptr(), u, n3.data_ptr(), u
    d.m, d.units = m, u
    check(lib().dm3d_attn_front(C.byref(d), _st()), "attn_front")
    return y, qk, v_t, q2, n3


def mlp_fused(x_h2: torch.Tensor, w0_t: torch.Tensor, b0: torch.Tensor, w1_t: torch.Tensor, b1: torch.Tensor, units: int,
              res: Optional[torch.Tensor] = None, res2: Optional[torch.Tensor] = None, out_h2: bool = False,
              tail=None) -> torch.Tensor:
    """Dense(units)(relu(Dense(4 units)(x))) + res + res2 in one launch (dm3d_mlp_fused): x [m, units] as a DM3D_FMT_H2 buffer (split_h2),
    w0_t / w1_t from pack_mlp_weights, biases / residuals float32.  Returns [m, units] float32, or a DM3D_FMT_H2 buffer with ``out_h2``.
    ``tail = (w2_t, b2, res3)`` (w2_t from pack_front_weights; res3 may be None): returns relu(Dense_2(that)) + res3 instead (float32)."""
    from ._lib import MlpDesc
    m = x_h2.numel() // units
    out = torch.empty(m, units, dtype=torch.float32, device=x_h2.device)
    d = MlpDesc()
    d.x, d.ldx, d.w0, d.b0, d.w1, d.b1 = x_h2.data_ptr(), units, w0_t.data_ptr(), b0.data_ptr(), w1_t.data_ptr(), b1.data_ptr()
    d.res, d.res2, d.ldr = _p(res), _p(res2), units
    d.out, d.ldo, d.out_fmt, d.m, d.units = out.data_ptr(), units, (_lib.FMT_H2 if out_h2 else _lib.FMT_F32), m, units
    if tail is not None:
        w2_t, b2, res3 = tail
        d.w2, d.b2, d.res3, d.ldr3 = w2_t.data_ptr(), b2.data_ptr(), _p(res3), units
    check(lib().dm3d_mlp_fused(C.byref(d), _st()), "mlp_fused")
    return out


# ---- autoencoder evaluation (include/dm3d.h, dm3d_metric_desc): per-slice squared error, SSIM and PSNR of a reconstruction -------------
class PairStats(NamedTuple):
    """What dm3d_pair_stats leaves on the device: per volume min, max and max - min of the compared channels of y (float32 [B]), per depth
    slice the float64 sum of squared differences over H x W x channels ([B, D])."""
    y_min: torch.Tensor
    y_max: torch.Tensor
    y_range: torch.Tensor
    sse: torch.Tensor


def _window(t, channels):
    """``channels = (first, count)`` selects a channel window of the NDHWC tensor ``t``, read in place (default: all)."""
    return (0, t.shape[4]) if channels is None else channels


def _volume_desc(d, x, y=None, x_channels=None, y_channels=None, *, alone=False, same=slice(0, 4),
                 same_text="x and y must be [B,D,H,W,C] with the same batch and spatial shape"):
    """Fills what the volume descriptors share by name, for one NDHWC tensor (``y`` None) or a pair: x, cx, x0c, nc, d, h, w (y, cy, y0c),
    and batch where ``d`` has one.  ``alone``: x is checked on its own before y is looked at; ``same``: the axes on which a pair must agree."""
    _f32c(x, "x")
    if alone and x.dim() != 5:
        raise ValueError(f"x must be [B,D,H,W,C], got {tuple(x.shape)}")
    if y is not None:
        _f32c(y, "y")
        if x.dim() != 5 or y.dim() != 5 or x.shape[same] != y.shape[same]:
            raise ValueError(f"{same_text}, got {tuple(x.shape)} and {tuple(y.shape)}")
    x0c, nc = _window(x, x_channels)
    if y is not None:
        y0c, ncy = _window(y, y_channels)
        if nc != ncy:
            raise ValueError(f"x contributes {nc} channels and y {ncy}: the same number must be compared")
        d.y, d.cy, d.y0c = y.data_ptr(), y.shape[4], y0c
    d.x, d.cx, d.x0c, d.nc = x.data_ptr(), x.shape[4], x0c, nc
    d.d, d.h, d.w = x.shape[1:4]
    if hasattr(d, "batch"):
        d.batch = x.shape[0]
    return d


def _mask_limits(d, x, threshold, max_extent):
    """The two refusals of the mask entries (distance transform, components): an axis longer than ``max_extent``, a threshold not finite."""
    if max(x.shape[1:4]) > max_extent:
        raise ValueError(f"a {x.shape[1]} x {x.shape[2]} x {x.shape[3]} volume exceeds {max_extent} voxels per axis")
    thr = float(threshold)
    if not math.isfinite(thr):
        raise ValueError(f"threshold must be finite, got {threshold}")
    d.threshold = thr
    return d


def _metric_desc(x, y, x_channels, y_channels):
    """The descriptor of a pair of NDHWC tensors; ``*_channels = (first, count)`` selects a channel window read in place (default: all)."""
    return _volume_desc(_lib.MetricDesc(), x, y, x_channels, y_channels)


def _metric_partials(d, elems: int, device) -> torch.Tensor:
    buf = torch.empty(max(1, elems), dtype=torch.float64, device=device)       # alive until the launches are enqueued (same stream)
    d.partials, d.partials_elems = buf.data_ptr(), buf.numel()
    return buf


def pair_stats(x: torch.Tensor, y: torch.Tensor, *, x_channels=None, y_channels=None) -> PairStats:
    """One pass over the truth ``x`` and the reconstruction ``y`` (NDHWC float32, channel counts may differ): ``PairStats``.  With a
    tensor viewed as [B, 1, 1, n, 1] the one "slice" is the flattened extent: sse / n is a plain mean squared error per sample."""
    d = _metric_desc(x, y, x_channels, y_channels)
    B, D = d.batch, d.d
    blocks = min(-(-(d.h * d.w) // 4096), _lib.PAIR_PARTIAL_BLOCKS)
    buf = _metric_partials(d, 3 * B * D * blocks, x.device)
    mm = torch.empty(3, B, dtype=torch.float32, device=x.device)
    sse = torch.empty(B, D, dtype=torch.float64, device=x.device)
    d.y_min, d.y_max, d.y_range, d.sse = mm[0].data_ptr(), mm[1].data_ptr(), mm[2].data_ptr(), sse.data_ptr()
    check(lib().dm3d_pair_stats(C.byref(d), _st()), "pair_stats")
    del buf
    return PairStats(mm[0], mm[1], mm[2], sse)


def _max_val(max_val, stats, x, y, x_channels, y_channels) -> torch.Tensor:
    """The device table of one float per volume both metrics read: the caller's value, or the reference's choice max(y) - min(y)."""
    if max_val is None:
        return (stats if stats is not None else pair_stats(x, y, x_channels=x_channels, y_channels=y_channels)).y_range
    return _max_val_table(max_val, x.shape[0], "volume", x.device)


def _max_val_table(max_val, rows: int, noun: str, device) -> torch.Tensor:
    """float32 [rows] on the device from a number, or from a tensor of one value or one per row (``noun`` names a row in the refusal)."""
    if isinstance(max_val, torch.Tensor):
        t = max_val.to(device=device, dtype=torch.float32).reshape(-1)
        t = t.expand(rows) if t.numel() == 1 else t
        if t.numel() != rows:
            raise ValueError(f"max_val must hold one value, or one per {noun} ({rows}), got {t.numel()}")
        return t.contiguous()
    return torch.full((rows,), float(max_val), dtype=torch.float32, device=device)


def ssim(x: torch.Tensor, y: torch.Tensor, max_val=None, *, x_channels=None, y_channels=None, stats: Optional[PairStats] = None) -> torch.Tensor:
    """tf.image.ssim(x[b], y[b], max_val) for every volume b, TensorFlow's defaults: float32 [B, D], one score per depth slice (the last
    three axes of a volume are the image).  ``max_val``: a number, a tensor of one value or one per volume, or None for the reference's
    max(y) - min(y) per volume (taken from ``stats``, a ``pair_stats`` of the same pair, or from a pass of its own; the value goes
    from that kernel to this one on the device).  A volume whose max_val is 0 scores NaN, as in TensorFlow."""
    d = _metric_desc(x, y, x_channels, y_channels)
    if d.h < 11 or d.w < 11:
        raise ValueError(f"ssim needs H and W of at least 11 (the 11 x 11 window), got {d.h} x {d.w}")
    mv = _max_val(max_val, stats, x, y, x_channels, y_channels)
    tiles = -(-(d.h - 10) // _lib.SSIM_TILE) * -(-(d.w - 10) // _lib.SSIM_TILE)
    buf = _metric_partials(d, d.batch * d.d * d.nc * tiles, x.device)
    out = torch.empty(d.batch, d.d, dtype=torch.float32, device=x.device)
    d.max_val, d.out = mv.data_ptr(), out.data_ptr()
    check(lib().dm3d_ssim(C.byref(d), _st()), "ssim")
    del buf
    return out


def psnr(x: torch.Tensor, y: torch.Tensor, max_val=None, *, x_channels=None, y_channels=None, stats: Optional[PairStats] = None) -> torch.Tensor:
    """tf.image.psnr(x[b], y[b], max_val) for every volume b: float32 [B, D], 20 log10(max_val) - 10 log10(mse) per depth slice; +inf where
    a slice is reconstructed exactly.  ``max_val`` and ``stats`` as in ``ssim``."""
    d = _metric_desc(x, y, x_channels, y_channels)
    if stats is None:
        stats = pair_stats(x, y, x_channels=x_channels, y_channels=y_channels)
    mv = _max_val(max_val, stats, x, y, x_channels, y_channels)
    out = torch.empty(d.batch, d.d, dtype=torch.float32, device=x.device)
    d.sse, d.max_val, d.out = stats.sse.data_ptr(), mv.data_ptr(), out.data_ptr()
    check(lib().dm3d_psnr_finalize(C.byref(d), _st()), "psnr_finalize")
    return out


# ---- 3-D multi-scale SSIM (include/dm3d.h, dm3d_ms_ssim_desc): fidelity of a reconstruction, diversity of a generated batch ---------
MS_SSIM_POWER_FACTORS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)        # Wang, Simoncelli, Bovik 2003


def ms_ssim_max_scales(spatial, filter_size: int = 11) -> int:
    """The largest number of scales (at most 5) whose coarsest volume still holds one window: min(spatial) >> (scales - 1) >= filter_size."""
    n = 0
    while n < 5 and (min(spatial) >> n) >= filter_size:
        n += 1
    return n


def ms_ssim(x: torch.Tensor, y: torch.Tensor, max_val=None, *, power_factors=MS_SSIM_POWER_FACTORS, filter_size: int = 11,
            filter_sigma: float = 1.5, x_channels=None, y_channels=None, stats: Optional[PairStats] = None, pairs=None) -> torch.Tensor:
    """Multi-scale SSIM (Wang et al. 2003) with a 3-D Gaussian window: float32 [P], one score per compared pair of volumes (the mean
    over the compared channels).  ``x`` [Nx, D, H, W, Cx] and ``y`` [Ny, D, H, W, Cy] are NDHWC float32 device tensors;
    ``*_channels = (first, count)`` reads a channel window in place.  ``len(power_factors)`` is the number of scales (1 to 5); between
    scales both volumes are averaged over 2 x 2 x 2 (an odd edge drops its last plane).  ``filter_size`` is odd, 3 to 11.

    ``pairs`` None compares volume p of x with volume p of y (P = Nx = Ny); an int tensor [P, 2] on the device makes row p compare
    ``x[pairs[p, 0]]`` with ``y[pairs[p, 1]]``, read in place.  ``max_val`` is a number, or a tensor of one value or one per row; None
    is the reference's max(y) - min(y) per volume (``stats`` as in ``ssim``) and is refused with ``pairs``, where a row's y is not one
    volume's own.  Everything stays on the device: the buffers are allocated here and nothing is read back.

    Not offered: the 2-D ``tf.image.ssim_multiscale`` form, other pooling rules, uniform windows."""
    power = tuple(float(w) for w in power_factors)
    if not 1 <= len(power) <= 5 or any(not w > 0.0 for w in power):
        raise ValueError(f"power_factors must be 1 to 5 positive numbers, got {power}")
    if filter_size % 2 == 0 or not 3 <= filter_size <= 11:
        raise ValueError(f"filter_size must be odd and in [3, 11], got {filter_size}")
    if pairs is not None:
        if max_val is None:
            raise ValueError("max_val=None (max(y) - min(y) per volume) is not defined under a pair table: pass max_val")
        if not isinstance(pairs, torch.Tensor) or pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.shape[0] < 1 or pairs.dtype not in (
                torch.int32, torch.int64):
            raise ValueError(f"pairs must be an int32 or int64 tensor [P, 2] with P >= 1, got {getattr(pairs, 'dtype', type(pairs))} "
                             f"{tuple(getattr(pairs, 'shape', ()))}")
    d = _volume_desc(_lib.MsSsimDesc(), x, y, x_channels, y_channels, same=slice(0 if pairs is None else 1, 4),
                     same_text="x and y must be [N,D,H,W,C] with the same spatial shape (and the same N without pairs)")
    D, H, W, ncx = d.d, d.h, d.w, d.nc
    fit = ms_ssim_max_scales((D, H, W), filter_size)
    if len(power) > fit:
        raise ValueError(f"ms_ssim: {len(power)} scales of a {D} x {H} x {W} volume leave an edge smaller than filter_size={filter_size}; "
                         f"at most {fit} scales fit")
    dev = x.device
    if pairs is None:
        P, idx = x.shape[0], None
        mv = _max_val(max_val, stats, x, y, x_channels, y_channels)
    else:
        if pairs.device != dev:
            raise ValueError("pairs must be on the device of x and y")
        P = pairs.shape[0]
        idx = pairs.to(torch.int32).t().contiguous()                            # [2, P]: the two tables
        mv = _max_val_table(max_val, P, "pair", dev)
    TD, TH, TW = _lib.MSSSIM_TILE
    tiles = sum(-(-((D >> j) - filter_size + 1) // TD) * -(-((H >> j) - filter_size + 1) // TH) * -(-((W >> j) - filter_size + 1) // TW)
                for j in range(len(power)))
    pooled = sum((D >> j) * (H >> j) * (W >> j) for j in range(1, len(power)))
    partials = torch.empty(max(1, 2 * P * ncx * tiles), dtype=torch.float64, device=dev)       # alive until the launches are enqueued
    scratch = torch.empty(max(1, (x.shape[0] + y.shape[0]) * ncx * pooled), dtype=torch.float32, device=dev)
    out = torch.empty(P, dtype=torch.float32, device=dev)
    if idx is not None:
        d.x_index, d.y_index = idx[0].data_ptr(), idx[1].data_ptr()
    d.pairs, d.nx, d.ny = P, x.shape[0], y.shape[0]
    d.filter_size, d.filter_sigma, d.scales = filter_size, float(filter_sigma), len(power)
    for j, w in enumerate(power):
        d.power_factors[j] = w
    d.max_val, d.out = mv.data_ptr(), out.data_ptr()
    d.partials, d.partials_elems, d.scratch, d.scratch_elems = partials.data_ptr(), partials.numel(), scratch.data_ptr(), scratch.numel()
    check(lib().dm3d_ms_ssim(C.byref(d), _st()), "ms_ssim")
    del partials, scratch, idx
    return out


# ---- mask-channel scores (include/dm3d.h, dm3d_mask_desc): overlap counts, the exact squared distance transform, surface distances ----
class MaskOverlap(NamedTuple):
    """What dm3d_mask_overlap counts per (volume, channel): int64 [B, nc] voxels of the truth mask, of the other mask, of both."""
    x: torch.Tensor
    y: torch.Tensor
    both: torch.Tensor


class SurfaceDistances(NamedTuple):
    """What dm3d_surface_distance leaves per (volume, channel), float64 [B, nc], in voxels: the Hausdorff distance, its percentile form,
    the average symmetric surface distance (all three NaN where either surface is empty) and the voxel counts of the two surfaces."""
    hd: torch.Tensor
    hd_percentile: torch.Tensor
    assd: torch.Tensor
    surface_x: torch.Tensor
    surface_y: torch.Tensor


def _mask_desc(x, y, threshold, x_channels, y_channels):
    """The descriptor of one NDHWC tensor (``y`` None) or of a pair; ``*_channels = (first, count)`` as in ``_metric_desc``."""
    d = _volume_desc(_lib.MaskDesc(), x, y, x_channels, y_channels, alone=True)
    return _mask_limits(d, x, threshold, _lib.EDT_MAX_EXTENT)


def mask_overlap(x: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, *, x_channels=None, y_channels=None) -> MaskOverlap:
    """The voxel counts behind Dice and IoU: ``MaskOverlap`` of int64 [B, nc], exact.  A mask is ``value > threshold`` (NaN is background),
    per volume and per channel of the window ``*_channels = (first, count)``, read in place from NDHWC float32 device tensors."""
    d = _mask_desc(x, y, threshold, x_channels, y_channels)
    counts = torch.empty(d.batch, d.nc, 3, dtype=torch.int64, device=x.device)
    d.counts = counts.data_ptr()
    check(lib().dm3d_mask_overlap(C.byref(d), _st()), "mask_overlap")
    return MaskOverlap(counts[..., 0], counts[..., 1], counts[..., 2])


def distance_transform(x: torch.Tensor, threshold: float = 0.5, *, channels=None, of: str = "surface") -> torch.Tensor:
    """The exact squared Euclidean distance transform of the masks ``x > threshold``: int32 [B, D, H, W, nc], at every voxel the smallest
    dz^2 + dy^2 + dx^2 to a voxel of the mask's surface (``of="surface"``: mask voxels with a 6-neighbour in the background or outside
    the volume) or of the mask itself (``of="foreground"``); INT32_MAX everywhere where there is none.  The result is a view of a
    channel-planar buffer [B, nc, D, H, W].  Distances are in voxels: anisotropic spacing is not offered, scale the axes yourself."""
    if of not in ("surface", "foreground"):
        raise ValueError(f'of must be "surface" or "foreground", got {of!r}')
    d = _mask_desc(x, None, threshold, channels, None)
    d.of = _lib.EDT_FOREGROUND if of == "foreground" else _lib.EDT_SURFACE
    B, D, H, W, nc = d.batch, d.d, d.h, d.w, d.nc
    out = torch.empty(B, nc, D, H, W, dtype=torch.int32, device=x.device)
    masks = torch.empty(out.numel(), dtype=torch.uint8, device=x.device)       # alive until the launches are enqueued (same stream)
    d.map, d.masks, d.masks_elems = out.data_ptr(), masks.data_ptr(), masks.numel()
    check(lib().dm3d_edt(C.byref(d), _st()), "edt")
    del masks
    return out.permute(0, 2, 3, 4, 1)


def _surface_distances(x, y, threshold, percentile, x_channels, y_channels, want_counts):
    pct = float(percentile)
    if not 0.0 < pct <= 100.0:
        raise ValueError(f"percentile must be in (0, 100], got {percentile}")
    d = _mask_desc(x, y, threshold, x_channels, y_channels)
    B, D, H, W, nc = d.batch, d.d, d.h, d.w, d.nc
    vox = B * nc * D * H * W
    bins = (D - 1) ** 2 + (H - 1) ** 2 + (W - 1) ** 2 + 1
    masks = torch.empty(2 * vox, dtype=torch.uint8, device=x.device)           # alive until the launches are enqueued (same stream)
    work = torch.empty(vox + 2 * B * nc * (bins + 1), dtype=torch.int32, device=x.device)
    out = torch.empty(B, nc, 5, dtype=torch.float64, device=x.device)
    counts = torch.empty(B, nc, 3, dtype=torch.int64, device=x.device) if want_counts else None
    d.percentile, d.out, d.counts = pct, out.data_ptr(), _p(counts)
    d.masks, d.masks_elems, d.work, d.work_elems = masks.data_ptr(), masks.numel(), work.data_ptr(), work.numel()
    check(lib().dm3d_surface_distance(C.byref(d), _st()), "surface_distance")
    del masks, work
    dist = SurfaceDistances(*(out[..., k] for k in range(5)))
    return dist, (MaskOverlap(counts[..., 0], counts[..., 1], counts[..., 2]) if want_counts else None)


def surface_distances(x: torch.Tensor, y: torch.Tensor, threshold: float = 0.5, percentile: float = 95.0, *, x_channels=None,
                      y_channels=None) -> SurfaceDistances:
    """Distances between the surfaces of the masks ``x > threshold`` and ``y > threshold`` (MONAI's definitions): ``SurfaceDistances`` of
    float64 [B, nc].  The directed distances X -> Y are the exact distance map of Y's surface read at X's surface voxels; ``hd`` is the
    larger of the two directed maxima, ``hd_percentile`` the larger of the two directed percentiles (numpy's linear rule,
    ``percentile`` in (0, 100]), ``assd`` the mean over both directed sets together.  Everything stays on the device.  Distances are in
    voxels: anisotropic spacing is not offered, the caller scales.  No axis may exceed 512 voxels."""
    return _surface_distances(x, y, threshold, percentile, x_channels, y_channels, False)[0]


# ---- connected components of the mask channels (include/dm3d.h, dm3d_ccl_desc): labels, count, largest, the three filters -------------
class Components(NamedTuple):
    """What dm3d_components leaves: ``labels`` int32 [B, D, H, W, nc] (0 at the background, scipy.ndimage.label's numbering per volume
    and channel; a view of a channel-planar buffer), ``count`` int32 [B, nc], ``largest`` int64 [B, nc, 2] = (label, size) of the
    component with the most voxels, the lowest label on a tie, (0, 0) for an empty mask."""
    labels: torch.Tensor
    count: torch.Tensor
    largest: torch.Tensor


CONNECTIVITIES = (6, 18, 26)


def _ccl_desc(x, threshold, channels, connectivity, planes):
    """The descriptor of one NDHWC tensor and its scratch of ``planes`` int32 planes (alive while the caller holds it)."""
    d = _volume_desc(_lib.CclDesc(), x, None, channels, alone=True)
    if connectivity not in CONNECTIVITIES:
        raise ValueError(f"connectivity must be 6, 18 or 26, got {connectivity!r}")
    _mask_limits(d, x, threshold, _lib.CCL_MAX_EXTENT).connectivity = connectivity
    vol = d.d * d.h * d.w
    nblk = -(-vol // _lib.CCL_BLOCK_VOXELS)
    work = torch.empty(planes * d.batch * d.nc * vol + 1 + d.batch * d.nc * (3 * nblk + 2), dtype=torch.int32, device=x.device)
    d.work, d.work_elems = work.data_ptr(), work.numel()
    return d, work


def connected_components(x: torch.Tensor, threshold: float = 0.5, *, channels=None, connectivity: int = 6) -> Components:
    """The connected components of the masks ``x > threshold`` (NaN is background), per volume and per channel of the window
    ``channels = (first, count)``, read in place from an NDHWC float32 device tensor: ``Components(labels, count, largest)``.
    ``connectivity`` is 6, 18 or 26 (``scipy.ndimage.generate_binary_structure(3, 1 | 2 | 3)``); nothing connects across volumes,
    channels or round the border.  Labels do not depend on the order anything ran in: runs repeat bitwise.  Nothing is read back.  No
    axis may exceed 512 voxels; anisotropy, per-label size tables and slice-wise labelling are not offered."""
    d, work = _ccl_desc(x, threshold, channels, connectivity, 2)
    labels = torch.empty(d.batch, d.nc, d.d, d.h, d.w, dtype=torch.int32, device=x.device)
    count = torch.empty(d.batch, d.nc, dtype=torch.int32, device=x.device)
    largest = torch.empty(d.batch, d.nc, 2, dtype=torch.int64, device=x.device)
    d.labels, d.count, d.largest = labels.data_ptr(), count.data_ptr(), largest.data_ptr()
    check(lib().dm3d_components(C.byref(d), _st()), "components")
    del work                                                                    # alive until the launches are enqueued (same stream)
    return Components(labels.permute(0, 2, 3, 4, 1), count, largest)


def _component_filter(x, threshold, channels, connectivity, mode, min_size=1):
    d, work = _ccl_desc(x, threshold, channels, connectivity, 3)
    out = torch.empty(d.batch, d.d, d.h, d.w, d.nc, dtype=torch.float32, device=x.device)
    d.mode, d.min_size, d.out = mode, min(int(min_size), 2 ** 31 - 1), out.data_ptr()
    check(lib().dm3d_component_filter(C.byref(d), _st()), "component_filter")
    del work
    return out


def component_filter(x: torch.Tensor, threshold: float = 0.5, *, channels=None, connectivity: int = 6, keep: Optional[str] = None,
                     min_size: Optional[int] = None, fill_holes: bool = False) -> torch.Tensor:
    """The masks ``x > threshold`` cleaned through their connected components: float32 [B, D, H, W, nc] of 0 and 1, ready for
    ``metrics.mask_metrics``.  At least one of

        min_size=n        (n >= 1) keep every component with at least n voxels          MONAI's RemoveSmallObjects
        keep="largest"    keep the component with the most voxels, the lowest label on a tie; an empty mask stays empty
                                                                                         MONAI's KeepLargestConnectedComponent
        fill_holes=True   add every background voxel whose 6-connected background component touches no face of the volume
                                                                                         scipy.ndimage.binary_fill_holes / MONAI's FillHoles

    must be asked for; several apply in that order, each stage reading the previous stage's result at threshold 0.5.  ``connectivity``
    (6, 18, 26) is the foreground's; the background of ``fill_holes`` is always 6-connected.  Nothing is read back."""
    if keep not in (None, "largest"):
        raise ValueError(f'keep must be "largest" or None, got {keep!r}')
    if min_size is not None and (int(min_size) != min_size or min_size < 1):
        raise ValueError(f"min_size must be an integer of at least 1, got {min_size!r}")
    if keep is None and min_size is None and not fill_holes:
        raise ValueError('component_filter needs at least one of min_size, keep="largest" and fill_holes=True')
    stages = []
    if min_size is not None:
        stages.append((_lib.CCL_MIN_SIZE, int(min_size)))
    if keep is not None:
        stages.append((_lib.CCL_LARGEST, 1))
    if fill_holes:
        stages.append((_lib.CCL_FILL_HOLES, 1))
    for mode, n in stages:
        x = _component_filter(x, threshold, channels, connectivity, mode, n)
        threshold, channels = 0.5, None
    return x


# ---- volume preprocessing (include/dm3d.h, "Volume preprocessing"): spline prefilter, affine resample, normalise, augment --------------
SPLINE_ORDERS = (0, 1, 3)


def _volume_check(x, name="x", *, spline=False, ndhwc=False, one_channel=False, host=None):
    """The tensor checks of the preprocessing entries, in one order on any machine: dtype, rank (``ndhwc``: five axes only), empty axes,
    the prefilter's extent (``spline``), one channel per volume (``one_channel``), then ``host()``, the caller's checks of its host
    arguments, whose value is returned, and the device last."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise ValueError(f"{name} must be a float32 tensor, got {getattr(x, 'dtype', type(x).__name__)}")
    if x.dim() not in ((5,) if ndhwc else (4, 5)):
        raise ValueError(f"{name} must be {'' if ndhwc else '[B,D,H,W] or '}[B,D,H,W,C], got {tuple(x.shape)}")
    if min(x.shape) < 1:
        raise ValueError(f"{name} has an empty axis: {tuple(x.shape)}")
    if spline and max(x.shape[1:4]) > _lib.SPLINE_MAX_EXTENT:
        raise ValueError(f"a {x.shape[1]} x {x.shape[2]} x {x.shape[3]} volume exceeds {_lib.SPLINE_MAX_EXTENT} voxels per axis, the longest line "
                         "the spline prefilter stages")
    if one_channel and x.dim() == 5 and x.shape[4] != 1:
        raise ValueError(f"{name} must hold one channel per volume, got C={x.shape[4]}")
    checked = host() if host is not None else None
    _f32c(x, name)
    return checked


def _planar(x):
    """[B,D,H,W] as it is, [B,D,H,W,C] as the channel-planar [B*C,D,H,W] (a view for C = 1, a copy otherwise), and the way back."""
    if x.dim() == 4:
        return x, lambda t: t
    B, D, H, W, Cn = x.shape
    if Cn == 1:
        return x.reshape(B, D, H, W), lambda t: t.unsqueeze(-1)
    return (x.permute(0, 4, 1, 2, 3).contiguous().view(B * Cn, D, H, W),
            lambda t: t.reshape(B, Cn, *t.shape[1:]).permute(0, 2, 3, 4, 1).contiguous())


def _spline_coefficients(planar):
    V, D, H, W = planar.shape
    coeff = torch.empty(V, D, H, W, dtype=torch.float64, device=planar.device)
    d = _lib.SplineDesc()
    d.x, d.coeff, d.volumes, d.d, d.h, d.w = planar.data_ptr(), coeff.data_ptr(), V, D, H, W
    check(lib().dm3d_spline_filter(C.byref(d), _st()), "spline_filter")
    return coeff


def spline_filter(x: torch.Tensor) -> torch.Tensor:
    """``scipy.ndimage.spline_filter(x, order=3, mode="mirror")`` over the three spatial axes of every volume of ``x`` ([B,D,H,W], or
    NDHWC with each channel a volume): the float64 cubic B-spline coefficients, in x's layout.  This is the prefilter scipy runs in front
    of ``mode="constant"`` interpolation; an axis of length 1 is left unfiltered, as scipy leaves it.  No axis may exceed 512 voxels."""
    _volume_check(x, spline=True)
    planar, back = _planar(x)
    return back(_spline_coefficients(planar))


def _affine_table(matrix, offset, batch, per):
    """The float64 host table [batch * per, 12] of (matrix row by row, offset) from what ``affine_transform`` accepts."""
    import numpy as np
    as_np = lambda v: (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)).astype(np.float64)
    m, off = as_np(matrix), as_np(offset)
    if m.shape in ((4, 4), (batch, 4, 4)):                                      # homogeneous: the offset is its last column, as in scipy
        if not np.array_equal(m[..., 3, :], np.broadcast_to([0.0, 0.0, 0.0, 1.0], m.shape[:-2] + (4,))):
            raise ValueError("the last row of a homogeneous matrix must be (0, 0, 0, 1)")
        if off.any():
            raise ValueError("offset must be left at 0 with a homogeneous matrix: its last column is the offset")
        m, off = m[..., :3, :3], m[..., :3, 3]
    if m.shape == (3,):
        m = np.diag(m)
    if m.shape == (3, 3):
        m = np.broadcast_to(m, (batch, 3, 3))
    if m.shape != (batch, 3, 3):
        raise ValueError(f"matrix must be a 3-vector, [3,3], [4,4] homogeneous or [B,3,3] with B={batch}, got {tuple(as_np(matrix).shape)}")
    if off.shape not in ((), (3,), (batch, 3)):
        raise ValueError(f"offset must be a scalar, a 3-vector or [B,3] with B={batch}, got {tuple(off.shape)}")
    off = np.broadcast_to(off, (batch, 3))
    if not (np.isfinite(m).all() and np.isfinite(off).all()):
        raise ValueError("matrix and offset must be finite")
    table = np.concatenate([m.reshape(batch, 9), off], 1)
    return np.ascontiguousarray(np.repeat(table, per, 0))


def affine_transform(x: torch.Tensor, matrix, offset=0.0, output_shape=None, order: int = 3, cval: float = 0.0, prefilter: bool = True,
                     mode: str = "constant") -> torch.Tensor:
    """``scipy.ndimage.affine_transform(volume, matrix, offset, output_shape, order=order, mode="constant", cval=cval)`` of every volume of
    ``x`` ([B,D,H,W], or NDHWC with each channel a volume): ``out[o] = interp(volume, matrix @ o + offset)``, float32, in x's layout with
    the spatial shape ``output_shape`` (default: x's).  ``matrix`` is a 3-vector (a diagonal, scipy's zoom form), [3,3], [4,4] homogeneous
    (last row (0, 0, 0, 1), its last column is the offset and ``offset`` stays 0), [B,4,4] or [B,3,3], ``offset`` a scalar, a 3-vector or [B,3]; both are host values, formed in float64.
    ``order`` 0 is nearest (floor(c + 0.5)), 1 trilinear, 3 cubic B-spline on the prefiltered coefficients (``prefilter=False``: x already
    holds them).  A coordinate below 0 or above n - 1 on any axis gives ``cval``; spline taps beyond the edge are mirrored.  Coordinates
    are ((o0 m0 + o1 m1) + o2 m2) + offset in float64, the taps are summed in float64 in one fixed order, runs repeat bitwise.  Orders 2,
    4 and 5 and the other boundary modes are not offered."""
    if order not in SPLINE_ORDERS:
        raise ValueError(f"order must be 0, 1 or 3, got {order!r}: orders 2, 4 and 5 are not offered")
    if mode != "constant":
        raise ValueError(f'mode must be "constant", got {mode!r}: the other boundary modes are not offered')
    if not math.isfinite(float(cval)):
        raise ValueError(f"cval must be finite, got {cval}")
    filtered = order == 3 and prefilter

    def host_arguments():
        shape = tuple(int(s) for s in (x.shape[1:4] if output_shape is None else output_shape))
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"output_shape must be three positive extents, got {output_shape!r}")
        return _affine_table(matrix, offset, x.shape[0], 1 if x.dim() == 4 else x.shape[4]), shape

    table, shape = _volume_check(x, spline=filtered, host=host_arguments)
    planar, back = _planar(x)
    src = _spline_coefficients(planar) if filtered else planar
    V = planar.shape[0]
    dev_table = torch.from_numpy(table).to(x.device)
    out = torch.empty(V, *shape, dtype=torch.float32, device=x.device)
    d = _lib.ResampleDesc()
    d.src, d.table, d.out, d.in_f64 = src.data_ptr(), dev_table.data_ptr(), out.data_ptr(), (_lib.RESAMPLE_F64 if filtered else _lib.RESAMPLE_F32)
    d.volumes, d.id, d.ih, d.iw = planar.shape
    d.od, d.oh, d.ow = shape
    d.order, d.cval = order, float(cval)
    check(lib().dm3d_affine_resample(C.byref(d), _st()), "affine_resample")
    del src, dev_table                                                          # alive until the launch is enqueued (same stream)
    return back(out)


class Normalized(NamedTuple):
    """What dm3d_volume_normalize leaves: the normalised volumes, ``minmax`` float32 [B, 2] (min and max of |x| per volume, exact) and
    ``constant`` int32 [B], 1 where max = min (that volume is written as zeros).  All on the device; nothing is read back."""
    out: torch.Tensor
    minmax: torch.Tensor
    constant: torch.Tensor


def volume_normalize(x: torch.Tensor) -> Normalized:
    """Per volume of ``x`` ([B,D,H,W] or [B,D,H,W,1]): a = |x| (the reference's ``vol[vol < 0] *= -1``), then (a - min a) / (max a - min a),
    evaluated in float64 and rounded once.  Lazy: the constant-volume flag stays on the device (``data.normalize`` reads it)."""
    _volume_check(x, one_channel=True)
    B, n = x.shape[0], x[0].numel()
    out = torch.empty_like(x)
    partials = torch.empty(B, _lib.NORM_PARTIAL_BLOCKS, 2, dtype=torch.float32, device=x.device)
    minmax = torch.empty(B, 2, dtype=torch.float32, device=x.device)
    flag = torch.empty(B, dtype=torch.int32, device=x.device)
    d = _lib.NormalizeDesc()
    d.x, d.out, d.volumes, d.n = x.data_ptr(), out.data_ptr(), B, n
    d.partials, d.minmax, d.flag = partials.data_ptr(), minmax.data_ptr(), flag.data_ptr()
    check(lib().dm3d_volume_normalize(C.byref(d), _st()), "volume_normalize")
    del partials
    return Normalized(out, minmax, flag)


class Augmented(NamedTuple):
    """What dm3d_augment leaves: the augmented images, the masks flipped with them (None without masks) and the per-sample ``flip``
    (int32 0 / 1), ``brightness`` and ``contrast`` (float32) that were applied, drawn or given.  All on the device."""
    images: torch.Tensor
    masks: Optional[torch.Tensor]
    flip: torch.Tensor
    brightness: torch.Tensor
    contrast: torch.Tensor


def augment(images: torch.Tensor, masks: Optional[torch.Tensor] = None, *, seed: Optional[int] = None, flip_chance: float = 0.6,
            brightness_range=(0.9, 1.1), contrast_range=(0.9, 1.1), flip=None, brightness=None, contrast=None) -> Augmented:
    """dm3d_augment on NDHWC batches (``data.augment`` documents the definitions).  Each of ``flip`` (int32 [B]), ``brightness`` and
    ``contrast`` (float32 [B]) that is not given is drawn on the device and needs ``seed``."""
    _volume_check(images, "images", ndhwc=True)
    if masks is not None:
        _volume_check(masks, "masks", ndhwc=True)
        if masks.shape[:4] != images.shape[:4]:
            raise ValueError(f"masks must be [B,D,H,W,C] with the batch and spatial shape of images, got {tuple(masks.shape)} and {tuple(images.shape)}")
    B, D, H, W, Cn = images.shape
    dev = images.device
    draw, tables = 0, []
    for bit, given, dtype, name in ((1, flip, torch.int32, "flip"), (2, brightness, torch.float32, "brightness"), (4, contrast, torch.float32, "contrast")):
        if given is None:
            draw |= bit
            tables.append(torch.empty(B, dtype=dtype, device=dev))
        else:
            if not isinstance(given, torch.Tensor) or given.dtype != dtype or tuple(given.shape) != (B,) or not given.is_cuda or not given.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {dtype} device tensor [B] with B={B}")
            tables.append(given)
    if draw and seed is None:
        raise ValueError("augment needs seed= unless flip, brightness and contrast are all given")
    for name, (lo, hi) in (("brightness_range", brightness_range), ("contrast_range", contrast_range)):
        if not (math.isfinite(lo) and math.isfinite(hi) and lo <= hi):
            raise ValueError(f"{name} must be finite and ascending, got ({lo}, {hi})")
    if not 0.0 <= flip_chance <= 1.0:
        raise ValueError(f"flip_chance must be in [0, 1], got {flip_chance}")
    out = torch.empty_like(images)
    mask_out = None if masks is None else torch.empty_like(masks)
    partials = torch.empty(B, _lib.AUG_PARTIAL_BLOCKS, dtype=torch.float64, device=dev)
    d = _lib.AugmentDesc()
    d.x, d.out, d.mask, d.mask_out = images.data_ptr(), out.data_ptr(), _p(masks), _p(mask_out)
    d.batch, d.d, d.h, d.w, d.c, d.cm = B, D, H, W, Cn, (0 if masks is None else masks.shape[4])
    d.flip, d.brightness, d.contrast = (t.data_ptr() for t in tables)
    d.draw, d.seed = draw, (int(seed) & (2 ** 64 - 1) if seed is not None else 0)
    d.flip_chance = flip_chance
    d.brightness_lo, d.brightness_hi = brightness_range
    d.contrast_lo, d.contrast_hi = contrast_range
    d.partials = partials.data_ptr()
    check(lib().dm3d_augment(C.byref(d), _st()), "augment")
    del partials
    return Augmented(out, mask_out, *tables)


# ---- spatial augmentation (include/dm3d.h, "Spatial augmentation"): Gaussian filter, elastic field, warp ---------------------------------
def _vec3(v, name, low=None):
    """A scalar or a 3-vector as three finite floats (at least ``low`` when given)."""
    import numpy as np
    try:
        a = np.broadcast_to(np.asarray(v, np.float64), (3,))
    except (TypeError, ValueError):
        a = None
    if a is None or not np.isfinite(a).all() or (low is not None and (a < low).any()):
        raise ValueError(f"{name} must be a finite scalar or 3-vector" + (f" of at least {low:g}" if low is not None else "") + f", got {v!r}")
    return [float(s) for s in a]


def _gauss_table(sigma, truncate):
    """The radii (-1 where scipy skips the axis: sigma <= 1e-15) and the host table [3, GAUSS_MAX_RADIUS + 1] of the float64 weights w[0 .. r]
    per axis d, h, w, formed as scipy.ndimage forms them: exp(-0.5 / sigma^2 * k^2) over k = -r .. r, divided by their sum."""
    import numpy as np
    sig = _vec3(sigma, "sigma", 0.0)
    if not (isinstance(truncate, (int, float)) and math.isfinite(truncate) and truncate > 0):
        raise ValueError(f"truncate must be a positive finite number, got {truncate!r}")
    radii, table = [], np.zeros((3, _lib.GAUSS_MAX_RADIUS + 1), np.float64)
    for a, s in enumerate(sig):
        if s <= 1e-15:
            radii.append(-1)
            continue
        r = int(float(truncate) * s + 0.5)
        if r > _lib.GAUSS_MAX_RADIUS:
            raise ValueError(f"sigma={s:g} with truncate={truncate:g} has radius {r}, above DM3D_GAUSS_MAX_RADIUS={_lib.GAUSS_MAX_RADIUS}")
        k = np.arange(-r, r + 1)
        phi = np.exp(-0.5 / (s * s) * k ** 2)
        phi = phi / phi.sum()
        table[a, :r + 1] = phi[r:]
        radii.append(r)
    return radii, table


def _gaussian(planar, out, radii, table, mode, cval, gain=None):
    d = _lib.GaussDesc()
    d.x, d.out, d.weights = planar.data_ptr(), out.data_ptr(), table.ctypes.data
    d.volumes, d.d, d.h, d.w = planar.shape
    d.rd, d.rh, d.rw = radii
    d.mode, d.cval = _lib.GAUSS_MODES[mode], float(cval)
    if gain is not None:
        d.gains, (d.gain0, d.gain1, d.gain2) = 3, gain
    check(lib().dm3d_gaussian_filter(C.byref(d), _st()), "gaussian_filter")      # the weights are copied into the launches during the call
    return out


def gaussian_filter(x: torch.Tensor, sigma, mode: str = "reflect", cval: float = 0.0, truncate: float = 4.0, *, order: int = 0) -> torch.Tensor:
    """``scipy.ndimage.gaussian_filter(volume, sigma, order=0, mode=mode, cval=cval, truncate=truncate)`` of every volume of ``x``
    ([B,D,H,W], or NDHWC with each channel a volume), float32 in x's layout.  ``sigma`` is a scalar or a 3-vector (d, h, w); an axis with
    sigma 0 is left out, an axis of length 1 is filtered (scipy sums its extended taps).  The float64 weights are formed on the host as
    scipy forms them (radius int(truncate sigma + 0.5), at most 64); each axis pass sums x[l] w0 + sum_{k=r..1} (x[l-k] + x[l+k]) w_k in
    float64 and stores float32, in the order d, h, w, so the result is scipy's bit for bit.  ``mode`` is "reflect", "mirror", "nearest" or
    "constant" (``cval``); "wrap" and Gaussian derivatives (``order`` != 0) are not offered.  No axis may exceed 512 voxels."""
    if order != 0:
        raise ValueError(f"order must be 0, got {order!r}: Gaussian derivatives are not offered")
    if mode not in _lib.GAUSS_MODES:
        raise ValueError(f'mode must be "reflect", "mirror", "nearest" or "constant", got {mode!r}: "wrap" is not offered')
    if not (isinstance(cval, (int, float)) and math.isfinite(cval)):
        raise ValueError(f"cval must be finite, got {cval!r}")
    radii, table = _volume_check(x, spline=True, host=lambda: _gauss_table(sigma, truncate))
    planar, back = _planar(x)
    return back(_gaussian(planar, torch.empty_like(planar), radii, table, mode, cval))


def _field_arguments(alpha, sigma, seed, truncate=4.0):
    """The host arguments of an elastic field, checked: (gain per component, radii, weight table)."""
    gain = _vec3(alpha, "alpha")
    radii, table = _gauss_table(sigma, truncate)
    if not isinstance(seed, int):
        raise ValueError(f"seed must be an integer, got {seed!r}")
    return gain, radii, table


def elastic_field(shape, batch: int, alpha, sigma, seed: int, draw: int = 0, device="cuda", truncate: float = 4.0) -> torch.Tensor:
    """The displacement field of a random elastic deformation (Simard et al. 2003), float32 [batch, 3, D, H, W] in voxels:
    ``gaussian_filter(U(-1, 1), sigma, mode="constant", cval=0) * alpha``; ``alpha`` and ``sigma`` are scalars or 3-vectors (alpha per
    displacement component d, h, w; sigma per spatial axis).  Element e of the flat field takes word e & 3 of the Philox4x32-10 block of
    counter (lo32(e >> 2), hi32(e >> 2), draw, 0xE1A5) under the 64-bit key ``seed``: v = float32(word) * 2^-32, then 2 v - 1 in float32.
    The draw is a launch of its own, the filter runs in place on it, the scaling is one float32 multiply.  Nothing is read back."""
    shape = tuple(int(s) for s in shape) if hasattr(shape, "__len__") else ()
    if len(shape) != 3 or min(shape) < 1:
        raise ValueError(f"shape must be three positive extents, got {shape!r}")
    if max(shape) > _lib.SPLINE_MAX_EXTENT:
        raise ValueError(f"shape {shape} exceeds {_lib.SPLINE_MAX_EXTENT} voxels per axis, the longest line the Gaussian filter stages")
    if not isinstance(batch, int) or batch < 1:
        raise ValueError(f"batch must be a positive integer, got {batch!r}")
    gain, radii, table = _field_arguments(alpha, sigma, seed, truncate)
    if not isinstance(draw, int) or not 0 <= draw < 2 ** 31:
        raise ValueError(f"draw must be an integer in [0, 2^31), got {draw!r}")
    field = torch.empty(batch, 3, *shape, dtype=torch.float32, device=device)
    _f32c(field, "the field (device=)")
    d = _lib.FieldDesc()
    d.out, d.n, d.seed, d.draw = field.data_ptr(), field.numel(), seed & (2 ** 64 - 1), draw
    check(lib().dm3d_uniform_field(C.byref(d), _st()), "uniform_field")
    planar = field.view(batch * 3, *shape)
    _gaussian(planar, planar, radii, table, "constant", 0.0, gain)
    return field


def warp(x: torch.Tensor, displacement: Optional[torch.Tensor] = None, matrix=None, offset=0.0, output_shape=None, order: int = 1, cval: float = 0.0,
         prefilter: bool = True, *, coordinates: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Every volume of ``x`` ([B,D,H,W], or NDHWC with each channel a volume) resampled at per-voxel coordinates, in one interpolation:
    ``out[o] = interp(volume, (matrix @ o + offset) + displacement[:, o])``, float32 in x's layout with the spatial shape ``output_shape``
    (default: the field's, else x's).  ``matrix`` / ``offset`` are what ``affine_transform`` accepts (None: the identity);
    ``displacement`` is a contiguous device tensor [B,3,od,oh,ow] (or [1,3,od,oh,ow], shared by the batch), float32 or float64, in voxels
    along d, h, w; the channels of one NDHWC item share its field.  Orders, ``cval``, ``prefilter``, the taps and the sums are
    ``affine_transform``'s; the coordinate is (((o0 m0 + o1 m1) + o2 m2) + offset) + u in float64.  ``coordinates`` instead of
    ``displacement`` gives absolute float64 coordinates (``map_coordinates``); then ``matrix`` stays None.  The other boundary modes of
    ``scipy.ndimage.map_coordinates`` are not offered."""
    if order not in SPLINE_ORDERS:
        raise ValueError(f"order must be 0, 1 or 3, got {order!r}: orders 2, 4 and 5 are not offered")
    if not (isinstance(cval, (int, float)) and math.isfinite(cval)):
        raise ValueError(f"cval must be finite, got {cval!r}")
    if displacement is not None and coordinates is not None:
        raise ValueError("displacement and coordinates must not both be given: coordinates are absolute, a displacement is added to the grid")
    if coordinates is not None and matrix is not None:
        raise ValueError("matrix must stay None with coordinates: they are absolute")
    field, fname = (displacement, "displacement") if coordinates is None else (coordinates, "coordinates")
    filtered = order == 3 and prefilter

    def host_arguments():
        import numpy as np
        B, per = x.shape[0], (1 if x.dim() == 4 else x.shape[4])
        default = x.shape[1:4] if field is None or not isinstance(field, torch.Tensor) or field.dim() != 5 else field.shape[2:]
        shape = tuple(int(s) for s in (default if output_shape is None else output_shape))
        if len(shape) != 3 or min(shape) < 1:
            raise ValueError(f"output_shape must be three positive extents, got {output_shape!r}")
        if field is not None:
            if not isinstance(field, torch.Tensor) or field.dtype not in (torch.float32, torch.float64):
                raise ValueError(f"{fname} must be a float32 or float64 tensor, got {getattr(field, 'dtype', type(field).__name__)}")
            if field.dim() != 5 or field.shape[0] not in (1, B) or tuple(field.shape[1:]) != (3,) + shape:
                raise ValueError(f"{fname} must be [B,3,od,oh,ow] or [1,3,od,oh,ow] with B={B} and the output shape {shape}, got {tuple(field.shape)}")
            if not field.is_cuda or not field.is_contiguous() or field.device != x.device:
                raise ValueError(f"{fname} must be a contiguous device tensor on x's device")
        if coordinates is not None:
            table = np.zeros((B * per, 12), np.float64)
        else:
            table = _affine_table(np.eye(3) if matrix is None else matrix, offset, B, per)
        return table, shape, (per if field is None or field.shape[0] == B else B * per)

    table, shape, per_field = _volume_check(x, spline=filtered, host=host_arguments)
    planar, back = _planar(x)
    src = _spline_coefficients(planar) if filtered else planar
    V = planar.shape[0]
    dev_table = torch.from_numpy(table).to(x.device)
    out = torch.empty(V, *shape, dtype=torch.float32, device=x.device)
    d = _lib.WarpDesc()
    d.src, d.table, d.field, d.out = src.data_ptr(), dev_table.data_ptr(), _p(field), out.data_ptr()
    d.in_f64 = _lib.RESAMPLE_F64 if filtered else _lib.RESAMPLE_F32
    d.field_f64 = _lib.RESAMPLE_F64 if field is not None and field.dtype == torch.float64 else _lib.RESAMPLE_F32
    d.volumes, d.id, d.ih, d.iw = planar.shape
    d.vols_per_field = per_field
    d.od, d.oh, d.ow = shape
    d.order, d.cval = order, float(cval)
    check(lib().dm3d_warp(C.byref(d), _st()), "warp")
    del src, dev_table                                                          # alive until the launch is enqueued (same stream)
    return back(out)


def map_coordinates(x: torch.Tensor, coordinates: torch.Tensor, order: int = 1, cval: float = 0.0, prefilter: bool = True) -> torch.Tensor:
    """``scipy.ndimage.map_coordinates(volume, coordinates[b], order=order, mode="constant", cval=cval, prefilter=prefilter)`` of every
    volume of ``x``: ``coordinates`` is a contiguous float64 (or float32) device tensor [B,3,od,oh,ow] (or [1,3,...], shared).  It is
    ``warp`` with a zero matrix and offset: (0 + 0 + 0 + 0) + c is c exactly."""
    if coordinates is None:
        raise ValueError("coordinates must be given")
    return warp(x, None, None, 0.0, None, order, cval, prefilter, coordinates=coordinates)


# ---- distribution metrics on feature vectors (include/dm3d.h, dm3d_dist_desc): moments, k-NN radii, PRDC counts, cubic-kernel sums -----
class FeatureMoments(NamedTuple):
    """What dm3d_feature_moments leaves: ``mean`` float64 [D] and the unbiased ``cov`` float64 [D, D], symmetric bit for bit."""
    mean: torch.Tensor
    cov: torch.Tensor


class PrdcCounts(NamedTuple):
    """What dm3d_prdc_counts leaves, all int32: ``count_fake`` [M], the real balls a generated row lies in; ``near_real`` [N], 1 where a
    real row lies in some generated row's ball; ``cover_real`` [N], 1 where a real row's nearest generated row lies in its ball."""
    count_fake: torch.Tensor
    near_real: torch.Tensor
    cover_real: torch.Tensor


def _features_check(t, name: str, other=None, min_rows: int = 2) -> None:
    """What every feature matrix must be, whatever machine it is checked on: 2-D, float32 or float64, within the limits."""
    if not isinstance(t, torch.Tensor) or t.dim() != 2:
        raise ValueError(f"{name} must be a 2-D feature tensor [rows, D], got {tuple(getattr(t, 'shape', ()))}: flatten or pool the features to one vector per sample first")
    if t.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"{name} must be float32 or float64, got {t.dtype}: cast with .float() or .double()")
    n, dim = t.shape
    if n < min_rows:
        raise ValueError(f"{name} has {n} rows, at least {min_rows} are needed")
    if dim < 1 or dim > _lib.DIST_MAX_DIM:
        raise ValueError(f"{name} has D={dim} features; 1 to {_lib.DIST_MAX_DIM} are taken: pool or project the features first")
    if n > _lib.DIST_MAX_ROWS:
        raise ValueError(f"{name} has {n} rows, at most {_lib.DIST_MAX_ROWS} are taken: score a subsample")
    if other is not None and other.shape[1] != dim:
        raise ValueError(f"{name} has D={dim} features, the other set has D={other.shape[1]}: both sets must come from one feature extractor")


def _features(t, name: str, other=None, min_rows: int = 2) -> torch.Tensor:
    """``_features_check``, then the device, then the exact widening to contiguous float64."""
    _features_check(t, name, other, min_rows)
    if not t.is_cuda:
        raise ValueError(f"{name} must be a device tensor: the distribution kernels have no CPU path")
    return t.to(torch.float64).contiguous()


def _feature_pair(real, fake, min_fake: int = 2):
    """Both sets of a two-set score: every shape check of both before the first device check."""
    _features_check(real, "real")
    _features_check(fake, "fake", real, min_fake)
    return _features(real, "real"), _features(fake, "fake", real, min_fake)


def _row_table(rows, name: str, device, per_subset: bool = False):
    """An optional int32 row table [n] (``per_subset``: [S, n]) on the device."""
    if rows is None:
        return None
    if not isinstance(rows, torch.Tensor) or rows.dim() != (2 if per_subset else 1) or rows.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"{name} must be an int32 or int64 tensor {'[subsets, rows]' if per_subset else '[rows]'} or None")
    return rows.to(device=device, dtype=torch.int32).contiguous()


def _dist_desc(x, rows_x, y=None, rows_y=None):
    d = _lib.DistDesc()
    d.x, d.nx, d.dim, d.rows_x = x.data_ptr(), x.shape[0], x.shape[1], _p(rows_x)
    d.n = x.shape[0] if rows_x is None else rows_x.shape[-1]
    if y is not None:
        d.y, d.ny, d.rows_y = y.data_ptr(), y.shape[0], _p(rows_y)
        d.m = y.shape[0] if rows_y is None else rows_y.shape[-1]
    return d


def feature_moments(x: torch.Tensor, rows: Optional[torch.Tensor] = None) -> FeatureMoments:
    """Mean and unbiased covariance of the feature vectors ``x`` [n, D] (float32 or float64 device tensor; float32 is widened exactly),
    or of its rows ``rows`` (int [r], read in place; repeats allowed): ``FeatureMoments(mean, cov)`` in float64, every sum sequential in
    row order, so runs repeat bitwise.  At least 2 rows.  Nothing is read back."""
    x = _features(x, "x", min_rows=1)
    rows = _row_table(rows, "rows", x.device)
    d = _dist_desc(x, rows)
    if d.n < 2:
        raise ValueError(f"x has {d.n} rows, at least 2 are needed for a covariance")
    mean = torch.empty(d.dim, dtype=torch.float64, device=x.device)
    cov = torch.empty(d.dim, d.dim, dtype=torch.float64, device=x.device)
    d.mean, d.cov = mean.data_ptr(), cov.data_ptr()
    check(lib().dm3d_feature_moments(C.byref(d), _st()), "feature_moments")
    return FeatureMoments(mean, cov)


def knn_radius(x: torch.Tensor, k: int = 5, rows: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The squared Euclidean distance of every row of ``x`` [n, D] to its ``k``-th nearest neighbour in the same set, float64 [n], by
    the ``prdc`` package's rule: the (k + 1)-th smallest entry of the row of the set's own distance matrix, itself included, so a
    duplicated row is a neighbour at distance 0.  1 <= k <= 16 and k < n.  No square root is taken.  Nothing is read back."""
    x = _features(x, "x", min_rows=1)
    rows = _row_table(rows, "rows", x.device)
    d = _dist_desc(x, rows)
    if int(k) != k or not 1 <= k <= _lib.DIST_MAX_K:
        raise ValueError(f"k must be an integer from 1 to {_lib.DIST_MAX_K}, got {k!r}")
    if k >= d.n:
        raise ValueError(f"k={k} needs more than k rows, the set has {d.n}: lower k or add samples")
    radius = torch.empty(d.n, dtype=torch.float64, device=x.device)
    d.k, d.radius = int(k), radius.data_ptr()
    check(lib().dm3d_knn_radius(C.byref(d), _st()), "knn_radius")
    return radius


def prdc_counts(real: torch.Tensor, fake: torch.Tensor, radius_real: torch.Tensor, radius_fake: torch.Tensor, *, rows_real=None,
                rows_fake=None) -> PrdcCounts:
    """The integers behind precision, recall, density and coverage of generated features ``fake`` [M, D] against real features
    ``real`` [N, D], given both sets' ``knn_radius`` (squared, float64 [N] and [M]): ``PrdcCounts(count_fake, near_real, cover_real)``,
    every comparison a strict < on squared distances, as in the ``prdc`` package.  The N x M distances are never stored.  Nothing is
    read back."""
    real, fake = _feature_pair(real, fake, 1)
    rows_real, rows_fake = _row_table(rows_real, "rows_real", real.device), _row_table(rows_fake, "rows_fake", real.device)
    d = _dist_desc(real, rows_real, fake, rows_fake)
    for t, name, n in ((radius_real, "radius_real", d.n), (radius_fake, "radius_fake", d.m)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float64 or tuple(t.shape) != (n,) or not t.is_cuda or not t.is_contiguous():
            raise ValueError(f"{name} must be a contiguous float64 device tensor [{n}], what knn_radius returns for that set")
    count = torch.empty(d.m, dtype=torch.int32, device=real.device)
    near = torch.empty(d.n, dtype=torch.int32, device=real.device)
    cover = torch.empty(d.n, dtype=torch.int32, device=real.device)
    d.radius_x, d.radius_y = radius_real.data_ptr(), radius_fake.data_ptr()
    d.count_y, d.near_x, d.cover_x = count.data_ptr(), near.data_ptr(), cover.data_ptr()
    check(lib().dm3d_prdc_counts(C.byref(d), _st()), "prdc_counts")
    return PrdcCounts(count, near, cover)


def poly_mmd(real: torch.Tensor, fake: torch.Tensor, rows_real: Optional[torch.Tensor] = None, rows_fake: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The three sums the unbiased MMD^2 needs under KID's kernel k(a, b) = (a . b / D + 1)^3, for S subsets at once: float64 [S, 3] =
    (sum_{i != j} k(x_i, x_j), sum_{i != j} k(y_i, y_j), sum_{i, j} k(x_i, y_j)).  ``rows_real`` [S, n] and ``rows_fake`` [S, m] (int,
    read in place) pick each subset's rows; None takes the whole set, and with both None S = 1.  Dot products, row sums and their
    sum run in index order: runs repeat bitwise.  Other kernels are not offered.  Nothing is read back."""
    real, fake = _feature_pair(real, fake)
    rows_real = _row_table(rows_real, "rows_real", real.device, True)
    rows_fake = _row_table(rows_fake, "rows_fake", real.device, True)
    subsets = {t.shape[0] for t in (rows_real, rows_fake) if t is not None}
    if len(subsets) > 1:
        raise ValueError(f"rows_real and rows_fake must list the same number of subsets, got {rows_real.shape[0]} and {rows_fake.shape[0]}")
    d = _dist_desc(real, rows_real, fake, rows_fake)
    d.subsets = subsets.pop() if subsets else 1
    if d.subsets < 1 or d.subsets > _lib.DIST_MAX_SUBSETS:
        raise ValueError(f"1 to {_lib.DIST_MAX_SUBSETS} subsets are taken, got {d.subsets}: split the call")
    if d.n < 2 or d.m < 2:
        raise ValueError(f"a subset needs at least 2 rows of each set, got {d.n} and {d.m}")
    sums = torch.empty(d.subsets, 3, dtype=torch.float64, device=real.device)
    work = torch.empty(d.subsets * (2 * d.n + d.m), dtype=torch.float64, device=real.device)
    d.sums, d.work, d.work_elems = sums.data_ptr(), work.data_ptr(), work.numel()
    check(lib().dm3d_poly_mmd(C.byref(d), _st()), "poly_mmd")
    del work                                                                    # alive until the launches are enqueued (same stream)
    return sums


# ---- fitting the VQ codebook (include/dm3d.h, dm3d_codebook_desc): per-code statistics, usage, EMA update, dead-code replacement ---------
class CodeStats(NamedTuple):
    """What dm3d_code_stats leaves: ``counts`` int32 [K]; ``sums`` float64 [K, D], each code's member rows added in ascending row order;
    ``invalid`` int32 [1], the rows whose index lies outside [0, K)."""
    counts: torch.Tensor
    sums: torch.Tensor
    invalid: torch.Tensor


class CodeUsage(NamedTuple):
    """What dm3d_code_usage leaves: ``perplexity`` 0-d float64 and ``active`` 0-d int32, the number of codes with a member."""
    perplexity: torch.Tensor
    active: torch.Tensor


class Replaced(NamedTuple):
    """What dm3d_codebook_replace reports, both 0-d int32 device tensors."""
    used_count: torch.Tensor
    unused_count: torch.Tensor


def _dev_tensor(t, name: str, dtype, shape, device: bool = True) -> torch.Tensor:
    words = {torch.float32: "float32", torch.float64: "float64", torch.int32: "int32"}[dtype]
    if not isinstance(t, torch.Tensor) or t.dtype != dtype or tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name} must be a {words} tensor {list(shape)}, got {getattr(t, 'dtype', type(t).__name__)} {list(getattr(t, 'shape', ()))}")
    if device and (not t.is_cuda or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous device tensor: the codebook kernels have no CPU path")
    return t


def _codebook_shape(k, dim) -> None:
    if not 1 <= k <= _lib.CODEBOOK_MAX_K:
        raise ValueError(f"K={k} codes; 1 to {_lib.CODEBOOK_MAX_K} are taken")
    if not 4 <= dim <= _lib.CODEBOOK_MAX_DIM or dim % 4:
        raise ValueError(f"D={dim}; a multiple of 4 from 4 to {_lib.CODEBOOK_MAX_DIM} is taken")


def code_stats(z: torch.Tensor, idx: torch.Tensor, num_codes: int) -> CodeStats:
    """Per-code member count and float64 member sum of the latent rows ``z`` [rows, D] (float32) under the assignment ``idx`` [rows]
    (int32, what ``vq_assign`` returns): ``CodeStats(counts, sums, invalid)``.  A code's sum adds its member rows in ascending row
    order, one at a time, with no atomic, so it depends on ``z`` and ``idx`` alone and runs repeat bitwise (``index_add_`` does not
    promise that).  An index outside [0, num_codes) counts in ``invalid`` and nowhere else.  Nothing is read back."""
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float32:
        raise ValueError(f"z must be a float32 tensor [rows, D], got {getattr(z, 'dtype', type(z).__name__)} {list(getattr(z, 'shape', ()))}")
    rows, dim = z.shape
    _codebook_shape(int(num_codes), dim)
    if not 1 <= rows <= _lib.CODEBOOK_MAX_ROWS:
        raise ValueError(f"z has {rows} rows; 1 to {_lib.CODEBOOK_MAX_ROWS} are taken")
    _dev_tensor(z, "z", torch.float32, (rows, dim))
    _dev_tensor(idx, "idx", torch.int32, (rows,))
    d = _lib.CodebookDesc()
    counts = torch.empty(num_codes, dtype=torch.int32, device=z.device)
    sums = torch.empty(num_codes, dim, dtype=torch.float64, device=z.device)
    invalid = torch.empty(1, dtype=torch.int32, device=z.device)
    d.z, d.idx, d.rows, d.dim, d.k = z.data_ptr(), idx.data_ptr(), rows, dim, int(num_codes)
    d.counts, d.sums, d.invalid = counts.data_ptr(), sums.data_ptr(), invalid.data_ptr()
    check(lib().dm3d_code_stats(C.byref(d), _st()), "code_stats")
    return CodeStats(counts, sums, invalid)


def code_usage(counts: torch.Tensor, rows: int, eps: float = 1e-10, used_accum: Optional[torch.Tensor] = None) -> CodeUsage:
    """Perplexity ``exp(-sum p log(p + eps))``, ``p = counts / rows``, summed in float64 over ascending code, and the number of codes
    with a member: ``CodeUsage(perplexity, active)``.  ``used_accum`` (int32 [K]), when given, is incremented by ``counts`` in place
    (NSVQ's ``codebooks_used``).  log and exp are the library's own stated operations, so the value repeats bitwise.  Nothing is read back."""
    if not isinstance(counts, torch.Tensor) or counts.dim() != 1:
        raise ValueError("counts must be an int32 tensor [K]")
    k = counts.shape[0]
    _codebook_shape(k, 4)
    if int(rows) != rows or not 1 <= rows <= _lib.CODEBOOK_MAX_ROWS:
        raise ValueError(f"rows must be an integer from 1 to {_lib.CODEBOOK_MAX_ROWS}, got {rows!r}")
    if not eps >= 0:
        raise ValueError(f"eps must be at least 0, got {eps!r}")
    _dev_tensor(counts, "counts", torch.int32, (k,))
    if used_accum is not None:
        _dev_tensor(used_accum, "used_accum", torch.int32, (k,))
    out = torch.empty(1, dtype=torch.float64, device=counts.device)
    active = torch.empty(1, dtype=torch.int32, device=counts.device)
    d = _lib.CodebookDesc()
    d.counts, d.rows, d.k, d.eps = counts.data_ptr(), int(rows), k, float(eps)
    d.perplexity, d.active, d.used_accum = out.data_ptr(), active.data_ptr(), _p(used_accum)
    check(lib().dm3d_code_usage(C.byref(d), _st()), "code_usage")
    return CodeUsage(out[0], active[0])


def _codebook_state(d, codebook, esq, cluster_size, ema_w, optional=False):
    if not isinstance(codebook, torch.Tensor) or codebook.dim() != 2:
        raise ValueError("codebook must be a float32 tensor [K, D] (rows are codes, the layout vq_assign reads)")
    k, dim = codebook.shape
    _codebook_shape(k, dim)
    both = not optional or cluster_size is not None or ema_w is not None
    if both and (cluster_size is None or ema_w is None):
        raise ValueError("cluster_size and ema_w are given together or not at all")
    for device in (False, True):                                       # every shape before the first device check
        _dev_tensor(codebook, "codebook", torch.float32, (k, dim), device)
        _dev_tensor(esq, "esq", torch.float32, (k,), device)
        if both:
            _dev_tensor(cluster_size, "cluster_size", torch.float32, (k,), device)
            _dev_tensor(ema_w, "ema_w", torch.float32, (k, dim), device)
    d.k, d.dim, d.codebook, d.esq, d.cluster_size, d.ema_w = k, dim, codebook.data_ptr(), esq.data_ptr(), _p(cluster_size), _p(ema_w)
    return k, dim


def codebook_ema(codebook: torch.Tensor, esq: torch.Tensor, cluster_size: torch.Tensor, ema_w: torch.Tensor, counts: torch.Tensor,
                 sums: torch.Tensor, decay: float = 0.99, epsilon: float = 1e-5) -> None:
    """The reference's VectorQuantizerEMA update (emavqvae.py:213-222) in one launch, in place on ``cluster_size`` [K], ``ema_w`` [K, D],
    ``codebook`` [K, D] and ``esq`` [K] (float32), from ``code_stats``' ``counts`` and ``sums``: N' = N decay + (1 - decay) count,
    W' = W decay + (1 - decay) sum, codebook = W' / N' * n / (n + epsilon) with n = sum N'.  A code whose N' is exactly 0 keeps its row
    and its esq (the literal rule divides by zero there).  Nothing is read back."""
    d = _lib.CodebookDesc()
    k, dim = _codebook_state(d, codebook, esq, cluster_size, ema_w)
    if not 0.0 <= decay <= 1.0:
        raise ValueError(f"decay must lie in [0, 1], got {decay!r}")
    if not epsilon >= 0:
        raise ValueError(f"epsilon must be at least 0, got {epsilon!r}")
    _dev_tensor(counts, "counts", torch.int32, (k,))
    _dev_tensor(sums, "sums", torch.float64, (k, dim))
    d.counts, d.sums, d.decay, d.epsilon = counts.data_ptr(), sums.data_ptr(), float(decay), float(epsilon)
    check(lib().dm3d_codebook_ema(C.byref(d), _st()), "codebook_ema")


def codebook_replace(codebook: torch.Tensor, esq: torch.Tensor, used: torch.Tensor, num_batches: int, threshold: float = 0.01, *,
                     seed: int = 0, draw: int = 0, noise_scale: float = 1e-12, cluster_size: Optional[torch.Tensor] = None,
                     ema_w: Optional[torch.Tensor] = None) -> Replaced:
    """NSVQ.replace_unused_codebooks (nsvqvae.py:193-230) with no host read, in place: a code is unused where
    ``used / num_batches < threshold``; the j-th unused code takes the row of the j-th used code (of the j-th entry of the tiled and
    shuffled used list where fewer codes are used than unused) plus ``noise_scale`` * N(0,1); with no used code every row gets the
    noise alone.  ``esq`` of the rewritten rows is recomputed, ``used`` is zeroed, and ``cluster_size`` / ``ema_w``, when given, copy
    the source's entries.  Shuffle and noise are Philox draws keyed by ``seed`` and ``draw`` (count the replacements in ``draw``), so a
    call repeats bitwise.  Returns ``Replaced(used_count, unused_count)`` on the device."""
    d = _lib.CodebookDesc()
    k, dim = _codebook_state(d, codebook, esq, cluster_size, ema_w, optional=True)
    _dev_tensor(used, "used", torch.int32, (k,))
    if int(num_batches) != num_batches or num_batches < 1:
        raise ValueError(f"num_batches must be an integer of at least 1, got {num_batches!r}")
    if not math.isfinite(noise_scale) or math.isnan(threshold):
        raise ValueError("noise_scale must be finite and threshold a number")
    out = torch.empty(2, dtype=torch.int32, device=codebook.device)
    work = torch.empty(k, dtype=torch.int32, device=codebook.device)
    d.used, d.num_batches, d.threshold, d.noise_scale = used.data_ptr(), int(num_batches), float(threshold), float(noise_scale)
    d.seed, d.draw = int(seed) & (2 ** 64 - 1), int(draw) & 0x7FFFFFFF
    d.used_count, d.unused_count, d.map = out.data_ptr(), out.data_ptr() + 4, work.data_ptr()
    check(lib().dm3d_codebook_replace(C.byref(d), _st()), "codebook_replace")
    del work                                                                    # alive until the launches are enqueued (same stream)
    return Replaced(out[0], out[1])
