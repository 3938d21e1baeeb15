"""ORACLE (kernel by kernel) — plain float64 restatements of the training and normalisation entries of the C ABI, one function per
entry, written from the comments of ``include/dm3d.h``.

TEST INFRASTRUCTURE ONLY: the product never imports it.  Every backward formula exists twice: the closed form the header states
(``*_bwd``) and ``torch.autograd`` applied to the float64 forward (``*_bwd_autograd``); ``tests/test_ref_kernels.py`` holds the two
against each other, ``tests/test_gpu_train_kernels.py`` holds the HIP kernels against the closed forms.
The last section restates the inference entries (conv, GEMM, attention, the fused attention-block kernels, the DDPM update) for
``tests/test_gpu_infer_kernels.py``, on top of the layer functions of ``oracle/ref_torch.py``.
After it come the sampler entries (the DDIM / DPM-Solver++ / stochastic DPM-Solver++ updates, the dynamic threshold, the edit blend, the
guidance, pred_to_eps and the objective loss) for ``tests/test_gpu_sampler_kernels.py``: numpy, each with an ``order`` switch between
the header's individually rounded float32 operations (the kernels match it bit for bit) and the same formula in float64.

Tensors are torch float64 unless a function says otherwise; the data-movement entries are numpy and keep the dtype they are given
(they are compared bitwise).
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

ACT_NONE, ACT_RELU, ACT_SILU = 0, 1, 2


def f64(a) -> torch.Tensor:
    return torch.as_tensor(np.asarray(a) if not torch.is_tensor(a) else a).double()


# ---- activations -----------------------------------------------------------------------------------------------------------------
def act(u, kind):
    if kind == ACT_RELU:
        return torch.relu(u)
    if kind == ACT_SILU:
        return u * torch.sigmoid(u)
    return u


def act_grad(u, kind):
    """d act(u) / du; ReLU'(0) = 0."""
    if kind == ACT_RELU:
        return (u > 0).to(u.dtype)
    if kind == ACT_SILU:
        s = torch.sigmoid(u)
        return s * (1 + u * (1 - s))
    return torch.ones_like(u)


def act_bwd(ref, dy, kind):
    return dy * act_grad(ref, kind)


def act_bwd_autograd(ref, dy, kind):
    u = ref.clone().requires_grad_(True)
    act(u, kind).backward(dy)
    return u.grad


# ---- BatchNormalization(training=True) ---------------------------------------------------------------------------------------------
def moments_acc(x):
    """acc[b][c][0..1] = (sum, sum of squares) of x[b, :, c]: what dm3d_groupnorm_stats leaves.  x [batch, voxels, c]."""
    return torch.stack([x.sum(1), (x * x).sum(1)], -1)


def batchnorm_finalize(acc, voxels, eps, gamma, beta, moving_mean=None, moving_var=None, momentum=0.99, unbiased_moving=1):
    """acc [batch][c][2] -> scale, shift, mean, rstd (and the moving averages when given)."""
    n = acc.shape[0] * voxels
    mean = acc[..., 0].sum(0) / n
    var = (acc[..., 1].sum(0) / n - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    scale = gamma * rstd
    shift = beta - mean * scale
    out = [scale, shift, mean, rstd]
    if moving_mean is not None:
        vmov = var * (n / (n - 1.0)) if (unbiased_moving and n > 1) else var
        out += [moving_mean * momentum + mean * (1 - momentum), moving_var * momentum + vmov * (1 - momentum)]
    return out


def affine_act_cat(x1, x2, scale, shift, kind):
    x = x1 if x2 is None else torch.cat([x1, x2], -1)
    if scale is not None:
        x = x * scale + shift
    return act(x, kind)


def bn_act_bwd(g, x, scale, shift, mean, rstd, kind):
    """Backward of y = act(BatchNorm_train(x)) from the vectors the forward kept.  x, g [rows][c].
    Returns dx, dgamma, dbeta, red [c][2] = (sum du, sum du*xhat)."""
    du = g * act_grad(x * scale + shift, kind)
    xhat = (x - mean) * rstd
    s, sx = du.sum(0), (du * xhat).sum(0)
    n = x.shape[0]
    dx = scale * (du - s / n - xhat * (sx / n))
    return dx, sx, s, torch.stack([s, sx], -1)


def bn_act_fwd(x, gamma, beta, eps, kind):
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    return act((x - mean) / torch.sqrt(var + eps) * gamma + beta, kind)


def bn_act_bwd_autograd(g, x, gamma, beta, eps, kind):
    xr, gr, br = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    bn_act_fwd(xr, gr, br, eps, kind).backward(g)
    return xr.grad, gr.grad, br.grad


# ---- GroupNormalization --------------------------------------------------------------------------------------------------------------
def groupnorm_scale_shift(x, groups, eps, gamma, beta):
    """x [batch, voxels, c] -> per-sample scale[b][c] = gamma*rstd, shift[b][c] = beta - mean*scale (biased group variance)."""
    B, V, Cn = x.shape
    xg = x.reshape(B, V, groups, Cn // groups)
    mean = xg.mean((1, 3))
    var = ((xg * xg).mean((1, 3)) - mean * mean).clamp_min(0)
    rstd = 1 / torch.sqrt(var + eps)
    gc = Cn // groups
    scale = gamma[None, :] * rstd.repeat_interleave(gc, 1)
    shift = beta[None, :] - mean.repeat_interleave(gc, 1) * scale
    return scale, shift


def groupnorm_partials(x):
    """part[b][slot][c][2] = (sum, sum of squares) over the 64 voxels of a slot, slots = ceil(voxels / 64)."""
    B, V, Cn = x.shape
    slots = -(-V // 64)
    xp = torch.zeros(B, slots * 64, Cn, dtype=x.dtype)
    xp[:, :V] = x
    xp = xp.reshape(B, slots, 64, Cn)
    return torch.stack([xp.sum(2), (xp * xp).sum(2)], -1)


def affine_act_batched(x, scale, shift, kind):
    """x [batch, rows, c], scale / shift [batch, c]."""
    return act(x * scale[:, None, :] + shift[:, None, :], kind)


# ---- Conv3D / Dense weight gradient, column sums, flipped kernel ---------------------------------------------------------------------
def wgrad(a, g, ksize):
    """dw[tap][ci][co] = sum over samples and voxels of a[voxel + tap - 1][ci] * g[voxel][co] with zero padding.
    a [B, D, H, W, cin], g [B, D, H, W, cout] -> [ksize^3, cin, cout] (tap = (dz*3 + dy)*3 + dx)."""
    if ksize == 1:
        return (a.reshape(-1, a.shape[-1]).T @ g.reshape(-1, g.shape[-1]))[None]
    B, D, H, W, _ = a.shape
    ap = F.pad(a, (0, 0, 1, 1, 1, 1, 1, 1))
    taps = []
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                taps.append(torch.einsum("bzyxi,bzyxo->io", ap[:, dz:dz + D, dy:dy + H, dx:dx + W], g))
    return torch.stack(taps)


def _conv_same(x, kernel):
    """Conv3D(padding="same", stride 1) as cross-correlation, kernel [k, k, k, cin, cout]."""
    k = kernel.shape[0]
    y = F.conv3d(x.permute(0, 4, 1, 2, 3), kernel.permute(4, 3, 0, 1, 2), None, padding=k // 2)
    return y.permute(0, 2, 3, 4, 1)


def wgrad_autograd(a, g, ksize):
    w = torch.zeros(ksize, ksize, ksize, a.shape[-1], g.shape[-1], dtype=a.dtype, requires_grad=True)
    _conv_same(a, w).backward(g)
    return w.grad.reshape(ksize ** 3, a.shape[-1], g.shape[-1])


def colsum(x, groups):
    """x [groups*rows][c] -> [groups][c]."""
    return x.reshape(groups, -1, x.shape[-1]).sum(1)


def colsum_autograd(x, groups):
    """The gradient of a per-group vector added to every row of its group."""
    v = torch.zeros(groups, x.shape[-1], dtype=x.dtype, requires_grad=True)
    (x.reshape(groups, -1, x.shape[-1]) + v[:, None, :]).backward(x.reshape(groups, -1, x.shape[-1]))
    return v.grad


def flip_transpose(w):
    """numpy [taps][cin][cout] -> [taps][cout][cin] with the taps reversed."""
    return np.ascontiguousarray(w[::-1].transpose(0, 2, 1))


def conv_dgrad_autograd(x, kernel, g):
    xr = x.clone().requires_grad_(True)
    _conv_same(xr, kernel).backward(g)
    return xr.grad


# ---- LayerNormalization / softmax backward ------------------------------------------------------------------------------------------
def layernorm_bwd(x, gamma, dy, eps):
    mean = x.mean(-1, keepdim=True)
    var = x.var(-1, unbiased=False, keepdim=True)
    rstd = 1 / torch.sqrt(var + eps)
    xhat = (x - mean) * rstd
    dg = dy * gamma
    dx = rstd * (dg - dg.mean(-1, keepdim=True) - xhat * (dg * xhat).mean(-1, keepdim=True))
    return dx, (dy * xhat).sum(0), dy.sum(0)


def layernorm_bwd_autograd(x, gamma, dy, eps):
    xr, gr = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
    br = torch.zeros_like(gamma, requires_grad=True)
    mean = xr.mean(-1, keepdim=True)
    var = xr.var(-1, unbiased=False, keepdim=True)
    ((xr - mean) / torch.sqrt(var + eps) * gr + br).backward(dy)
    return xr.grad, gr.grad, br.grad


def softmax_bwd(p, dp, scale):
    return scale * p * (dp - (p * dp).sum(-1, keepdim=True))


def softmax_bwd_autograd(logits, dp, scale):
    """p = softmax(scale * logits); returns (p, dL/dlogits)."""
    s = logits.clone().requires_grad_(True)
    p = torch.softmax(scale * s, -1)
    p.backward(dp)
    return p.detach(), s.grad


# ---- data movement (numpy, dtype preserved) --------------------------------------------------------------------------------------------
def upsample2(x):
    """[B, D, H, W, C] -> [B, 2D, 2H, 2W, C], nearest (numpy or torch)."""
    if isinstance(x, np.ndarray):
        return x.repeat(2, 1).repeat(2, 2).repeat(2, 3)
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2).repeat_interleave(2, 3)


def sumpool2_add(dst, y):
    """dst [B, D, H, W, C] + the 8 children of y [B, 2D, 2H, 2W, C], added one at a time in the order (dz, dy, dx) = 000, 001, ... 111
    in the dtype given (numpy or torch)."""
    out = dst
    for k in range(8):
        out = out + y[:, (k >> 2)::2, ((k >> 1) & 1)::2, (k & 1)::2]
    return out


def sumpool2_autograd(y):
    B, D2, H2, W2, Cn = y.shape
    x = torch.zeros(B, D2 // 2, H2 // 2, W2 // 2, Cn, dtype=y.dtype, requires_grad=True)
    upsample2(x).backward(y)
    return x.grad


def dilate2(src, in_extent, off):
    """src [B, od, oh, ow, C] -> zeros [B, id, ih, iw, C] with src[o] at 2*o + off per axis (positions outside are dropped)."""
    B, od, oh, ow, Cn = src.shape
    dst = np.zeros((B,) + tuple(in_extent) + (Cn,), src.dtype)
    nz = min(od, (in_extent[0] - off[0] + 1) // 2)
    ny = min(oh, (in_extent[1] - off[1] + 1) // 2)
    nx = min(ow, (in_extent[2] - off[2] + 1) // 2)
    dst[:, off[0]:off[0] + 2 * nz:2, off[1]:off[1] + 2 * ny:2, off[2]:off[2] + 2 * nx:2] = src[:, :nz, :ny, :nx]
    return dst


def scatter_add_rows(table, idx, src):
    """float64 table[idx[r]] += src[r]; rows with an index outside the table are ignored."""
    out = table.clone()
    for r, t in enumerate(idx.tolist()):
        if 0 <= t < out.shape[0]:
            out[t] += src[r]
    return out


def gather_rows(table, idx):
    return table[np.clip(idx, 0, table.shape[0] - 1)]


def q_sample_f32(lat, noise, t, sqab, sq1ab):
    """float32 numpy, each operation rounded: sqab[t[b]]*lat + sq1ab[t[b]]*noise with t clamped to the table."""
    tt = np.clip(t, 0, len(sqab) - 1)
    shape = (-1,) + (1,) * (lat.ndim - 1)
    a, s = sqab[tt].astype(np.float32).reshape(shape), sq1ab[tt].astype(np.float32).reshape(shape)
    return (a * lat.astype(np.float32)).astype(np.float32) + (s * noise.astype(np.float32)).astype(np.float32)


# ---- loss and optimizer ---------------------------------------------------------------------------------------------------------------
def mse_loss_grad(pred, noise, inv):
    d = pred - noise
    return (d * d).sum() * inv, 2 * d * inv


def mse_loss_grad_autograd(pred, noise, inv):
    p = pred.clone().requires_grad_(True)
    loss = ((noise - p) ** 2).sum() * inv
    loss.backward()
    return loss.detach(), p.grad


def adam(w, g, m, v, lr_t, b1, b2, eps):
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    return w - lr_t * m / (torch.sqrt(v) + eps), m, v


# ---- inference entries (tests/test_gpu_infer_kernels.py) -----------------------------------------------------------------------------------
def conv3d_fused(x1, kernel, *, x2=None, ksize=3, stride=1, upsample=False, transpose=False, bias=None, pro=None, vec=None, vec_idx=None,
                 relu=False, prelu_alpha=None, res=None, relu_out=False, skip=None, post=None):
    """dm3d_conv3d_ndhwc in float64, in the order include/dm3d.h states: prologue silu(x*scale + shift) on concat(x1, x2) (pro = (scale,
    shift), each [c] or per sample [batch, c]), the convolution (Conv3D 'same' k1 / k3 at stride 1 or 2, k4 at stride 2; on the nearest-2x
    upsampled tensor; Conv3DTranspose k4 s2 with a [4,4,4,Cout,Cin] kernel), + bias + vec[vec_idx[b]], ReLU, PReLU (alpha
    [out_d,out_h,out_w,cout]), + res, + the fused 1x1 skip conv of the raw skip = (x, kernel [cin, cout]), ReLU after the add, and the
    consumer's silu(v*scale + shift) (post)."""
    from oracle import ref_torch as rt
    x = f64(x1) if x2 is None else torch.cat([f64(x1), f64(x2)], -1)
    B = x.shape[0]
    if pro is not None:
        s, t = f64(pro[0]), f64(pro[1])
        if s.dim() == 2:
            s, t = s[:, None, None, None, :], t[:, None, None, None, :]
        x = rt._swish(x * s + t)
    k = f64(kernel)
    if transpose:
        y = rt._conv3d_transpose_k4s2(x, k, None)
    elif ksize == 4:
        y = rt._conv3d_k4s2(x, k, None)
    else:
        y = rt._conv3d(rt._upsample2(x) if upsample else x, k, None, stride)
    if bias is not None:
        y = y + f64(bias)
    if vec is not None:
        rows = torch.arange(B) if vec_idx is None else torch.as_tensor(np.asarray(vec_idx)).long()
        y = y + f64(vec)[rows][:, None, None, None, :y.shape[-1]]
    if relu:
        y = torch.relu(y)
    if prelu_alpha is not None:
        y = rt._prelu(y, f64(prelu_alpha))
    if res is not None:
        y = y + f64(res)
    if skip is not None:
        y = y + f64(skip[0]) @ f64(skip[1])
    if relu_out:
        y = torch.relu(y)
    if post is not None:
        y = rt._swish(y * f64(post[0]) + f64(post[1]))
    return y


def gemm_tn(a, b, *, alpha=1.0, bias=None, bias_along_m=False, kind=ACT_NONE, res=None, res2=None):
    """out[b][m][n] = act(alpha * sum_k A[b][m][k] B[b][n][k] + bias) + res + res2; a [batch, m, k], b [batch or 1, n, k]."""
    y = alpha * torch.einsum("bmk,bnk->bmn", f64(a), f64(b).expand(a.shape[0], -1, -1))
    if bias is not None:
        y = y + (f64(bias)[:, None] if bias_along_m else f64(bias))
    y = act(y, kind)
    for r in (res, res2):
        if r is not None:
            y = y + f64(r)
    return y


def attention(q, k, v, scale, res=None):
    """softmax(q k^T * scale) v + res per sample: q [batch, lq, c]; k, v [batch or 1, lk, c].  ref_torch._attention with the factor
    passed (it fixes units^-0.5)."""
    from oracle import ref_torch as rt
    q, k, v = f64(q), f64(k).expand(q.shape[0], -1, -1), f64(v).expand(q.shape[0], -1, -1)
    y = rt._attention(q * (scale * float(q.shape[-1]) ** 0.5), k, v, q.shape[-1])
    return y if res is None else y + f64(res)


def mlp_fused(x, w0, b0, w1, b1, res=None, res2=None, tail=None):
    """Dense_1(relu(Dense_0(x))) + res + res2 with weights [out, in]; tail = (w2, b2, res3): relu(Dense_2(that)) + res3."""
    y = torch.relu(f64(x) @ f64(w0).T + f64(b0)) @ f64(w1).T + f64(b1)
    for r in (res, res2):
        if r is not None:
            y = y + f64(r)
    if tail is not None:
        y = torch.relu(y @ f64(tail[0]).T + f64(tail[1]))
        if tail[2] is not None:
            y = y + f64(tail[2])
    return y


def layernorm(x, gamma, beta, eps):
    x = f64(x)
    return F.layer_norm(x, (x.shape[-1],), f64(gamma), f64(beta), eps)


def attn_front(x, w_in, b_in, w_qk, b_qk, w_v, b_v, norms, eps):
    """dm3d_attn_front: y = relu(x W_in^T + b_in), n_i = LayerNormalization_i(y), q|k = n1 W_qk^T + b_qk, v^T, q2 = n2 W_qk[:u]^T + b_qk[:u], n3."""
    u = f64(w_in).shape[0]
    y = torch.relu(f64(x) @ f64(w_in).T + f64(b_in))
    n1, n2, n3 = (layernorm(y, g, b, eps) for g, b in norms)
    return dict(y=y, qk=n1 @ f64(w_qk).T + f64(b_qk), vt=(n1 @ f64(w_v).T + f64(b_v)).T.contiguous(),
                q2=n2 @ f64(w_qk)[:u].T + f64(b_qk)[:u], n3=n3)


def affine_act(x, scale, shift, kind):
    u = f64(x)
    if scale is not None:
        u = u * f64(scale) + f64(shift)
    return act(u, kind)


def vq_assign_f32(z, sim, esq):
    """float32 numpy, each operation rounded, in the header's order: argmin_k (|z_r|^2 + esq[k]) - 2*sim[r][k], lowest index on ties.
    |z_r|^2 is the float64 sum rounded once (the kernel's summation order is its own: callers keep candidates apart or exactly tied)."""
    zz = (np.asarray(z, np.float64) ** 2).sum(-1).astype(np.float32)
    d = (zz[:, None] + np.asarray(esq, np.float32)[None, :]).astype(np.float32) - (np.float32(2) * np.asarray(sim, np.float32)).astype(np.float32)
    return np.argmin(d, -1).astype(np.int32), d


def ddpm_update(tables, x, eps, t, noise=None):
    """dm3d_ddpm_update in float64 on the float32 tables (a ref_torch.Betas): (mean, var) of mode 0 and the mode-1 state
    clip(mean) + sqrt(max(var, 1e-20)) * z with z = 0 where t == 0; t is clamped to the tables first."""
    from oracle import ref_torch as rt

    class _T:
        pass
    tab = _T()
    for n in rt.Betas.NAMES:
        setattr(tab, n, f64(getattr(tables, n)))
    tt = torch.as_tensor(np.clip(np.asarray(t), 0, len(tab.beta) - 1)).long()
    x5 = f64(x).reshape(x.shape[0], 1, 1, 1, -1)
    e5 = f64(eps).reshape(x5.shape)
    mean, var = rt.ddpm_sample(tab, x5, e5, tt)
    step = None
    if noise is not None:
        z = f64(noise).reshape(x5.shape) * (tt > 0).double().reshape(-1, 1, 1, 1, 1)
        step = rt.ddpm_step(tab, x5, e5, tt, z).reshape(x.shape)
    return mean.reshape(x.shape), var.reshape(-1), step


# ---- the sampler entries (tests/test_gpu_sampler_kernels.py) --------------------------------------------------------------------------
# numpy, [batch, per_sample] arrays and the raw tables the descriptors point to.  order="f32": every operation the header lists is one
# numpy operation on float32 operands, so each is rounded on its own, in the header's order (IEEE add, sub, mul and div are correctly
# rounded on either side: the result is the kernel's bit for bit).  order="f64": the same formula on the same float32 table values in
# float64.  Branches are taken on the table values, as the kernels take them; a value a branch does not read is never mixed in.
def _dt(order):
    return {"f32": np.float32, "f64": np.float64}[order]


def _rows_of(pos, rows):
    return np.clip(np.asarray(pos, np.int64), 0, rows - 1)


def _col(table, r, c, dt):
    """Column c of the rows r of a table, as a [batch, 1] array of dt."""
    return np.asarray(table)[r, c].astype(dt).reshape(-1, 1)


def x0_estimate(x, p, coef, pos, frame=None, order="f32"):
    """The raw x0 estimate and the model's eps of the update kernels.  Without a frame: x0 = (x - sqrt(1-a)*p) / sqrt(a) (mul, sub, div),
    eps = p.  With a frame row (k0x, k0p, kex, kep): x0 = k0x*x + k0p*p, eps = kex*x + kep*p (mul, mul, add each)."""
    dt = _dt(order)
    r = _rows_of(pos, len(coef))
    x, p = np.asarray(x).astype(dt), np.asarray(p).astype(dt)
    with np.errstate(all="ignore"):
        if frame is None:
            return (x - _col(coef, r, 1, dt) * p) / _col(coef, r, 0, dt), p
        return (_col(frame, r, 0, dt) * x + _col(frame, r, 1, dt) * p, _col(frame, r, 2, dt) * x + _col(frame, r, 3, dt) * p)


def x0_bounded(x0, clip, bound=None):
    """clamp(x0, -1, 1) on the rows with clip, or clamp(x0, -s, s) / s with the dynamic bound s [batch]; a NaN passes."""
    dt = x0.dtype.type
    clip = np.asarray(clip, bool).reshape(-1, 1)
    with np.errstate(all="ignore"):
        if bound is None:
            lim = np.minimum(np.maximum(x0, dt(-1)), dt(1))
        else:
            s = np.asarray(bound).astype(dt).reshape(-1, 1)
            lim = np.minimum(np.maximum(x0, -s), s) / s
    return np.where(clip, lim, x0)


def ddim_update(x, eps, coef, pos, noise=None, frame=None, x0_bound=None, order="f32"):
    """dm3d_ddim_update[_frame]: res = (a_x0*x0 + a_eps*eps) + sigma*z with z = noise where the row's sigma != 0 and 0 elsewhere."""
    dt = _dt(order)
    r = _rows_of(pos, len(coef))
    x0, ek = x0_estimate(x, eps, coef, pos, frame, order)
    x0 = x0_bounded(x0, np.asarray(coef)[r, 5] != 0, x0_bound)
    sigma = _col(coef, r, 4, dt)
    z = np.zeros_like(x0) if noise is None else np.where(sigma != 0, np.asarray(noise).astype(dt), dt(0))
    with np.errstate(all="ignore"):
        return (_col(coef, r, 2, dt) * x0 + _col(coef, r, 3, dt) * ek) + sigma * z


def dpm_sde_update(x, eps, coef, pos, hist=None, noise=None, frame=None, x0_bound=None, order="f32"):
    """dm3d_dpm_sde_update[_frame]: (res, x0) with res = ((c_x*x + c_0*x0) + c_1*hist) + c_z*z; the hist add only where c_1 != 0 and a
    history is given, the noise add only where c_z != 0 (column 6)."""
    dt = _dt(order)
    r = _rows_of(pos, len(coef))
    x0, _ = x0_estimate(x, eps, coef, pos, frame, order)
    x0 = x0_bounded(x0, np.asarray(coef)[r, 5] != 0, x0_bound)
    c_1, c_z = _col(coef, r, 4, dt), (_col(coef, r, 6, dt) if noise is not None else None)
    with np.errstate(all="ignore"):
        res = _col(coef, r, 2, dt) * np.asarray(x).astype(dt) + _col(coef, r, 3, dt) * x0
        if hist is not None:
            res = np.where(c_1 != 0, res + c_1 * np.asarray(hist).astype(dt), res)
        if noise is not None:
            res = np.where(c_z != 0, res + c_z * np.asarray(noise).astype(dt), res)
    return res, x0


def dpm_update(x, eps, coef, pos, hist=None, frame=None, x0_bound=None, order="f32"):
    """dm3d_dpm_update[_frame]: (res, x0) with res = (c_x*x + c_0*x0) + c_1*hist; column 6 is not read."""
    return dpm_sde_update(x, eps, coef, pos, hist, None, frame, x0_bound, order)


def x0_bound(x, eps, coef, pos, rank, frac, smax, frame=None, order="f32"):
    """dm3d_x0_threshold: bound[b] = s from the sorted magnitudes of the raw x0 estimate (np.sort: a NaN last); 1 on rows with clip == 0."""
    dt = _dt(order)
    r = _rows_of(pos, len(coef))
    x0, _ = x0_estimate(x, eps, coef, pos, frame, order)
    out = np.ones(len(r), dt)
    n = x0.shape[1]
    for b in range(len(r)):
        if np.asarray(coef)[r[b], 5] == 0:
            continue
        v = np.sort(np.abs(x0[b]))
        i = int(np.clip(int(rank[b]), 0, n - 1))
        v0, v1 = v[i], v[min(i + 1, n - 1)]
        with np.errstate(all="ignore"):
            raw = v0 + dt(frac[b]) * (v1 - v0)
        out[b] = raw if np.isnan(raw) else min(max(raw, dt(1)), dt(smax[b]))
    return out


def edit_update(x0, levels, pos, noise, mode=0, x=None, w=None, channels=1, order="f32"):
    """dm3d_edit_update: known_t = sqrt(a')*x0 + sqrt(1-a')*z (x0 itself where sqrt(1-a') == 0); mode 1 blends it into x with the
    per-voxel weight w [batch, per_sample / channels]: x where w == 0, known_t where w == 1, w*known_t + (1-w)*x between."""
    dt = _dt(order)
    r = _rows_of(pos, len(levels))
    x0 = np.asarray(x0).astype(dt)
    sq1 = _col(levels, r, 1, dt)
    with np.errstate(all="ignore"):
        known = np.where(sq1 == 0, x0, _col(levels, r, 0, dt) * x0 + sq1 * np.asarray(noise).astype(dt))
        if mode == 0:
            return known
        we = np.repeat(np.asarray(w).astype(dt), channels, axis=1)
        x = np.asarray(x).astype(dt)
        return np.where(we == 0, x, np.where(we == 1, known, we * known + (dt(1) - we) * x))


def guide_update(eps_pos, eps_neg, scale, rescale=None, order="f32"):
    """dm3d_guide_update modes 0 and 1: (eps_g, f, out).  eps_g = eps_neg + w*(eps_pos - eps_neg) (sub, mul, add), eps_pos at w == 1 and
    eps_neg at w == 0; f[b] = phi*std(eps_pos)/std(eps_g) + (1 - phi) from float64 sums of the values and their squares (1 where
    std(eps_g) == 0), rounded once to float32 at order="f32"; out = f*eps_g on the rows with phi != 0, eps_g itself elsewhere."""
    dt = _dt(order)
    ep, en = np.asarray(eps_pos).astype(dt), np.asarray(eps_neg).astype(dt)
    w = np.asarray(scale).astype(dt).reshape(-1, 1)
    with np.errstate(all="ignore"):
        g = np.where(w == 1, ep, np.where(w == 0, en, en + w * (ep - en)))
    phi = np.zeros(len(w)) if rescale is None else np.asarray(rescale).astype(np.float64)
    n = float(ep.shape[1])
    f = np.ones(len(w), np.float64)
    out = g.copy()
    for b in np.nonzero(phi != 0)[0]:
        a, c = ep[b].astype(np.float64), g[b].astype(np.float64)
        var_p = max(float((a * a).sum()) / n - (float(a.sum()) / n) ** 2, 0.0)
        var_g = max(float((c * c).sum()) / n - (float(c.sum()) / n) ** 2, 0.0)
        f[b] = 1.0 if var_g == 0.0 else phi[b] * np.sqrt(var_p / var_g) + (1.0 - phi[b])
        out[b] = dt(f[b]) * g[b]
    return g, f.astype(dt), out


def pred_to_eps(pred, x, table, t_idx, order="f32"):
    """dm3d_pred_to_eps: eps = c_p*pred + c_x*x (mul, mul, add) with (c_p, c_x) = table[clamp(t_idx[b])]."""
    dt = _dt(order)
    r = _rows_of(t_idx, len(table))
    with np.errstate(all="ignore"):
        return _col(table, r, 0, dt) * np.asarray(pred).astype(dt) + _col(table, r, 1, dt) * np.asarray(x).astype(dt)


def objective_loss(pred, noise, x0, coef, inv, want_dpred=True, order="f32"):
    """dm3d_objective_loss_grad: (dpred, loss_rows, loss).  d = pred - (a_z*noise + a_0*x0); dpred = d * (float)(2*inv*w);
    loss_rows[b] = w*inv*sum d^2 in float64; loss = their sum in index order."""
    dt = _dt(order)
    coef = np.asarray(coef)
    rows = np.arange(len(coef))
    d = np.asarray(pred).astype(dt) - (_col(coef, rows, 0, dt) * np.asarray(noise).astype(dt) + _col(coef, rows, 1, dt) * np.asarray(x0).astype(dt))
    w = coef[:, 2].astype(np.float64)
    dpred = d * (2.0 * inv * w).astype(dt).reshape(-1, 1) if want_dpred else None
    loss_rows = w * inv * (d.astype(np.float64) ** 2).sum(1)
    loss = 0.0
    for v in loss_rows:
        loss += float(v)
    return dpred, loss_rows, loss
