// dm3d_unipc.hip — the UniPC update (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion
// Models"; the data-prediction multistep form): the corrector at the level the U-Net has just been evaluated at and the predictor to
// the next level, in one launch.  Every per-step constant comes from two coefficient tables the host writes once per chain (include/dm3d.h,
// dm3d_unipc_desc), so rows of order 1, 2 and 3, either variant, rows without a corrector and the step to the clean sample share one
// kernel.  A pure HBM stream like dpm_kernel: 16 B per lane; read x, eps and whatever of the corrected state and of the three history
// slots the row's coefficients name, write the x0 estimate, the corrected state and the predicted one.  No noise term: no Philox.
// The row, the estimate and the descriptor rules are dm3d_update.h's, shared with the DDIM and DPM-Solver++ kernels.
#include "dm3d_update.h"

namespace {

struct unipc_args {
    float* x; const float* eps; float* xc; float* hist[3]; float* out; float* xc_out; float* x0_out;
    long per4;                                     // float4 per sample
    const float* coef; const float* corr; const int* t_next; int rows;
    const int* pos; int* t_idx;
    int mode;
    const float* x0_bound;
};

__device__ __forceinline__ f32x4 load4(const float* p, long i) { return reinterpret_cast<const f32x4*>(p)[i]; }

__global__ __launch_bounds__(256) void unipc_kernel(const unipc_args p) {
    const int b = blockIdx.y;
    const dm3d_row w = dm3d_row_decode<false>(p.coef, nullptr, p.pos, p.rows, p.x0_bound, b);
    const f32x4 k = reinterpret_cast<const f32x4*>(p.corr)[2 * w.r];
    const float k_t = reinterpret_cast<const f32x4*>(p.corr)[2 * w.r + 1][0];
    const float p_x = w.c0[2], p_0 = w.c0[3], p_1 = w.c1[0], p_2 = w.c1[2];
    const int rot = min(max((int)w.c1[3], 0), 2);
    // which slot plays which role at this row (uniform over the block): the newest estimate sits one slot behind the one written
    // (selects between constant indices: a run-time index into the argument block would send it through scratch)
    float* const s0 = rot == 0 ? p.hist[2] : rot == 1 ? p.hist[0] : p.hist[1];
    float* const s1 = rot == 0 ? p.hist[1] : rot == 1 ? p.hist[2] : p.hist[0];
    float* const s2 = rot == 0 ? p.hist[0] : rot == 1 ? p.hist[1] : p.hist[2];
    const bool corrects = k_t != 0.f;
    // a zero coefficient leaves its buffer unread (dpm_kernel's rule for c_1); a null slot is never read either
    const bool rd_c = corrects && k[0] != 0.f && p.xc != nullptr;
    const bool c_0 = corrects && k[1] != 0.f && s0 != nullptr, c_1 = corrects && k[2] != 0.f && s1 != nullptr;
    const bool c_2 = corrects && k[3] != 0.f && s2 != nullptr;
    const bool q_1 = p_1 != 0.f && s0 != nullptr, q_2 = p_2 != 0.f && s1 != nullptr;
    // the next step's U-Net row, as dpm_kernel: the kernel never reads t_idx, so this one lane per sample races with nobody
    if (p.t_idx && blockIdx.x == 0 && threadIdx.x == 0) p.t_idx[b] = p.t_next[w.r];
    float* dst = dm3d_mode_dst(p.mode, p.out, p.x);
    float* xc_dst = dm3d_mode_dst(p.mode, p.xc_out, p.xc);
    float* x0_dst = dm3d_mode_dst(p.mode, p.x0_out, s2);
    const long base = (long)b * p.per4;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256) {
        const f32x4 x = load4(p.x, base + i);
        const f32x4 e = load4(p.eps, base + i);
        const f32x4 xc = rd_c ? load4(p.xc, base + i) : zero;
        const f32x4 h0 = (c_0 || q_1) ? load4(s0, base + i) : zero;
        const f32x4 h1 = (c_1 || q_2) ? load4(s1, base + i) : zero;
        const f32x4 h2 = c_2 ? load4(s2, base + i) : zero;
        f32x4 m, cn, o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            m[j] = dm3d_row_x0<false>(w, x[j], e[j]);
            float c = x[j];
            if (corrects) {
                c = rd_c ? __fmul_rn(k[0], xc[j]) : 0.f;
                c = c_0 ? __fadd_rn(c, __fmul_rn(k[1], h0[j])) : c;
                c = c_1 ? __fadd_rn(c, __fmul_rn(k[2], h1[j])) : c;
                c = c_2 ? __fadd_rn(c, __fmul_rn(k[3], h2[j])) : c;
                c = __fadd_rn(c, __fmul_rn(k_t, m[j]));
            }
            cn[j] = c;
            float r = __fadd_rn(__fmul_rn(p_x, c), __fmul_rn(p_0, m[j]));
            r = q_1 ? __fadd_rn(r, __fmul_rn(p_1, h0[j])) : r;
            r = q_2 ? __fadd_rn(r, __fmul_rn(p_2, h1[j])) : r;
            o[j] = r;
        }
        reinterpret_cast<f32x4*>(dst)[base + i] = o;
        if (xc_dst) reinterpret_cast<f32x4*>(xc_dst)[base + i] = cn;
        if (x0_dst) reinterpret_cast<f32x4*>(x0_dst)[base + i] = m;
    }
}

}  // namespace

extern "C" int dm3d_unipc_update(const dm3d_unipc_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "unipc: null descriptor");
    if (int rc = dm3d_update_rules("unipc", d, nullptr, d->corr != nullptr, "/corr",
                                   {d->corr, d->xc, d->hist[0], d->hist[1], d->hist[2], d->xc_out, d->x0_out})) return rc;
    DM3D_REQUIRE(d->mode == 0 || (d->xc && d->hist[0] && d->hist[1] && d->hist[2]), "unipc: mode 1 needs xc and all three hist slots");
    // every tensor is read and written lane by lane at one index, so two of them sharing a byte at all is a caller's mistake
    const void* bufs[] = {d->x, d->eps, d->xc, d->hist[0], d->hist[1], d->hist[2], d->out, d->xc_out, d->x0_out};
    const uint64_t bytes = (uint64_t)d->batch * (uint64_t)d->per_sample * sizeof(float);
    for (size_t i = 0; i < sizeof(bufs) / sizeof(bufs[0]); ++i)
        for (size_t j = i + 1; j < sizeof(bufs) / sizeof(bufs[0]); ++j)
            DM3D_REQUIRE(!dm3d_ranges_overlap(bufs[i], bytes, bufs[j], bytes), "unipc: tensors %d and %d (of x, eps, xc, hist[0..2], out, xc_out, "
                         "x0_out) overlap", (int)i, (int)j);
    unipc_args a{};
    a.x = d->x; a.eps = d->eps; a.xc = d->xc; a.out = d->out; a.xc_out = d->xc_out; a.x0_out = d->x0_out;
    for (int s = 0; s < 3; ++s) a.hist[s] = d->hist[s];
    a.per4 = d->per_sample / 4; a.coef = d->coef; a.corr = d->corr; a.t_next = d->t_next; a.rows = d->rows; a.pos = d->pos;
    a.t_idx = d->t_idx; a.mode = d->mode; a.x0_bound = d->x0_bound;
    hipLaunchKernelGGL(unipc_kernel, dm3d_stream_grid(a.per4, d->batch), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check("unipc_kernel");
}
