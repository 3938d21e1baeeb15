// dm3d_guide.hip — classifier-free guidance between the U-Net and the update of a guided chain (include/dm3d.h, dm3d_guide_desc):
// the combine eps_neg + w (eps_pos - eps_neg) with per-sample w, the guidance rescale of Lin et al. 2023 (section 3.4) from per-sample
// standard deviations, and the mirror that hands the updated first half of a 2B plan to its second half.  Three pure HBM streams
// like ddim_kernel, 16 B per lane.  The standard deviations come from float64 sums (a float32 product is exact in float64, so a
// volume with |mean| >> std keeps its variance), reduced in a fixed order: the block by dm3d_block_sum_f64, blocks through a partials
// buffer in block order by a second launch (no atomics, no grid-wide barrier).
#include "dm3d_common.h"

namespace {

constexpr int PARTS = DM3D_GUIDE_PARTIAL_BLOCKS;

struct GuideArgs {
    const float* eps_pos; const float* eps_neg; float* out;
    long per4;                                     // float4 per sample
    const float* scale; const float* rescale; double* partials;
    float* x; int* t_idx; int batch;
};

__global__ __launch_bounds__(256) void guide_combine_kernel(const GuideArgs p) {
    __shared__ double red[4][4];
    const int b = blockIdx.y;
    const float w = p.scale[b];
    const bool stats = p.partials != nullptr && p.rescale != nullptr && p.rescale[b] != 0.f;
    const bool pos_only = w == 1.f, neg_only = w == 0.f;
    const bool store = !(pos_only && p.out == p.eps_pos);
    if (!store && !stats) return;                                            // in place at w = 1: the row is eps_out already
    const long base = (long)b * p.per4;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};                                    // sum eps_pos, sum eps_pos^2, sum eps_g, sum eps_g^2
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256) {
        f32x4 ep = {0.f, 0.f, 0.f, 0.f}, en = ep, g;
        if (!neg_only || stats) ep = reinterpret_cast<const f32x4*>(p.eps_pos)[base + i];
        if (!pos_only) en = reinterpret_cast<const f32x4*>(p.eps_neg)[base + i];
        if (pos_only) g = ep;
        else if (neg_only) g = en;
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k) g[k] = __fadd_rn(en[k], __fmul_rn(w, __fsub_rn(ep[k], en[k])));
        }
        if (store) reinterpret_cast<f32x4*>(p.out)[base + i] = g;
        if (stats) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double a = (double)ep[k], c = (double)g[k];
                acc[0] += a; acc[1] += a * a; acc[2] += c; acc[3] += c * c;
            }
        }
    }
    if (!stats) return;                                                      // uniform over the block
    dm3d_block_sum_f64(acc, red);
    if (threadIdx.x == 0) {
        double* dst = p.partials + ((long)b * PARTS + blockIdx.x) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) dst[k] = acc[k];
    }
}

__global__ __launch_bounds__(256) void guide_rescale_kernel(const GuideArgs p) {
    __shared__ double red[4][4];
    __shared__ float f_sh;
    const int b = blockIdx.y;
    const float phi = p.rescale[b];
    if (phi == 0.f) return;
    // every block of the row reduces the row's partials itself, in the same order: they all arrive at the same f
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if (threadIdx.x < gridDim.x) {                                           // gridDim.x <= PARTS = 256: combine's grid
        const double* src = p.partials + ((long)b * PARTS + threadIdx.x) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = src[k];
    }
    dm3d_block_sum_f64(v, red);
    if (threadIdx.x == 0) {
        const double n = (double)(p.per4 * 4);
        const double mp = v[0] / n, mg = v[2] / n;
        double var_p = v[1] / n - mp * mp, var_g = v[3] / n - mg * mg;       // population variances
        var_p = var_p < 0.0 ? 0.0 : var_p;                                   // (a NaN passes both)
        var_g = var_g < 0.0 ? 0.0 : var_g;
        f_sh = var_g == 0.0 ? 1.0f : (float)((double)phi * sqrt(var_p / var_g) + (1.0 - (double)phi));
    }
    __syncthreads();
    const float f = f_sh;
    const long base = (long)b * p.per4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256) {
        f32x4 o = reinterpret_cast<const f32x4*>(p.out)[base + i];
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = __fmul_rn(f, o[k]);
        reinterpret_cast<f32x4*>(p.out)[base + i] = o;
    }
}

__global__ __launch_bounds__(256) void guide_mirror_kernel(const GuideArgs p) {
    const int b = blockIdx.y;
    if (p.t_idx && blockIdx.x == 0 && threadIdx.x == 0) p.t_idx[p.batch + b] = p.t_idx[b];
    const long src = (long)b * p.per4, dst = (long)(p.batch + b) * p.per4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256)
        reinterpret_cast<f32x4*>(p.x)[dst + i] = reinterpret_cast<const f32x4*>(p.x)[src + i];
}

}  // namespace

extern "C" int dm3d_guide_update(const dm3d_guide_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "guide: null descriptor");
    DM3D_REQUIRE(d->mode >= 0 && d->mode <= 2, "guide: mode %d not in {0,1,2}", d->mode);
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0,
                 "guide: batch=%d per_sample=%lld (batch in [1, 65535], per_sample a positive multiple of 4)", d->batch,
                 (long long)d->per_sample);
    if (d->mode == 0) {
        DM3D_REQUIRE(d->eps_pos && d->eps_neg && d->out && d->scale, "guide: mode 0: eps_pos/eps_neg/out/scale must be non-null");
        DM3D_REQUIRE((const float*)d->out != d->eps_neg, "guide: out may alias eps_pos only, never eps_neg");
        DM3D_REQUIRE(!d->partials || d->rescale, "guide: partials without rescale");
    } else if (d->mode == 1) {
        DM3D_REQUIRE(d->out && d->rescale && d->partials, "guide: mode 1: out/rescale/partials must be non-null");
    } else {
        DM3D_REQUIRE(d->x, "guide: mode 2: x must be non-null");
        DM3D_REQUIRE(d->batch <= 32767, "guide: mode 2: batch=%d (the plan holds 2*batch <= 65534 rows)", d->batch);
    }
    DM3D_REQUIRE(dm3d_aligned16(d->eps_pos) && dm3d_aligned16(d->eps_neg) && dm3d_aligned16(d->out) && dm3d_aligned16(d->partials) &&
                 dm3d_aligned16(d->x), "guide: pointers must be 16-byte aligned");
    GuideArgs a{};
    a.eps_pos = d->eps_pos; a.eps_neg = d->eps_neg; a.out = d->out; a.per4 = d->per_sample / 4;
    a.scale = d->scale; a.rescale = d->rescale; a.partials = d->partials; a.x = d->x; a.t_idx = d->t_idx; a.batch = d->batch;
    const long blocks = (a.per4 + 255) / 256;
    dim3 grid((unsigned)(blocks > PARTS ? PARTS : blocks), (unsigned)d->batch);             // ddpm_kernel's grid; at most PARTS partials a row
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->mode == 0) {
        hipLaunchKernelGGL(guide_combine_kernel, grid, dim3(256), 0, st, a);
        return dm3d_launch_check("guide_combine_kernel");
    }
    if (d->mode == 1) {
        hipLaunchKernelGGL(guide_rescale_kernel, grid, dim3(256), 0, st, a);
        return dm3d_launch_check("guide_rescale_kernel");
    }
    hipLaunchKernelGGL(guide_mirror_kernel, grid, dim3(256), 0, st, a);
    return dm3d_launch_check("guide_mirror_kernel");
}
