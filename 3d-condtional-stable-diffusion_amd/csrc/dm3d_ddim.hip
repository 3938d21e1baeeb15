// dm3d_ddim.hip — the DDIM update (Song et al., "Denoising Diffusion Implicit Models", eq. 12) over a schedule of timesteps:
// strided sampling (eta = 0 deterministic, eta > 0 stochastic, eta = 1 strided DDPM) and inversion share one kernel, because
// every per-step constant comes from a coefficient table the host writes once per chain (include/dm3d.h, dm3d_ddim_desc).
// A pure HBM stream like ddpm_kernel: 16 B per lane, read x and eps, write x (or out).
#include "dm3d_common.h"
#include "dm3d_philox.h"

namespace {

struct DdimArgs {
    float* x; const float* eps; const float* noise; float* out;
    long per4;                                     // float4 per sample
    const float* coef; const int* tau; const int* t_next; int rows;
    const int* pos; int* t_idx;
    uint64_t seed; const uint64_t* seed_dev; int mode;
    const float* x0_bound;
    const float* frame;
};

// One block's share of the update.  FRAME: `eps` holds the network's output in its own frame and row r of p.frame, (k0x, k0p, kex, kep),
// turns it into x0 and eps; cols 0 and 1 of coef are not used then.  Two kernels, chosen by the host, so that the eps kernel is the
// one it always was, registers included.
template <bool FRAME>
__device__ __forceinline__ void ddim_block(const DdimArgs& p) {
    const int b = blockIdx.y;
    const int r = min(max(p.pos[b], 0), p.rows - 1);
    const f32x4 c0 = reinterpret_cast<const f32x4*>(p.coef)[2 * r];          // sqrt(ab), sqrt(1-ab), a_x0, a_eps
    const f32x4 c1 = reinterpret_cast<const f32x4*>(p.coef)[2 * r + 1];      // sigma, clip, -, -
    const float sqab = c0[0], sq1ab = c0[1], a_x0 = c0[2], a_eps = c0[3], sigma = c1[0];
    f32x4 kf = {0.f, 0.f, 0.f, 0.f};
    if (FRAME) kf = reinterpret_cast<const f32x4*>(p.frame)[r];
    const bool clip = c1[1] != 0.f, draw = sigma != 0.f;
    const bool dyn = clip && p.x0_bound != nullptr;                          // the dynamic threshold's bound, read once per block
    const float s = dyn ? p.x0_bound[b] : 1.0f;
    const int tau = p.tau[r];
    const uint64_t seed = p.seed_dev ? *p.seed_dev : p.seed;
    // the next step's U-Net row; the kernel never reads t_idx, so this one lane per sample races with nobody
    if (p.t_idx && blockIdx.x == 0 && threadIdx.x == 0) p.t_idx[b] = p.t_next[r];
    float* dst = p.mode == 0 ? p.out : p.x;
    const long base = (long)b * p.per4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256) {
        const f32x4 x = reinterpret_cast<const f32x4*>(p.x)[base + i];
        const f32x4 e = reinterpret_cast<const f32x4*>(p.eps)[base + i];
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (draw) z = p.noise ? reinterpret_cast<const f32x4*>(p.noise)[base + i]
                              : philox_normal4((uint64_t)(base + i), (uint32_t)tau, 0xdd1au, seed);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float x0 = FRAME ? dm3d_frame_estimate(x[k], e[k], kf[0], kf[1])
                             : dm3d_x0_estimate(x[k], e[k], sqab, sq1ab);            // ddpm_kernel's order
            const float ek = FRAME ? dm3d_frame_estimate(x[k], e[k], kf[2], kf[3]) : e[k];       // the model's eps
            if (clip) x0 = dm3d_x0_bounded(x0, dyn, s);                              // a NaN passes, as in ddpm_kernel's clip
            o[k] = __fadd_rn(__fadd_rn(__fmul_rn(a_x0, x0), __fmul_rn(a_eps, ek)), __fmul_rn(sigma, z[k]));
        }
        reinterpret_cast<f32x4*>(dst)[base + i] = o;
    }
}

__global__ __launch_bounds__(256) void ddim_kernel(const DdimArgs p) { ddim_block<false>(p); }
__global__ __launch_bounds__(256) void ddim_frame_kernel(const DdimArgs p) { ddim_block<true>(p); }

}  // namespace

extern "C" int dm3d_ddim_update_frame(const dm3d_ddim_desc* d, const float* frame, void* stream) {
    DM3D_REQUIRE(d != nullptr, "ddim: null descriptor");
    DM3D_REQUIRE(d->x && d->eps && d->coef && d->tau && d->pos, "ddim: x/eps/coef/tau/pos must be non-null");
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0,
                 "ddim: batch=%d per_sample=%lld (must be a positive multiple of 4)", d->batch, (long long)d->per_sample);
    DM3D_REQUIRE(d->rows > 0, "ddim: rows=%d", d->rows);
    DM3D_REQUIRE(d->mode == 0 || d->mode == 1, "ddim: mode %d not in {0,1}", d->mode);
    DM3D_REQUIRE(d->mode == 1 || d->out, "ddim: mode 0 needs out");
    DM3D_REQUIRE(!d->t_idx || d->t_next, "ddim: t_idx needs t_next");
    DM3D_REQUIRE(dm3d_aligned16(d->x) && dm3d_aligned16(d->eps) && dm3d_aligned16(d->noise) && dm3d_aligned16(d->out) &&
                 dm3d_aligned16(d->coef) && dm3d_aligned16(frame), "ddim: pointers must be 16-byte aligned");
    DdimArgs a{};
    a.x = d->x; a.eps = d->eps; a.noise = d->noise; a.out = d->out; a.per4 = d->per_sample / 4;
    a.coef = d->coef; a.tau = d->tau; a.t_next = d->t_next; a.rows = d->rows; a.pos = d->pos; a.t_idx = d->t_idx;
    a.seed = d->seed; a.seed_dev = d->seed_dev; a.mode = d->mode; a.x0_bound = d->x0_bound; a.frame = frame;
    const long blocks = (a.per4 + 255) / 256;
    dim3 grid((unsigned)(blocks > 256 ? 256 : blocks), (unsigned)d->batch);                 // ddpm_kernel's grid
    hipLaunchKernelGGL(frame ? ddim_frame_kernel : ddim_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check(frame ? "ddim_frame_kernel" : "ddim_kernel");
}

extern "C" int dm3d_ddim_update(const dm3d_ddim_desc* d, void* stream) { return dm3d_ddim_update_frame(d, nullptr, stream); }
