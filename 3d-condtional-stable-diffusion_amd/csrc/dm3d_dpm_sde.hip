// dm3d_dpm_sde.hip — the stochastic DPM-Solver++(2M) update (Lu et al. 2022, "DPM-Solver++", the SDE form of the appendix; k-diffusion's
// dpmpp_2m_sde): dpm_kernel's multistep update of the data-prediction form plus one noise term per step.  Every per-step constant comes
// from a coefficient table the host writes once per chain (include/dm3d.h, dm3d_dpm_sde_desc), so first-order rows, second-order rows,
// the step to the clean sample and rows without noise (eta = 0: dpm_kernel's result bitwise) share one kernel.  A pure HBM stream like
// dpm_kernel: 16 B per lane, read x, eps and (second-order rows only) the previous x0 estimate, write x and this step's x0 estimate;
// z is an injected tensor or ddim_kernel's in-kernel Philox draw under a stream constant of this kernel's own.
#include "dm3d_common.h"
#include "dm3d_philox.h"

namespace {

struct DpmSdeArgs {
    float* x; const float* eps; float* hist; float* out; float* x0_out; const float* noise;
    long per4;                                     // float4 per sample
    const float* coef; const int* tau; const int* t_next; int rows;
    const int* pos; int* t_idx;
    uint64_t seed; const uint64_t* seed_dev; int mode;
    const float* x0_bound;
    const float* frame;
};

// One block's share of the update.  FRAME: `eps` holds the network's output in its own frame and (k0x, k0p) of row r of p.frame turn
// it into x0; cols 0 and 1 of coef are not used then.  Two kernels, chosen by the host, as dpm_kernel / dpm_frame_kernel.
template <bool FRAME>
__device__ __forceinline__ void dpm_sde_block(const DpmSdeArgs& p) {
    const int b = blockIdx.y;
    const int r = min(max(p.pos[b], 0), p.rows - 1);
    const f32x4 c0 = reinterpret_cast<const f32x4*>(p.coef)[2 * r];          // sqrt(ab), sqrt(1-ab), c_x, c_0
    const f32x4 c1 = reinterpret_cast<const f32x4*>(p.coef)[2 * r + 1];      // c_1, clip, c_z, -
    float ka = c0[0], kb = c0[1];
    if (FRAME) {
        const f32x4 kf = reinterpret_cast<const f32x4*>(p.frame)[r];         // k0x, k0p, kex, kep
        ka = kf[0], kb = kf[1];
    }
    const float c_x = c0[2], c_0 = c0[3], c_1 = c1[0], c_z = c1[2];
    const bool clip = c1[1] != 0.f, draw = c_z != 0.f;
    const bool dyn = clip && p.x0_bound != nullptr;                          // the dynamic threshold's bound, read once per block
    const float s = dyn ? p.x0_bound[b] : 1.0f;
    const bool second = c_1 != 0.f && p.hist != nullptr;                     // a first-order row never reads the history
    const int tau = p.tau[r];
    const uint64_t seed = p.seed_dev ? *p.seed_dev : p.seed;
    // the next step's U-Net row; the kernel never reads t_idx, so this one lane per sample races with nobody
    if (p.t_idx && blockIdx.x == 0 && threadIdx.x == 0) p.t_idx[b] = p.t_next[r];
    float* dst = p.mode == 0 ? p.out : p.x;
    float* x0_dst = p.mode == 0 ? p.x0_out : p.hist;
    const long base = (long)b * p.per4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256) {
        const f32x4 x = reinterpret_cast<const f32x4*>(p.x)[base + i];
        const f32x4 e = reinterpret_cast<const f32x4*>(p.eps)[base + i];
        f32x4 h = {0.f, 0.f, 0.f, 0.f}, z = {0.f, 0.f, 0.f, 0.f};
        if (second) h = reinterpret_cast<const f32x4*>(p.hist)[base + i];
        if (draw) z = p.noise ? reinterpret_cast<const f32x4*>(p.noise)[base + i]
                              : philox_normal4((uint64_t)(base + i), (uint32_t)tau, 0x5de2u, seed);
        f32x4 o, x0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float v = FRAME ? dm3d_frame_estimate(x[k], e[k], ka, kb)
                            : dm3d_x0_estimate(x[k], e[k], ka, kb);                  // dpm_kernel's order
            if (clip) v = dm3d_x0_bounded(v, dyn, s);                                // a NaN passes, as in dpm_kernel's clip
            x0[k] = v;
            const float first = __fadd_rn(__fmul_rn(c_x, x[k]), __fmul_rn(c_0, v));
            const float ode = second ? __fadd_rn(first, __fmul_rn(c_1, h[k])) : first;
            o[k] = draw ? __fadd_rn(ode, __fmul_rn(c_z, z[k])) : ode;                // c_z == 0: dpm_kernel's result bitwise
        }
        reinterpret_cast<f32x4*>(dst)[base + i] = o;
        if (x0_dst) reinterpret_cast<f32x4*>(x0_dst)[base + i] = x0;
    }
}

__global__ __launch_bounds__(256) void dpm_sde_kernel(const DpmSdeArgs p) { dpm_sde_block<false>(p); }
__global__ __launch_bounds__(256) void dpm_sde_frame_kernel(const DpmSdeArgs p) { dpm_sde_block<true>(p); }

}  // namespace

extern "C" int dm3d_dpm_sde_update_frame(const dm3d_dpm_sde_desc* d, const float* frame, void* stream) {
    DM3D_REQUIRE(d != nullptr, "dpm_sde: null descriptor");
    DM3D_REQUIRE(d->x && d->eps && d->coef && d->pos && d->tau, "dpm_sde: x/eps/coef/pos/tau must be non-null");
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0,
                 "dpm_sde: batch=%d per_sample=%lld (must be a positive multiple of 4)", d->batch, (long long)d->per_sample);
    DM3D_REQUIRE(d->rows > 0, "dpm_sde: rows=%d", d->rows);
    DM3D_REQUIRE(d->mode == 0 || d->mode == 1, "dpm_sde: mode %d not in {0,1}", d->mode);
    DM3D_REQUIRE(d->mode == 1 || d->out, "dpm_sde: mode 0 needs out");
    DM3D_REQUIRE(d->mode == 0 || d->hist, "dpm_sde: mode 1 needs hist");
    DM3D_REQUIRE(!d->t_idx || d->t_next, "dpm_sde: t_idx needs t_next");
    DM3D_REQUIRE(dm3d_aligned16(d->x) && dm3d_aligned16(d->eps) && dm3d_aligned16(d->hist) && dm3d_aligned16(d->out) &&
                 dm3d_aligned16(d->x0_out) && dm3d_aligned16(d->coef) && dm3d_aligned16(d->noise) && dm3d_aligned16(frame),
                 "dpm_sde: pointers must be 16-byte aligned");
    DpmSdeArgs a{};
    a.x = d->x; a.eps = d->eps; a.hist = d->hist; a.out = d->out; a.x0_out = d->x0_out; a.noise = d->noise; a.per4 = d->per_sample / 4;
    a.coef = d->coef; a.tau = d->tau; a.t_next = d->t_next; a.rows = d->rows; a.pos = d->pos; a.t_idx = d->t_idx;
    a.seed = d->seed; a.seed_dev = d->seed_dev; a.mode = d->mode; a.x0_bound = d->x0_bound; a.frame = frame;
    const long blocks = (a.per4 + 255) / 256;
    dim3 grid((unsigned)(blocks > 256 ? 256 : blocks), (unsigned)d->batch);                 // dpm_kernel's grid
    hipLaunchKernelGGL(frame ? dpm_sde_frame_kernel : dpm_sde_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check(frame ? "dpm_sde_frame_kernel" : "dpm_sde_kernel");
}

extern "C" int dm3d_dpm_sde_update(const dm3d_dpm_sde_desc* d, void* stream) { return dm3d_dpm_sde_update_frame(d, nullptr, stream); }
