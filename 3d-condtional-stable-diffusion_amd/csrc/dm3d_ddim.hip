// dm3d_ddim.hip — the DDIM update (Song et al., "Denoising Diffusion Implicit Models", eq. 12) over a schedule of timesteps:
// strided sampling (eta = 0 deterministic, eta > 0 stochastic, eta = 1 strided DDPM) and inversion share one kernel, because
// every per-step constant comes from a coefficient table the host writes once per chain (include/dm3d.h, dm3d_ddim_desc).
// A pure HBM stream like ddpm_kernel: 16 B per lane, read x and eps, write x (or out).
#include "dm3d_update.h"

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

// One block's share of the update: rows (sqrt(ab), sqrt(1-ab), a_x0, a_eps | sigma, clip, -, -).  FRAME: `eps` holds the network's
// output in its own frame and row r of p.frame, (k0x, k0p, kex, kep), turns it into x0 and eps.  Two kernels, chosen by the host, so
// that the eps kernel is the one it always was, registers included: for that the statements ahead of the loop keep their order and
// the model's eps is formed before the bounded x0 ("Shared code").
template <bool FRAME>
__device__ __forceinline__ void ddim_block(const DdimArgs& p) {
    const int b = blockIdx.y;
    const dm3d_row w = dm3d_row_decode<FRAME>(p.coef, p.frame, p.pos, p.rows, p.x0_bound, b);
    const float a_x0 = w.c0[2], a_eps = w.c0[3], sigma = w.c1[0];
    const bool draw = sigma != 0.f;
    const int tau = p.tau[w.r];
    const uint64_t seed = p.seed_dev ? *p.seed_dev : p.seed;
    // the next step's U-Net row; the kernel never reads t_idx, so this one lane per sample races with nobody
    if (p.t_idx && blockIdx.x == 0 && threadIdx.x == 0) p.t_idx[b] = p.t_next[w.r];
    float* dst = dm3d_mode_dst(p.mode, p.out, p.x);
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
            const float ek = FRAME ? dm3d_frame_estimate(x[k], e[k], w.kf[2], w.kf[3]) : e[k];   // the model's eps
            const float x0 = dm3d_row_x0<FRAME>(w, x[k], e[k]);
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
    if (int rc = dm3d_update_rules("ddim", d, frame, d->tau != nullptr, "/tau", {d->noise})) return rc;
    DdimArgs a{};
    a.x = d->x; a.eps = d->eps; a.noise = d->noise; a.out = d->out; a.per4 = d->per_sample / 4;
    a.coef = d->coef; a.tau = d->tau; a.t_next = d->t_next; a.rows = d->rows; a.pos = d->pos; a.t_idx = d->t_idx;
    a.seed = d->seed; a.seed_dev = d->seed_dev; a.mode = d->mode; a.x0_bound = d->x0_bound; a.frame = frame;
    hipLaunchKernelGGL(frame ? ddim_frame_kernel : ddim_kernel, dm3d_stream_grid(a.per4, d->batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check(frame ? "ddim_frame_kernel" : "ddim_kernel");
}

extern "C" int dm3d_ddim_update(const dm3d_ddim_desc* d, void* stream) { return dm3d_ddim_update_frame(d, nullptr, stream); }
