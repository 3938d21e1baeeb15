// dm3d_update.h — what the solver update kernels (dm3d_ddim.hip, dm3d_dpm.hip, dm3d_dpm_sde.hip) and the first pass of the dynamic
// threshold (dm3d_thresh.hip) share: the decode of a sample's table row, the x0 estimate and its bound, the one body of the two
// DPM-Solver++(2M) updates, and the descriptor rules of the three entry points.  A change to the clamp, to the estimate or to the
// row layout is made here, once, and reaches every kernel that has to agree on it bitwise.
#pragma once
#include "dm3d_common.h"
#include "dm3d_philox.h"

// ---- the x0 estimate ------------------------------------------------------------------------------------------------
// (x - sqrt(1-a)*eps) / sqrt(a) as mul, sub, div, each rounded (ddpm_kernel's order).  One function for the update kernels and the
// dynamic threshold's selection: the magnitudes ranked are bitwise the values clamped.
__device__ __forceinline__ float dm3d_x0_estimate(float x, float eps, float sqab, float sq1ab) {
    return __fdiv_rn(__fsub_rn(x, __fmul_rn(sq1ab, eps)), sqab);
}
// The same estimate, and ddim_kernel's eps, from the network's output p in its own frame (include/dm3d.h, dm3d_ddim_update_frame): one row
// (k0x, k0p, kex, kep) of the host's frame table gives x0 = k0x*x + k0p*p and eps = kex*x + kep*p, each as mul, mul, add, each rounded.
// No division: a v-model's row is (a, -s, s, a), finite where sqrt(alpha_bar) is 0 (the zero-terminal-SNR schedule's last timestep).
__device__ __forceinline__ float dm3d_frame_estimate(float x, float p, float kx, float kp) {
    return __fadd_rn(__fmul_rn(kx, x), __fmul_rn(kp, p));
}
// The bounded estimate: clamp(x0, -1, 1), or with a dynamic bound s (include/dm3d.h, dm3d_thresh_desc) clamp(x0, -s, s) / s.  A NaN
// passes; `dyn` is uniform over the block, so the static path is the one instruction pair it always was.
__device__ __forceinline__ float dm3d_x0_bounded(float x0, bool dyn, float s) {
    if (x0 != x0) return x0;
    if (dyn) return __fdiv_rn(fminf(fmaxf(x0, -s), s), s);
    return fminf(fmaxf(x0, -1.0f), 1.0f);
}

// ---- a sample's row ---------------------------------------------------------------------------------------------------
// What a block reads of row r = clamp(pos[b]) before its loop; uniform over the block.
struct dm3d_row {
    int r;
    f32x4 c0, c1;                                  // the row of coef: cols 0-3 and 4-7 (col 5: clip; the others are the solver's own)
    f32x4 kf;                                      // FRAME: the row of frame, (k0x, k0p, kex, kep); else zeros
    float ka, kb;                                  // the estimate's pair: (k0x, k0p) or cols 0 and 1 of coef, (sqrt(ab), sqrt(1-ab))
    bool clip, dyn;                                // the estimate is bounded; there is a dynamic bound (it counts only where clip)
    float s;                                       // that bound, read once per block (1 where the row has none)
};

// FRAME: `eps` holds the network's output in its own frame; cols 0 and 1 of coef are not used then.  x0_bound may be null.
template <bool FRAME>
__device__ __forceinline__ dm3d_row dm3d_row_decode(const float* coef, const float* frame, const int* pos, int rows,
                                                    const float* x0_bound, int b) {
    dm3d_row w;
    w.r = min(max(pos[b], 0), rows - 1);
    w.c0 = reinterpret_cast<const f32x4*>(coef)[2 * w.r];
    w.c1 = reinterpret_cast<const f32x4*>(coef)[2 * w.r + 1];
    w.kf = f32x4{0.f, 0.f, 0.f, 0.f};
    if (FRAME) w.kf = reinterpret_cast<const f32x4*>(frame)[w.r];
    w.ka = FRAME ? w.kf[0] : w.c0[0];
    w.kb = FRAME ? w.kf[1] : w.c0[1];
    w.clip = w.c1[1] != 0.f;
    w.dyn = x0_bound != nullptr;
    w.s = w.clip && w.dyn ? x0_bound[b] : 1.0f;
    return w;
}

// The x0 estimate of one element as the threshold ranks it, and as the updates use it: bounded where the row clips (a NaN passes).
template <bool FRAME>
__device__ __forceinline__ float dm3d_row_estimate(const dm3d_row& w, float x, float e) {
    return FRAME ? dm3d_frame_estimate(x, e, w.ka, w.kb) : dm3d_x0_estimate(x, e, w.ka, w.kb);
}
template <bool FRAME>
__device__ __forceinline__ float dm3d_row_x0(const dm3d_row& w, float x, float e) {
    const float v = dm3d_row_estimate<FRAME>(w, x, e);
    return w.clip ? dm3d_x0_bounded(v, w.dyn, w.s) : v;
}

// Where a mode-0 call (a new tensor) and a mode-1 call (the chain's own buffer) write.
__device__ __forceinline__ float* dm3d_mode_dst(int mode, float* fresh, float* own) { return mode == 0 ? fresh : own; }

// ---- the DPM-Solver++(2M) update, ODE and SDE form --------------------------------------------------------------------
struct dm3d_dpm_args {
    float* x; const float* eps; float* hist; float* out; float* x0_out;
    long per4;                                     // float4 per sample
    const float* coef; const int* t_next; int rows;
    const int* pos; int* t_idx;
    int mode;
    const float* x0_bound;
    const float* frame;
};
// The SDE kernels' arguments: the ODE kernels' and the draw's.  Two structs, so that the ODE kernels keep their 112 bytes of arguments:
// with these four members in their struct too, dpm_kernel (the same instructions) measured 1.0-1.6 % slower per launch.
struct dm3d_dpm_sde_args : dm3d_dpm_args {
    const float* noise; const int* tau; uint64_t seed; const uint64_t* seed_dev;
};
template <bool SDE> struct dm3d_dpm_args_for { typedef dm3d_dpm_args type; };
template <> struct dm3d_dpm_args_for<true> { typedef dm3d_dpm_sde_args type; };

// One block's share of the update: rows (sqrt(ab), sqrt(1-ab), c_x, c_0 | c_1, clip, c_z, -).  SDE: the row's c_z z is added, z an
// injected tensor or ddim_kernel's Philox draw under this solver's own stream constant; a row with c_z == 0 gives the ODE kernel's
// result bitwise.  The ODE kernels (SDE false) read neither col 6 nor noise, tau or the seed.  The statements ahead of the loop keep
// the order the two earlier bodies had: the compiler's registers depend on it ("Shared code").
template <bool FRAME, bool SDE>
__device__ __forceinline__ void dm3d_dpm_block(const typename dm3d_dpm_args_for<SDE>::type& p) {
    const int b = blockIdx.y;
    const dm3d_row w = dm3d_row_decode<FRAME>(p.coef, p.frame, p.pos, p.rows, p.x0_bound, b);
    const float c_x = w.c0[2], c_0 = w.c0[3], c_1 = w.c1[0], c_z = SDE ? w.c1[2] : 0.f;
    const bool second = c_1 != 0.f && p.hist != nullptr;                     // a first-order row never reads the history
    const bool draw = c_z != 0.f;
    int tau = 0;
    uint64_t seed = 0;
    if constexpr (SDE) {
        tau = p.tau[w.r];
        seed = p.seed_dev ? *p.seed_dev : p.seed;
    }
    // the next step's U-Net row (as in ddim_block: a helper of its own reorders the prologue's scalar code); the kernel never reads
    // t_idx, so this one lane per sample races with nobody
    if (p.t_idx && blockIdx.x == 0 && threadIdx.x == 0) p.t_idx[b] = p.t_next[w.r];
    float* dst = dm3d_mode_dst(p.mode, p.out, p.x);
    float* x0_dst = dm3d_mode_dst(p.mode, p.x0_out, p.hist);
    const long base = (long)b * p.per4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256) {
        const f32x4 x = reinterpret_cast<const f32x4*>(p.x)[base + i];
        const f32x4 e = reinterpret_cast<const f32x4*>(p.eps)[base + i];
        f32x4 h = {0.f, 0.f, 0.f, 0.f}, z = {0.f, 0.f, 0.f, 0.f};
        if (second) h = reinterpret_cast<const f32x4*>(p.hist)[base + i];
        if constexpr (SDE)
            if (draw) z = p.noise ? reinterpret_cast<const f32x4*>(p.noise)[base + i]
                                  : philox_normal4((uint64_t)(base + i), (uint32_t)tau, 0x5de2u, seed);
        f32x4 o, x0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            x0[k] = dm3d_row_x0<FRAME>(w, x[k], e[k]);
            const float first = __fadd_rn(__fmul_rn(c_x, x[k]), __fmul_rn(c_0, x0[k]));
            o[k] = second ? __fadd_rn(first, __fmul_rn(c_1, h[k])) : first;
            if constexpr (SDE) o[k] = draw ? __fadd_rn(o[k], __fmul_rn(c_z, z[k])) : o[k];
        }
        reinterpret_cast<f32x4*>(dst)[base + i] = o;
        if (x0_dst) reinterpret_cast<f32x4*>(x0_dst)[base + i] = x0;
    }
}

// ---- host side ----------------------------------------------------------------------------------------------------
// The rules the three update descriptors share (their common members carry one name), before any device call; `d` is not null and
// `who` prefixes the messages.  `own`: the entry's further required pointers are all there, `own_names` names them in the message;
// `vec`: its further pointers the kernel reads 16 bytes at a time (null is aligned).
template <class Desc>
static inline int dm3d_update_rules(const char* who, const Desc* d, const float* frame, bool own, const char* own_names,
                                    std::initializer_list<const void*> vec) {
    DM3D_REQUIRE(d->x && d->eps && d->coef && d->pos && own, "%s: x/eps/coef/pos%s must be non-null", who, own_names);
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0,
                 "%s: batch=%d per_sample=%lld (must be a positive multiple of 4)", who, d->batch, (long long)d->per_sample);
    DM3D_REQUIRE(d->rows > 0, "%s: rows=%d", who, d->rows);
    DM3D_REQUIRE(d->mode == 0 || d->mode == 1, "%s: mode %d not in {0,1}", who, d->mode);
    DM3D_REQUIRE(d->mode == 1 || d->out, "%s: mode 0 needs out", who);
    DM3D_REQUIRE(!d->t_idx || d->t_next, "%s: t_idx needs t_next", who);
    bool aligned = dm3d_aligned16(d->x) && dm3d_aligned16(d->eps) && dm3d_aligned16(d->out) && dm3d_aligned16(d->coef) && dm3d_aligned16(frame);
    for (const void* q : vec) aligned = aligned && dm3d_aligned16(q);
    DM3D_REQUIRE(aligned, "%s: pointers must be 16-byte aligned", who);
    return DM3D_OK;
}

// The descriptor of either DPM entry as kernel arguments (the SDE members are the caller's), after its rules.
template <class Desc>
static inline int dm3d_dpm_args_of(const char* who, const Desc* d, const float* frame, bool own, const char* own_names,
                                   const void* noise, dm3d_dpm_args& a) {
    if (int rc = dm3d_update_rules(who, d, frame, own, own_names, {d->hist, d->x0_out, noise})) return rc;
    DM3D_REQUIRE(d->mode == 0 || d->hist, "%s: mode 1 needs hist", who);
    a.x = d->x; a.eps = d->eps; a.hist = d->hist; a.out = d->out; a.x0_out = d->x0_out; a.per4 = d->per_sample / 4;
    a.coef = d->coef; a.t_next = d->t_next; a.rows = d->rows; a.pos = d->pos; a.t_idx = d->t_idx; a.mode = d->mode;
    a.x0_bound = d->x0_bound; a.frame = frame;
    return DM3D_OK;
}
