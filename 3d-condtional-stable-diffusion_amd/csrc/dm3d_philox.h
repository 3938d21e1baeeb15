// dm3d_philox.h — the counter-based N(0,1) generator of the sampling kernels (dm3d_elem.hip: randn, ddpm_update;
// dm3d_ddim.hip: ddim_update; dm3d_edit.hip: edit_update).  Each caller keys its draws with a stream constant of its own in the counter.
#pragma once
#include "dm3d_common.h"

// ---- Philox4x32-10 + Box-Muller ---------------------------------------------------------------------------------------
static __device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}
// four N(0,1) draws for 128-bit counter (i_lo, i_hi, s0, s1) under key seed
static __device__ __forceinline__ f32x4 philox_normal4(uint64_t idx, uint32_t s0, uint32_t s1, uint64_t seed) {
    uint32_t c[4] = {(uint32_t)idx, (uint32_t)(idx >> 32), s0, s1};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u0 = ((float)c[0] + 0.5f) * 2.3283064365386963e-10f;   // (0,1]: float rounding can reach 1, log(1)=0 is fine
    const float u1 = (float)c[1] * 2.3283064365386963e-10f;
    const float u2 = ((float)c[2] + 0.5f) * 2.3283064365386963e-10f;
    const float u3 = (float)c[3] * 2.3283064365386963e-10f;
    const float r0 = sqrtf(-2.0f * logf(u0)), r1 = sqrtf(-2.0f * logf(u2));
    float s_0, c_0, s_1, c_1;
    sincosf(6.283185307179586f * u1, &s_0, &c_0);
    sincosf(6.283185307179586f * u3, &s_1, &c_1);
    return f32x4{r0 * c_0, r0 * s_0, r1 * c_1, r1 * s_1};
}
