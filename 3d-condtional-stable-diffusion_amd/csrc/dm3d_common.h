// dm3d_common.h — shared host/device helpers for libdm3d_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdarg.h>
#include <atomic>
#include <initializer_list>
#include "dm3d.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- error plumbing (never throws across the ABI) ---------------------------------------------------------------
char* dm3d_err_buf();   // thread-local, 512 bytes
static inline int dm3d_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(dm3d_err_buf(), 512, fmt, ap);
    va_end(ap);
    return code;
}
#define DM3D_REQUIRE(cond, ...) do { if (!(cond)) return dm3d_fail(DM3D_EINVAL, __VA_ARGS__); } while (0)
#define DM3D_HIP(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) \
    return dm3d_fail(DM3D_EHIP, "%s failed: %s", #call, hipGetErrorString(e_)); } while (0)
static inline int dm3d_launch_check(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return dm3d_fail(DM3D_EHIP, "launch of %s failed: %s", what, hipGetErrorString(e));
    return DM3D_OK;
}
static inline bool dm3d_aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }   // bytes: a power of two
static inline bool dm3d_aligned16(const void* p) { return dm3d_aligned(p, 16); }
// Whether the byte ranges [p, p + p_bytes) and [q, q + q_bytes) share a byte (a null pointer is no range).
static inline bool dm3d_ranges_overlap(const void* p, uint64_t p_bytes, const void* q, uint64_t q_bytes) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return p && q && a < b + q_bytes && b < a + p_bytes;
}
static inline int64_t dm3d_round_up(int64_t v, int64_t m) { return (v + m - 1) / m * m; }
// The grid of a stream kernel over [batch][per4] float4 (ddpm_kernel's): at most 256 blocks of 256 lanes a sample, which stride over it.
static inline dim3 dm3d_stream_grid(long per4, int batch) {
    const long blocks = (per4 + 255) / 256;
    return dim3((unsigned)(blocks > 256 ? 256 : blocks), (unsigned)batch);
}

// Raises the dynamic-LDS limit of `kernels` to `lds` bytes on the device the launch goes to (the attribute belongs to the device), once per
// device: `set` is the caller's static array of 64 flags, one array per kernel instantiation (atomic: two host threads may meet in a first
// launch; the attribute call itself is idempotent).  Returns the device ordinal, or a negative DM3D_E* code; `who` names the caller in the text.
template <class... K>
static inline int dm3d_dyn_lds(size_t lds, std::atomic<bool>* set, const char* who, K*... kernels) {
    int dev = 0;
    DM3D_HIP(hipGetDevice(&dev));
    DM3D_REQUIRE(dev >= 0 && dev < 64, "%s: device ordinal %d", who, dev);
    if (!set[dev]) {
        for (const void* f : {reinterpret_cast<const void*>(kernels)...})
            DM3D_HIP(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        set[dev] = true;
    }
    return dev;
}

// H3 range guard (include/dm3d.h, range_flag): running max |value| of what an epilogue stores.  -DDM3D_NO_RANGE_GUARD builds the
// A/B variant without it (tools/mk_variant.sh).
#ifdef DM3D_NO_RANGE_GUARD
#define DM3D_AMAX(a, v) ((void)(v))
#else
#define DM3D_AMAX(a, v) ((a) = fmaxf((a), fabsf(v)))
#endif

// ---- device helpers -----------------------------------------------------------------------------------------------
__device__ __forceinline__ float dm3d_silu(float y) {
    // y * sigmoid(y) as mul, v_exp_f32, add, v_rcp_f32, mul (both ~1 ulp, far inside the 1e-3 parity budget).
    // __frcp_rn / 1.0f/x would expand to the ~10-instruction correctly-rounded division sequence.
    return y * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(y * -1.4426950408889634f));
}
__device__ __forceinline__ float dm3d_act(float v, int act) {
    if (act == DM3D_ACT_RELU) return fmaxf(v, 0.0f);
    if (act == DM3D_ACT_SILU) return dm3d_silu(v);
    return v;
}

// The fixed-order float64 sum of v[0..K-1] over a block of 256 lanes, the one tree behind every "runs repeat bitwise" of include/dm3d.h:
// a wave adds lane l and lane l ^ off for off = 32, 16, .. 1, lane 0 of each wave leaves its K totals in red[wave], and after the one
// barrier every lane returns ((red[0] + red[1]) + red[2]) + red[3].  Only lane 0's wave total is ever stored, and at every step lane 0
// and the lanes it will still read (l < off) add their own value and that of lane l + off = l ^ off, in that order: the pairs and their
// order are those of a __shfl_down tree, so which of the two shuffles is written here moves no bit.  Every lane of the block must
// arrive; one call per kernel (red is not reused); red takes 8 K bytes of LDS per wave, 32 K per block.
template <int K>
__device__ __forceinline__ void dm3d_block_sum_f64(double (&v)[K], double (*red)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[threadIdx.x >> 6][k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((red[0][k] + red[1][k]) + red[2][k]) + red[3][k];
}

// One (tap, Cin-chunk) step of the implicit GEMM for a wave owning MR x NR tiles of 32x32 outputs.
// v_mfma_f32_32x32x2_f32: lane l supplies A[i = l&31][k = l>>5] and B[k = l>>5][j = l&31]; the two lane halves carry
// two different k, so with CK channels per chunk half h takes channels [h*CK/2, (h+1)*CK/2) as CK/8 float4 reads and
// MFMA (q, j) contracts channels {q*4+j, CK/2+q*4+j}.  A and B use the same assignment, so the order is irrelevant.
//   a_lds[mr]: this lane's voxel row (channel 0 of the chunk) for row-tile mr, already offset by the tap
//   b_lds[nr]: this lane's output-channel row of the weight slice for col-tile nr
template <int MR, int NR, int CK>
__device__ __forceinline__ void dm3d_mma_step(f32x16 (&acc)[MR][NR], const float* (&a_lds)[MR],
                                              const float* (&b_lds)[NR], int half) {
    constexpr int KQ = CK / 8;
    f32x4 a[MR][KQ], b[NR][KQ];
#pragma unroll
    for (int mr = 0; mr < MR; ++mr)
#pragma unroll
        for (int q = 0; q < KQ; ++q) a[mr][q] = *reinterpret_cast<const f32x4*>(a_lds[mr] + half * (CK / 2) + q * 4);
#pragma unroll
    for (int nr = 0; nr < NR; ++nr)
#pragma unroll
        for (int q = 0; q < KQ; ++q) b[nr][q] = *reinterpret_cast<const f32x4*>(b_lds[nr] + half * (CK / 2) + q * 4);
#pragma unroll
    for (int q = 0; q < KQ; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mr = 0; mr < MR; ++mr)
#pragma unroll
                for (int nr = 0; nr < NR; ++nr)
                    acc[mr][nr] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[mr][q][j], b[nr][q][j], acc[mr][nr], 0, 0, 0);
}

// C/D layout of the 32x32 MFMA: register r of lane l holds row (r&3) + 8*(r>>2) + 4*(l>>5), column l&31.
__device__ __forceinline__ int dm3d_acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }
