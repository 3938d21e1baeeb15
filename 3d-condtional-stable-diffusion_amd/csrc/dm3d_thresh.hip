// dm3d_thresh.hip — dynamic thresholding of the x0 estimate (Saharia et al. 2022, "Imagen", section 2.3) for the DDIM and DPM-Solver++
// chains: the per-volume bound s = clamp(quantile_p(|x0|), 1, smax) the update kernels then clamp and divide by (include/dm3d.h,
// dm3d_thresh_desc).  The quantile is exact: the two order statistics v_i, v_{i+1} it interpolates come from an MSB-first radix
// select over the 31 magnitude bits of |x0| (non-negative floats order as their bit patterns; a NaN's pattern is above +inf's, so it
// sorts last), in three counting passes of 12, 10 and 9 bits that carry both ranks.
//   pass 1   reads x and eps, computes x0 with the update kernels' own device function, stashes the magnitudes and counts the top
//            12 bits (exponent and 4 mantissa bits: about 16 bins an octave, so no bin of a smooth volume holds more than a few
//            percent of it);
//   pass 2/3 read the stash, find from the histogram before them the bin each rank fell into (every block scans it itself, in the
//            same order: they all arrive at the same bin) and count the next digit of the elements under that prefix; while both
//            ranks share a prefix they share a histogram;
//   final    one block a volume finds the last digit of both ranks and writes bound[b].
// Counts are integers: a block counts in LDS, then adds its non-empty bins to the volume's histogram with global atomics, whose sum
// does not depend on the order of arrival.  In LDS a wave aggregates one digit group, the first valid lane's: those lanes add their
// count once, every other valid lane adds 1 on its own.  That removes the worst case (a volume of one repeated value: one add a wave,
// not 64 serialised ones) and leaves a wave of g distinct digits with g adds, of which those that share a digit serialise: at most
// 32-fold (two values, half the lanes each), a few-fold on a smooth volume ("Counting" and the measurement paragraph).  Nothing else is shared between blocks, so runs repeat bitwise.  The
// histograms are cleared by a kernel of their own at the head of every launch (a kernel node like the others, so a captured step
// stays one chain of kernels); no host read anywhere: graph-capturable.
#include "dm3d_update.h"

namespace {

constexpr int BITS1 = 12, BITS2 = 10, BITS3 = 9;                       // 31 magnitude bits, most significant first
constexpr int BINS1 = 1 << BITS1, BINS2 = 1 << BITS2, BINS3 = 1 << BITS3;
constexpr int ITEMS = 8;                                                // float4 per lane a block aims for
constexpr int MAX_BLOCKS = 256;

struct SelState { uint32_t prefix[2]; uint32_t k[2]; };                 // of ranks i and i+1: the bits found so far, the rank under them

// per volume: two states, then the three histograms (pass 2 and 3: one per rank), then (after all volumes') the stash
constexpr int64_t HIST_WORDS = BINS1 + 2 * BINS2 + 2 * BINS3;
constexpr int64_t HEAD_BYTES = 2 * (int64_t)sizeof(SelState);

struct ThreshArgs {
    const float* x; const float* eps;
    long per4;                                     // float4 per sample
    const float* coef; const float* frame; int rows; const int* pos;
    const int* rank; const float* frac; const float* smax; float* bound;
    SelState* st1; SelState* st2;                  // [batch]: after pass 1's / pass 2's histogram
    uint32_t* h1; uint32_t* h2; uint32_t* h3;      // [batch][BINS1], [batch][2][BINS2], [batch][2][BINS3]
    uint32_t* mag;                                 // [batch][per_sample]: the bit patterns of |x0|
};

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// whether the row of volume b clips: passes 2, 3 and final need no more of it
__device__ __forceinline__ bool row_clips(const ThreshArgs& p, int b) {
    return dm3d_row_decode<false>(p.coef, nullptr, p.pos, p.rows, nullptr, b).clip;
}

// h[digit] += 1 for the lanes with `valid`; every lane of the wave calls it.  The lanes that share the first valid lane's digit add
// their count once.
__device__ __forceinline__ void hist_add(uint32_t* h, bool valid, uint32_t digit) {
    const unsigned long long todo = __ballot(valid);
    if (todo == 0) return;
    const int leader = __ffsll(todo) - 1;
    const uint32_t d0 = __shfl(digit, leader, 64);
    const unsigned long long same = __ballot(valid && digit == d0);
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&h[d0], (uint32_t)__popcll(same));
    else if (valid && digit != d0) atomicAdd(&h[digit], 1u);
}

// The bin of histogram h[NB] that holds rank k, and k's rank inside it: res[0], res[1] (shared), for every lane after the call.
// 256 lanes, NB / 256 consecutive bins each; sums are integers, so the scan's order does not matter.  k < sum(h).
template <int NB>
__device__ __forceinline__ void find_digit(const uint32_t* __restrict__ h, uint32_t k, uint32_t* wave_sum, uint32_t* res) {
    constexpr int PER = NB / 256;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t c[PER], sum = 0;
#pragma unroll
    for (int j = 0; j < PER; ++j) { c[j] = h[threadIdx.x * PER + j]; sum += c[j]; }
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t n = __shfl_up(inc, off, 64);
        if (lane >= off) inc += n;
    }
    if (lane == 63) wave_sum[wave] = inc;
    if (threadIdx.x == 0) { res[0] = 0; res[1] = 0; }
    __syncthreads();
    uint32_t below = inc - sum;
    for (int w = 0; w < wave; ++w) below += wave_sum[w];
    if (k >= below && k - below < sum) {                                 // one lane
        uint32_t rest = k - below;
        int bin = PER - 1;
        bool found = false;
#pragma unroll
        for (int j = 0; j < PER; ++j) {                                  // unrolled: c stays in registers
            if (!found && rest < c[j]) { bin = j; found = true; }
            if (!found) rest -= c[j];
        }
        res[0] = threadIdx.x * PER + bin; res[1] = rest;
    }
    __syncthreads();
}

__device__ __forceinline__ void merge_hist(uint32_t* __restrict__ dst, const uint32_t* h, int bins) {
    for (int j = threadIdx.x; j < bins; j += 256) {
        const uint32_t c = h[j];
        if (c) atomicAdd(&dst[j], c);
    }
}

__global__ __launch_bounds__(256) void thresh_clear_kernel(u32x4* __restrict__ h, long n4) {
    const u32x4 zero = {0u, 0u, 0u, 0u};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) h[i] = zero;
}

// FRAME: `eps` holds the network's output in its own frame (dm3d_update.h, dm3d_row).
template <bool FRAME>
__device__ __forceinline__ void pass1_stream(const ThreshArgs& p, uint32_t* h, long base, const dm3d_row& w) {
    for (long i0 = (long)blockIdx.x * 256; i0 < p.per4; i0 += (long)gridDim.x * 256) {      // uniform: hist_add needs whole waves
        const long i = i0 + threadIdx.x;
        const bool valid = i < p.per4;
        u32x4 m = {0u, 0u, 0u, 0u};
        if (valid) {
            const f32x4 x = reinterpret_cast<const f32x4*>(p.x)[base + i];
            const f32x4 e = reinterpret_cast<const f32x4*>(p.eps)[base + i];
#pragma unroll
            for (int k = 0; k < 4; ++k) m[k] = __float_as_uint(dm3d_row_estimate<FRAME>(w, x[k], e[k])) & 0x7fffffffu;
            reinterpret_cast<u32x4*>(p.mag)[base + i] = m;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) hist_add(h, valid, m[k] >> (BITS2 + BITS3));
    }
}

__global__ __launch_bounds__(256) void thresh_pass1_kernel(const ThreshArgs p) {
    __shared__ uint32_t h[BINS1];
    const int b = blockIdx.y;
    const dm3d_row w = dm3d_row_decode<false>(p.coef, nullptr, p.pos, p.rows, nullptr, b);      // no bound: these passes make it
    if (!w.clip) return;                                                 // uniform over the block
    for (int j = threadIdx.x; j < BINS1; j += 256) h[j] = 0;
    __syncthreads();
    const long base = (long)b * p.per4;
    if (p.frame) pass1_stream<true>(p, h, base, dm3d_row_decode<true>(p.coef, p.frame, p.pos, p.rows, nullptr, b));    // uniform over the grid
    else pass1_stream<false>(p, h, base, w);
    __syncthreads();
    merge_hist(p.h1 + (long)b * BINS1, h, BINS1);
}

// PASS 2: ranks from the table, bins from h1, counts bits 18..9 into h2.  PASS 3: state st1, bins from h2, counts bits 8..0 into h3.
template <int PASS>
__global__ __launch_bounds__(256) void thresh_pass_kernel(const ThreshArgs p) {
    constexpr int NB = PASS == 2 ? BINS2 : BINS3, NB_PREV = PASS == 2 ? BINS1 : BINS2, BITS_PREV = PASS == 2 ? BITS1 : BITS2;
    constexpr int LOW = PASS == 2 ? BITS3 : 0;                           // bits below this pass's digit
    constexpr int BITS = PASS == 2 ? BITS2 : BITS3;
    __shared__ uint32_t h[2][NB];
    __shared__ uint32_t wave_sum[4], res[2];
    const int b = blockIdx.y;
    if (!row_clips(p, b)) return;
    const long n = p.per4 * 4;
    SelState s;
    const uint32_t* prev;
    bool split;
    if (PASS == 2) {
        long i = p.rank[b];
        i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);                         // a rank outside the volume is clamped into it
        s.prefix[0] = s.prefix[1] = 0; s.k[0] = (uint32_t)i; s.k[1] = (uint32_t)(i + 1 > n - 1 ? n - 1 : i + 1);
        prev = p.h1 + (long)b * BINS1;
        split = false;
    } else {
        s = p.st1[b];
        prev = p.h2 + (long)b * 2 * BINS2;
        split = s.prefix[0] != s.prefix[1];
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        find_digit<NB_PREV>(prev + (q == 1 && split ? NB_PREV : 0), s.k[q], wave_sum, res);
        s.prefix[q] = (s.prefix[q] << BITS_PREV) | res[0]; s.k[q] = res[1];
        __syncthreads();                                                 // res is read before the next call rewrites it
    }
    split = s.prefix[0] != s.prefix[1];
    if (blockIdx.x == 0 && threadIdx.x == 0) (PASS == 2 ? p.st1 : p.st2)[b] = s;
    for (int j = threadIdx.x; j < 2 * NB; j += 256) (&h[0][0])[j] = 0;
    __syncthreads();
    const long base = (long)b * p.per4;
    for (long i0 = (long)blockIdx.x * 256; i0 < p.per4; i0 += (long)gridDim.x * 256) {
        const long i = i0 + threadIdx.x;
        const bool valid = i < p.per4;
        u32x4 m = {0u, 0u, 0u, 0u};
        if (valid) m = reinterpret_cast<const u32x4*>(p.mag)[base + i];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t pre = m[k] >> (LOW + BITS), digit = (m[k] >> LOW) & (NB - 1);
            hist_add(h[0], valid && pre == s.prefix[0], digit);
            if (split) hist_add(h[1], valid && pre == s.prefix[1], digit);
        }
    }
    __syncthreads();
    uint32_t* dst = (PASS == 2 ? p.h2 : p.h3) + (long)b * 2 * NB;
    merge_hist(dst, h[0], NB);
    if (split) merge_hist(dst + NB, h[1], NB);
}

__global__ __launch_bounds__(256) void thresh_final_kernel(const ThreshArgs p) {
    __shared__ uint32_t wave_sum[4], res[2];
    const int b = blockIdx.x;
    if (!row_clips(p, b)) {
        if (threadIdx.x == 0) p.bound[b] = 1.0f;
        return;
    }
    const SelState s = p.st2[b];
    const bool split = s.prefix[0] != s.prefix[1];
    const uint32_t* prev = p.h3 + (long)b * 2 * BINS3;
    uint32_t bits[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        find_digit<BINS3>(prev + (q == 1 && split ? BINS3 : 0), s.k[q], wave_sum, res);
        bits[q] = (s.prefix[q] << BITS3) | res[0];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float v0 = __uint_as_float(bits[0]), v1 = __uint_as_float(bits[1]);
        const float raw = __fadd_rn(v0, __fmul_rn(p.frac[b], __fsub_rn(v1, v0)));
        p.bound[b] = raw != raw ? raw : fminf(fmaxf(raw, 1.0f), p.smax[b]);
    }
}

}  // namespace

extern "C" int64_t dm3d_x0_threshold_scratch_bytes(int32_t batch, int64_t per_sample) {
    if (batch <= 0 || per_sample <= 0) return 0;
    return (int64_t)batch * (HEAD_BYTES + HIST_WORDS * 4 + per_sample * 4);
}

extern "C" int dm3d_x0_threshold(const dm3d_thresh_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "thresh: null descriptor");
    DM3D_REQUIRE(d->x && d->eps && d->coef && d->pos, "thresh: x/eps/coef/pos must be non-null");
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0 && d->per_sample <= 0x7ffffffcll,
                 "thresh: batch=%d per_sample=%lld (batch in [1, 65535], per_sample a positive multiple of 4 below 2^31)", d->batch,
                 (long long)d->per_sample);
    DM3D_REQUIRE(d->rows > 0, "thresh: rows=%d", d->rows);
    DM3D_REQUIRE(d->rank && d->frac && d->smax && d->bound && d->scratch, "thresh: rank/frac/smax/bound/scratch must be non-null");
    DM3D_REQUIRE(dm3d_aligned16(d->x) && dm3d_aligned16(d->eps) && dm3d_aligned16(d->coef) && dm3d_aligned16(d->scratch) &&
                 dm3d_aligned16(d->frame), "thresh: x/eps/coef/scratch/frame must be 16-byte aligned");
    const int64_t B = d->batch;
    char* s = static_cast<char*>(d->scratch);
    ThreshArgs a{};
    a.x = d->x; a.eps = d->eps; a.per4 = d->per_sample / 4; a.coef = d->coef; a.frame = d->frame; a.rows = d->rows; a.pos = d->pos;
    a.rank = d->rank; a.frac = d->frac; a.smax = d->smax; a.bound = d->bound;
    a.st1 = reinterpret_cast<SelState*>(s); a.st2 = a.st1 + B;
    a.h1 = reinterpret_cast<uint32_t*>(s + B * HEAD_BYTES); a.h2 = a.h1 + B * BINS1; a.h3 = a.h2 + B * 2 * BINS2;
    a.mag = a.h3 + B * 2 * BINS3;                                        // 16-byte aligned: every size above is a multiple of 16
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long clear4 = (long)(B * HIST_WORDS / 4);                      // h1, h2 and h3 of every sample are one 16-byte aligned range
    const long clear_blocks = (clear4 + 255) / 256;
    hipLaunchKernelGGL(thresh_clear_kernel, dim3((unsigned)(clear_blocks > 1024 ? 1024 : clear_blocks)), dim3(256), 0, st,
                       reinterpret_cast<u32x4*>(a.h1), clear4);
    const long blocks = (a.per4 + 256 * ITEMS - 1) / (256 * ITEMS);
    dim3 grid((unsigned)(blocks > MAX_BLOCKS ? MAX_BLOCKS : blocks), (unsigned)d->batch);
    hipLaunchKernelGGL(thresh_pass1_kernel, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(thresh_pass_kernel<2>, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(thresh_pass_kernel<3>, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(thresh_final_kernel, dim3((unsigned)d->batch), dim3(256), 0, st, a);
    return dm3d_launch_check("thresh kernels");
}
