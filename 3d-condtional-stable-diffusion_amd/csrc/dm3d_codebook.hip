// dm3d_codebook.hip — fitting the VQ codebook on the device (include/dm3d.h, dm3d_codebook_desc): per-code counts and float64 member
// sums, usage (perplexity, active codes), the exponential-moving-average update of the reference's VectorQuantizerEMA and the dead-code
// replacement of NSVQ.replace_unused_codebooks.
//
// The hot kernel is the segmented sum.  A wave owns one code and 64 neighbouring features, a lane one feature's float64 accumulator.
// The wave streams idx 256 rows at a time (four coalesced loads in flight), ballots the members of each 64-row group and queues their
// row numbers in ascending order in 64 words of LDS of its own; a full queue, and the end of idx, are drained 16 rows at a time: 16
// loads issued together, then 16 adds in queue order.  The order of the adds is therefore the order of the rows, whatever the launch
// does, and nothing is added atomically.  idx is small and stays in L2 for the k * ceil(dim / 64) waves that read it.
#include "dm3d_common.h"
#include "dm3d_philox.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int SLICE = DM3D_CODEBOOK_SLICE;         // features of a wave
constexpr int BATCH = DM3D_CODEBOOK_BATCH;         // queued rows loaded together
constexpr int MAXK = DM3D_CODEBOOK_MAX_K;
constexpr int MAXD = DM3D_CODEBOOK_MAX_DIM;
static_assert(SLICE == 64, "a lane per feature of the slice");

// ---- code_stats ---------------------------------------------------------------------------------------------------------------------
// Adds the n <= 64 queued rows to acc in queue order.  n is wave-uniform.
__device__ __forceinline__ void drain(const volatile int* queue, int n, const float* zcol, int dim, bool live, double& acc) {
    for (int j0 = 0; j0 < n; j0 += BATCH) {
        float v[BATCH];
#pragma unroll
        for (int u = 0; u < BATCH; ++u) {
            const int j = j0 + u < n ? j0 + u : n - 1;                 // the tail repeats the last row: loaded, not added
            const int row = queue[j];
            v[u] = live ? zcol[(size_t)row * dim] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < BATCH; ++u)
            if (j0 + u < n) acc = acc + (double)v[u];
    }
}

__global__ __launch_bounds__(256) void code_stats_kernel(const float* z, const int* idx, int rows, int dim, int k, int slices, int* counts,
                                                         double* sums, int* invalid) {
    __shared__ int queues[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int unit = blockIdx.x * 4 + wave;                            // (code, slice), wave-uniform
    if (unit >= k * slices) return;
    const int code = unit / slices, slice = unit - code * slices;
    const int f = slice * SLICE + lane;
    const bool live = f < dim;
    const float* zcol = z + (live ? f : 0);
    volatile int* queue = queues[wave];
    const bool counts_invalid = unit == 0;                             // one wave counts the rows no code takes

    double acc = 0.0;
    int queued = 0, members = 0, bad = 0;
    for (int base = 0; base < rows; base += 256) {                     // rows <= 2^30: base + 255 + 64 stays below 2^31
        int id[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int r = base + g * 64 + lane;
            id[g] = r < rows ? idx[r] : code;                          // past the end: neither a member (masked below) nor invalid
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int r = base + g * 64 + lane;
            const bool mine = r < rows && id[g] == code;
            const unsigned long long mask = __ballot(mine);
            if (counts_invalid) bad += __popcll(__ballot(id[g] < 0 || id[g] >= k));
            if (mask == 0) continue;                                   // wave-uniform
            const int n = __popcll(mask);
            if (queued + n > 64) {
                __builtin_amdgcn_wave_barrier();
                drain(queue, queued, zcol, dim, live, acc);
                __builtin_amdgcn_wave_barrier();
                queued = 0;
            }
            if (mine) queue[queued + __popcll(mask & ((1ull << lane) - 1ull))] = r;    // ascending: the rank of the lane among the members
            queued += n;
            members += n;
        }
    }
    __builtin_amdgcn_wave_barrier();
    drain(queue, queued, zcol, dim, live, acc);
    if (live) sums[(size_t)code * dim + f] = acc;
    if (slice == 0 && lane == 0) counts[code] = members;
    if (counts_invalid && lane == 0) invalid[0] = bad;
}

// ---- dlog and dexp: the stated operations of include/dm3d.h ---------------------------------------------------------------------------
__device__ __forceinline__ double dlog(double x) {
    int e;
    double m = frexp(x, &e);
    if (m < 0.70710678118654757) { m = m * 2.0; e = e - 1; }
    const double s = (m - 1.0) / (m + 1.0);
    const double w = s * s;
    double p = 1.0 / 25.0;
#pragma unroll
    for (int j = 23; j >= 3; j -= 2) p = p * w + 1.0 / (double)j;
    p = p * w + 1.0;
    return (double)e * 0.69314718055994529 + (2.0 * s) * p;
}

__device__ __forceinline__ double dexp(double y) {
    const double n = rint(y * 1.4426950408889634);
    const double r = (y - n * 0.693147180369123816490) - n * 1.90821492927058770002e-10;
    constexpr double fact[15] = {1.0, 1.0, 2.0, 6.0, 24.0, 120.0, 720.0, 5040.0, 40320.0, 362880.0, 3628800.0, 39916800.0, 479001600.0,
                                 6227020800.0, 87178291200.0};
    double q = 1.0 / fact[14];
#pragma unroll
    for (int j = 13; j >= 1; --j) q = q * r + 1.0 / fact[j];
    q = q * r + 1.0;
    return ldexp(q, (int)n);
}

// ---- code_usage: one workgroup ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void code_usage_kernel(const int* counts, int rows, int k, double eps, double* perplexity, int* active,
                                                         int* used_accum) {
    __shared__ double term[MAXK];
    __shared__ int live_codes;
    if (threadIdx.x == 0) live_codes = 0;
    __syncthreads();
    int mine = 0;
    for (int c = threadIdx.x; c < k; c += 256) {
        const int n = counts[c];
        const double p = (double)n / (double)rows;
        term[c] = p * dlog(p + eps);
        mine += n > 0 ? 1 : 0;
        if (used_accum) used_accum[c] += n;
    }
    if (mine) atomicAdd(&live_codes, mine);                            // integers: the order moves no bit
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll 8
        for (int c = 0; c < k; ++c) s = s + term[c];                   // ascending c: this loop is the sequential sum
        perplexity[0] = dexp(-s);
        active[0] = live_codes;
    }
}

// ---- codebook_ema: one workgroup, since n needs every N' before any row is written --------------------------------------------------------
constexpr int EMA_LANES = 1024;

// esq of row `row` by the stated rule: float32, sequential in f, multiply and add rounded separately.  dim % 4 == 0, row 16-byte aligned.
__device__ __forceinline__ float row_esq(const float* row, int dim) {
    float s = 0.0f;
    for (int f = 0; f < dim; f += 4) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + f);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float q = v[i] * v[i];
            s = s + q;
        }
    }
    return s;
}

__global__ __launch_bounds__(EMA_LANES) void codebook_ema_kernel(const int* counts, const double* sums, int k, int dim, float decay, float epsilon,
                                                                float* cluster_size, float* ema_w, float* codebook, float* esq) {
    __shared__ float size_new[MAXK];
    __shared__ float scale;
    const float om = 1.0f - decay;
    for (int c = threadIdx.x; c < k; c += EMA_LANES) {
        const float a = cluster_size[c] * decay;
        const float b = om * (float)counts[c];
        size_new[c] = a + b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double n = 0.0;
#pragma unroll 8
        for (int c = 0; c < k; ++c) n = n + (double)size_new[c];       // ascending c
        scale = (float)(n / (n + (double)epsilon));
    }
    __syncthreads();
    const float g = scale;
    for (int c = threadIdx.x; c < k; c += EMA_LANES) cluster_size[c] = size_new[c];
    const int total = k * dim;                                         // <= 2^22
    for (int i = threadIdx.x; i < total; i += EMA_LANES) {
        const int c = i / dim;
        const float a = ema_w[i] * decay;
        const float b = om * (float)sums[i];
        const float w = a + b;
        ema_w[i] = w;
        const float size = size_new[c];
        if (size != 0.0f) {                                            // N' == 0: the code has never had a member and keeps its row
            const float e = w / size;
            codebook[i] = e * g;
        }
    }
    __threadfence();
    __syncthreads();                                                   // the rows are written: a lane per code sums its row in order
    for (int c = threadIdx.x; c < k; c += EMA_LANES)
        if (size_new[c] != 0.0f) esq[c] = row_esq(codebook + (size_t)c * dim, dim);
}

// ---- codebook_replace ------------------------------------------------------------------------------------------------------------------------
// One workgroup: U and V in ascending order, the shuffle of the tiled list, map[c].
__global__ __launch_bounds__(256) void replace_plan_kernel(const int* used, int k, int num_batches, double threshold, int draw, uint64_t seed,
                                                          int* used_count, int* unused_count, int* map) {
    __shared__ int list[MAXK];                                         // U from the front, V from the back: list[k - 1 - j] = V[j]
    __shared__ unsigned long long keyed[MAXK];                         // (key << 32) | i, sorted ascending
    __shared__ int before[257];                                        // used codes in front of a lane's run of codes
    const int tid = threadIdx.x;
    const int per = (k + 255) / 256;                                   // a lane owns `per` neighbouring codes
    const int c0 = tid * per, c1 = c0 + per < k ? c0 + per : k;
    int mine = 0;
    for (int c = c0; c < c1; ++c) mine += (double)used[c] / (double)num_batches < threshold ? 0 : 1;
    before[tid + 1] = mine;
    if (tid == 0) before[0] = 0;
    __syncthreads();
    if (tid == 0)
        for (int t = 1; t <= 256; ++t) before[t] += before[t - 1];
    __syncthreads();
    const int nu = before[256], nv = k - nu;
    int u = before[tid], v = (c0 < k ? c0 : k) - u;                    // codes in front of c0 are used or unused
    for (int c = c0; c < c1; ++c) {
        const bool dead = (double)used[c] / (double)num_batches < threshold;
        if (dead) list[k - 1 - v++] = c; else list[u++] = c;
        if (nu == 0) map[c] = c;                                       // no used code: noise on every row
        else if (!dead) map[c] = -1;                                   // a used row stays; an unused one gets its source below, once
    }
    if (tid == 0) { used_count[0] = nu; unused_count[0] = nv; }
    __syncthreads();
    if (nu == 0 || nv == 0) return;
    if (nu >= nv) {
        for (int j = tid; j < nv; j += 256) map[list[k - 1 - j]] = list[j];
        return;
    }
    const int entries = nu * (nv / nu + 1);                            // nv < entries <= nu + nv = k
    int pow2 = 1;
    while (pow2 < entries) pow2 <<= 1;
    for (int i = tid; i < pow2; i += 256) {
        unsigned long long key = ~0ull;                                // the padding sorts behind every entry
        if (i < entries) {
            uint32_t ctr[4] = {(uint32_t)i, 0u, (uint32_t)draw, (uint32_t)DM3D_STREAM_CODEBOOK_SHUFFLE};
            philox4x32_10(ctr, (uint32_t)seed, (uint32_t)(seed >> 32));
            key = ((unsigned long long)ctr[0] << 32) | (unsigned long long)i;
        }
        keyed[i] = key;
    }
    for (int size = 2; size <= pow2; size <<= 1)                       // bitonic sort: the keys are distinct, so the result is the sorted list
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int i = tid; i < pow2; i += 256) {
                const int j = i ^ stride;
                if (j > i) {
                    const unsigned long long a = keyed[i], b = keyed[j];
                    const bool up = (i & size) == 0;
                    if ((a > b) == up) { keyed[i] = b; keyed[j] = a; }
                }
            }
        }
    __syncthreads();
    for (int j = tid; j < nv; j += 256) map[list[k - 1 - j]] = list[(int)(keyed[j] & 0xffffffffull) % nu];
}

// A workgroup of one wave per code: the row of map[c] plus noise, its esq, the copied EMA state; used[c] = 0.
__global__ __launch_bounds__(64) void replace_apply_kernel(const int* map, int k, int dim, float noise_scale, int draw, uint64_t seed,
                                                          float* codebook, float* esq, float* cluster_size, float* ema_w, int* used) {
    __shared__ float row[MAXD];
    const int c = blockIdx.x, lane = threadIdx.x;
    if (lane == 0) used[c] = 0;
    const int s = map[c];                                              // wave-uniform
    if (s < 0) return;
    const int quads = dim >> 2;
    for (int q = lane; q < quads; q += 64) {
        const f32x4 z = philox_normal4((uint64_t)c * (uint64_t)quads + (uint64_t)q, (uint32_t)draw, (uint32_t)DM3D_STREAM_CODEBOOK, seed);
        const f32x4 src = *reinterpret_cast<const f32x4*>(codebook + (size_t)s * dim + 4 * q);
        f32x4 out;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float t = noise_scale * z[i];
            out[i] = src[i] + t;
        }
        *reinterpret_cast<f32x4*>(codebook + (size_t)c * dim + 4 * q) = out;
        *reinterpret_cast<f32x4*>(row + 4 * q) = out;
        if (s != c && ema_w)
            *reinterpret_cast<f32x4*>(ema_w + (size_t)c * dim + 4 * q) = *reinterpret_cast<const f32x4*>(ema_w + (size_t)s * dim + 4 * q);
    }
    __syncthreads();
    if (lane == 0) {
        esq[c] = row_esq(row, dim);
        if (s != c && cluster_size) cluster_size[c] = cluster_size[s];
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
bool aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

struct Buf { const void* p; uint64_t bytes; const char* name; bool written; };

// Null (unless optional: p == nullptr is then skipped by the caller), alignment, and no written buffer sharing a byte with another one.
int check_buffers(const char* who, const Buf* bufs, int n, const unsigned* align) {
    for (int i = 0; i < n; ++i) DM3D_REQUIRE(bufs[i].p != nullptr, "%s: %s must be non-null", who, bufs[i].name);
    for (int i = 0; i < n; ++i) DM3D_REQUIRE(aligned(bufs[i].p, align[i]), "%s: %s must be %u-byte aligned", who, bufs[i].name, align[i]);
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j)
            if (bufs[i].written || bufs[j].written)
                DM3D_REQUIRE(!dm3d_ranges_overlap(bufs[i].p, bufs[i].bytes, bufs[j].p, bufs[j].bytes), "%s: %s overlaps %s", who, bufs[i].name,
                             bufs[j].name);
    return DM3D_OK;
}

int check_shape(const dm3d_codebook_desc* d, const char* who, bool rows) {
    DM3D_REQUIRE(d != nullptr, "%s: null descriptor", who);
    DM3D_REQUIRE(d->k >= 1, "%s: k=%d (at least 1)", who, d->k);
    DM3D_REQUIRE(d->k <= DM3D_CODEBOOK_MAX_K, "%s: k=%d exceeds DM3D_CODEBOOK_MAX_K=%d", who, d->k, DM3D_CODEBOOK_MAX_K);
    if (rows) {
        DM3D_REQUIRE(d->rows >= 1, "%s: rows=%d (at least 1)", who, d->rows);
        DM3D_REQUIRE(d->rows <= DM3D_CODEBOOK_MAX_ROWS, "%s: rows=%d exceeds DM3D_CODEBOOK_MAX_ROWS=%d", who, d->rows, DM3D_CODEBOOK_MAX_ROWS);
    }
    return DM3D_OK;
}

int check_dim(const dm3d_codebook_desc* d, const char* who) {
    DM3D_REQUIRE(d->dim >= 4, "%s: dim=%d (at least 4)", who, d->dim);
    DM3D_REQUIRE(d->dim <= DM3D_CODEBOOK_MAX_DIM, "%s: dim=%d exceeds DM3D_CODEBOOK_MAX_DIM=%d", who, d->dim, DM3D_CODEBOOK_MAX_DIM);
    DM3D_REQUIRE(d->dim % 4 == 0, "%s: dim=%d must be a multiple of 4", who, d->dim);
    return DM3D_OK;
}

}  // namespace

extern "C" int dm3d_code_stats(const dm3d_codebook_desc* d, void* stream) {
    const char* who = "code_stats";
    int rc = check_shape(d, who, true);
    if (rc != DM3D_OK || (rc = check_dim(d, who)) != DM3D_OK) return rc;
    const uint64_t kd = (uint64_t)d->k * d->dim;
    const Buf bufs[5] = {{d->z, (uint64_t)d->rows * d->dim * 4, "z", false}, {d->idx, (uint64_t)d->rows * 4, "idx", false},
                         {d->counts, (uint64_t)d->k * 4, "counts", true}, {d->sums, kd * 8, "sums", true}, {d->invalid, 4, "invalid", true}};
    const unsigned align[5] = {4, 4, 4, 8, 4};
    if ((rc = check_buffers(who, bufs, 5, align)) != DM3D_OK) return rc;
    const int slices = (d->dim + SLICE - 1) / SLICE;
    const unsigned blocks = (unsigned)((d->k * slices + 3) / 4);
    hipLaunchKernelGGL(code_stats_kernel, dim3(blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d->z, d->idx, d->rows, d->dim, d->k, slices,
                       d->counts, d->sums, d->invalid);
    return dm3d_launch_check("code_stats_kernel");
}

extern "C" int dm3d_code_usage(const dm3d_codebook_desc* d, void* stream) {
    const char* who = "code_usage";
    int rc = check_shape(d, who, true);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->eps >= 0.0, "%s: eps=%g (at least 0)", who, d->eps);
    Buf bufs[4] = {{d->counts, (uint64_t)d->k * 4, "counts", false}, {d->perplexity, 8, "perplexity", true}, {d->active, 4, "active", true},
                   {d->used_accum, (uint64_t)d->k * 4, "used_accum", true}};
    const unsigned align[4] = {4, 8, 4, 4};
    if ((rc = check_buffers(who, bufs, d->used_accum ? 4 : 3, align)) != DM3D_OK) return rc;
    hipLaunchKernelGGL(code_usage_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), d->counts, d->rows, d->k, d->eps, d->perplexity,
                       d->active, d->used_accum);
    return dm3d_launch_check("code_usage_kernel");
}

extern "C" int dm3d_codebook_ema(const dm3d_codebook_desc* d, void* stream) {
    const char* who = "codebook_ema";
    int rc = check_shape(d, who, false);
    if (rc != DM3D_OK || (rc = check_dim(d, who)) != DM3D_OK) return rc;
    DM3D_REQUIRE(d->decay >= 0.0f && d->decay <= 1.0f, "%s: decay=%g (0 to 1)", who, (double)d->decay);
    DM3D_REQUIRE(d->epsilon >= 0.0f, "%s: epsilon=%g (at least 0)", who, (double)d->epsilon);
    const uint64_t kd = (uint64_t)d->k * d->dim;
    const Buf bufs[6] = {{d->counts, (uint64_t)d->k * 4, "counts", false}, {d->sums, kd * 8, "sums", false},
                         {d->cluster_size, (uint64_t)d->k * 4, "cluster_size", true}, {d->ema_w, kd * 4, "ema_w", true},
                         {d->codebook, kd * 4, "codebook", true}, {d->esq, (uint64_t)d->k * 4, "esq", true}};
    const unsigned align[6] = {4, 8, 4, 16, 16, 4};
    if ((rc = check_buffers(who, bufs, 6, align)) != DM3D_OK) return rc;
    hipLaunchKernelGGL(codebook_ema_kernel, dim3(1), dim3(EMA_LANES), 0, static_cast<hipStream_t>(stream), d->counts, d->sums, d->k, d->dim, d->decay,
                       d->epsilon, d->cluster_size, d->ema_w, d->codebook, d->esq);
    return dm3d_launch_check("codebook_ema_kernel");
}

extern "C" int dm3d_codebook_replace(const dm3d_codebook_desc* d, void* stream) {
    const char* who = "codebook_replace";
    int rc = check_shape(d, who, false);
    if (rc != DM3D_OK || (rc = check_dim(d, who)) != DM3D_OK) return rc;
    DM3D_REQUIRE(d->num_batches >= 1, "%s: num_batches=%d (at least 1)", who, d->num_batches);
    DM3D_REQUIRE(d->threshold == d->threshold, "%s: threshold is NaN", who);
    DM3D_REQUIRE(d->noise_scale - d->noise_scale == 0.0f, "%s: noise_scale must be finite", who);
    DM3D_REQUIRE((d->cluster_size == nullptr) == (d->ema_w == nullptr), "%s: cluster_size and ema_w are given together or not at all", who);
    const uint64_t kd = (uint64_t)d->k * d->dim, k4 = (uint64_t)d->k * 4;
    Buf bufs[8] = {{d->codebook, kd * 4, "codebook", true}, {d->esq, k4, "esq", true}, {d->used, k4, "used", true},
                   {d->used_count, 4, "used_count", true}, {d->unused_count, 4, "unused_count", true}, {d->map, k4, "map", true},
                   {d->cluster_size, k4, "cluster_size", true}, {d->ema_w, kd * 4, "ema_w", true}};
    const unsigned align[8] = {16, 4, 4, 4, 4, 4, 4, 16};
    if ((rc = check_buffers(who, bufs, d->ema_w ? 8 : 6, align)) != DM3D_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(replace_plan_kernel, dim3(1), dim3(256), 0, st, d->used, d->k, d->num_batches, d->threshold, d->draw, d->seed, d->used_count,
                       d->unused_count, d->map);
    if ((rc = dm3d_launch_check("replace_plan_kernel")) != DM3D_OK) return rc;
    hipLaunchKernelGGL(replace_apply_kernel, dim3((unsigned)d->k), dim3(64), 0, st, d->map, d->k, d->dim, d->noise_scale, d->draw, d->seed, d->codebook,
                       d->esq, d->cluster_size, d->ema_w, d->used);
    return dm3d_launch_check("replace_apply_kernel");
}
