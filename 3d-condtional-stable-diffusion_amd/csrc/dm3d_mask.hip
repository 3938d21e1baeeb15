// dm3d_mask.hip — scores of the mask channels (include/dm3d.h, dm3d_mask_desc): overlap counts, surfaces, the exact squared Euclidean
// distance transform and the directed surface-distance statistics behind Dice, IoU, Hausdorff and ASSD.  The float32 NDHWC tensors are
// read in place through their channel windows; every quantity up to the last kernel is an integer (counts by integer atomics, squared
// distances by min-plus over int32, a histogram of them by integer atomics), so no result depends on the order blocks run in, and the
// last kernel forms its float64 values from the histogram in a fixed order: runs repeat bitwise.  Plain HIP: no MFMA, no float atomics.
// The window and volume checks and the tiling of the three transform passes are dm3d_volume.h's.
#include "dm3d_volume.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int MAXE = DM3D_EDT_MAX_EXTENT;          // longest column staged in LDS
constexpr int LANES = DM3D_LINE_LANES, LDT = DM3D_LINE_LDT;   // columns a block stages side by side; LDS row of one column position
constexpr int BIG = 0x3fffffff;                    // "no feature yet": BIG + 511^2 stays below INT32_MAX
constexpr int VOX = 1024;                          // voxels a block of the streaming kernels walks (4 per lane)

__global__ __launch_bounds__(256) void mask_zero_kernel(unsigned* p, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = 0u;
}

struct FeatArgs {
    const float* x; const float* y;                // y may be null (dm3d_edt)
    int d, h, w, cx, cy, x0c, y0c, nc;
    float thr;
    int x_foreground;                              // fx takes the mask itself, not its surface
    unsigned long long* counts;                    // [batch * nc][3] or null
    uint8_t* fx; uint8_t* fy;                      // [batch * nc][d][h][w] or null
};

// value > thr at voxel (z, y, x) of one channel of one volume; outside the volume and NaN are background
__device__ __forceinline__ bool mask_at(const float* src, int cs, int z, int y, int x, int d, int h, int w, float thr) {
    if ((unsigned)z >= (unsigned)d || (unsigned)y >= (unsigned)h || (unsigned)x >= (unsigned)w) return false;
    return src[(((long)z * h + y) * w + x) * cs] > thr;
}
__device__ __forceinline__ bool surface_at(const float* src, int cs, int z, int y, int x, int d, int h, int w, float thr) {
    const bool inner = mask_at(src, cs, z - 1, y, x, d, h, w, thr) && mask_at(src, cs, z + 1, y, x, d, h, w, thr) &&
                       mask_at(src, cs, z, y - 1, x, d, h, w, thr) && mask_at(src, cs, z, y + 1, x, d, h, w, thr) &&
                       mask_at(src, cs, z, y, x - 1, d, h, w, thr) && mask_at(src, cs, z, y, x + 1, d, h, w, thr);
    return !inner;
}

// Grid (ceil(dhw / VOX), batch * nc).  A lane walks voxels v0 + r * 256 + lane, so a wave reads consecutive voxels.
__global__ __launch_bounds__(256) void mask_feature_kernel(const FeatArgs p) {
    __shared__ unsigned red[4][3];
    const int bc = blockIdx.y, b = bc / p.nc, c = bc % p.nc;
    const long vol = (long)p.d * p.h * p.w;
    const float* xs = p.x + b * vol * p.cx + p.x0c + c;
    const float* ys = p.y ? p.y + b * vol * p.cy + p.y0c + c : nullptr;
    unsigned n[3] = {0u, 0u, 0u};
#pragma unroll
    for (int r = 0; r < VOX / 256; ++r) {
        const long v = (long)blockIdx.x * VOX + r * 256 + threadIdx.x;
        if (v >= vol) continue;
        const int x = (int)(v % p.w), y = (int)((v / p.w) % p.h), z = (int)(v / ((long)p.w * p.h));
        const bool mx = xs[v * p.cx] > p.thr;
        const bool my = ys ? ys[v * p.cy] > p.thr : false;
        n[0] += mx; n[1] += my; n[2] += mx & my;
        if (p.fx) p.fx[bc * vol + v] = mx && (p.x_foreground || surface_at(xs, p.cx, z, y, x, p.d, p.h, p.w, p.thr));
        if (p.fy && ys) p.fy[bc * vol + v] = my && surface_at(ys, p.cy, z, y, x, p.d, p.h, p.w, p.thr);
    }
    if (!p.counts) return;                                                      // uniform over the grid
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n[k] += __shfl_xor(n[k], off, 64);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 3; ++k) red[threadIdx.x >> 6][k] = n[k];
    __syncthreads();
    if (threadIdx.x < 3) {
        const unsigned t = red[0][threadIdx.x] + red[1][threadIdx.x] + red[2][threadIdx.x] + red[3][threadIdx.x];
        if (t) atomicAdd(p.counts + (long)bc * 3 + threadIdx.x, (unsigned long long)t);
    }
}

struct PassArgs {
    const uint8_t* feat;                           // first pass: the features (a column position holds 0 where feat, BIG elsewhere)
    int* map;                                      // in place (first pass: out only)
    dm3d_line_pass line;                           // a line is a column here, of length 1 .. MAXE
    int first, last;                               // last: values of BIG and above leave as INT32_MAX
};

// out[i] = min_j (i - j)^2 + g[j] for LANES neighbouring columns of one group, in place.  The columns are staged in LDS as [n][LDT]
// (dm3d_line_walk); a 32-lane half of a wave owns the 32 columns at one j, so its LDS reads are 32 consecutive banks, and each lane
// carries 4 outputs of its column per read.  The results go through a second LDS image so that the stores run in the order of the loads.
template <bool ALONG>
__global__ __launch_bounds__(256) void edt_pass_kernel(const PassArgs p) {
    extern __shared__ int lds[];
    const int n = p.line.n;
    int* col = lds;
    int* res = lds + n * LDT;
    const dm3d_line_block blk = dm3d_line_block_of(p.line);
    dm3d_line_walk<ALONG>(p.line, blk, [&](int at, long off, bool live) {
        int v = BIG;
        if (live) v = p.first ? (p.feat[off] ? 0 : BIG) : p.map[off];
        col[at] = v;
    });
    __syncthreads();
    const int xl = threadIdx.x & (LANES - 1), rg = threadIdx.x / LANES;
    for (int i0 = rg * 4; i0 < n; i0 += 4 * (256 / LANES)) {
        int o0 = BIG, o1 = BIG, o2 = BIG, o3 = BIG;
#pragma unroll 4
        for (int j = 0; j < n; ++j) {
            const int g = col[j * LDT + xl], dj = i0 - j;
            o0 = min(o0, dj * dj + g);
            o1 = min(o1, (dj + 1) * (dj + 1) + g);
            o2 = min(o2, (dj + 2) * (dj + 2) + g);
            o3 = min(o3, (dj + 3) * (dj + 3) + g);
        }
        const int o[4] = {o0, o1, o2, o3};
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (i0 + r < n) res[(i0 + r) * LDT + xl] = o[r] >= BIG ? (p.last ? INT_MAX : BIG) : o[r];
    }
    __syncthreads();
    dm3d_line_walk<ALONG>(p.line, blk, [&](int at, long off, bool live) {
        if (live) p.map[off] = res[at];
    });
}

// Grid (ceil(dhw / VOX), batch * nc): hist[bc][dir][k] += 1 for every voxel of `surf` whose squared distance is k; a distance of `bins`
// and above (INT32_MAX: the other surface is empty) goes to slot `bins`, so the slots always add up to the surface's voxel count.  Up to
// four values shared by lanes of a wave are added once per wave: neighbouring surface voxels mostly lie at a few distances.
__global__ __launch_bounds__(256) void mask_hist_kernel(const uint8_t* surf, const int* map, unsigned* hist, long vol, int bins, int dir) {
    const int bc = blockIdx.y;
    unsigned* h = hist + ((long)bc * 2 + dir) * (bins + 1);
#pragma unroll
    for (int r = 0; r < VOX / 256; ++r) {
        const long v = (long)blockIdx.x * VOX + r * 256 + threadIdx.x;
        bool live = v < vol && surf[bc * vol + v];
        int k = 0;
        if (live) {
            k = map[bc * vol + v];
            k = (unsigned)k < (unsigned)bins ? k : bins;
        }
        for (int round = 0; round < 4; ++round) {
            const unsigned long long act = __ballot(live);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const int k0 = __shfl(k, leader, 64);
            const unsigned long long same = __ballot(live && k == k0);
            if ((int)(threadIdx.x & 63) == leader) atomicAdd(h + k0, (unsigned)__popcll(same));
            if (k == k0) live = false;
        }
        if (live) atomicAdd(h + k, 1u);
    }
}

struct StatArgs {
    const unsigned* hist;                          // [batch * nc][2][bins + 1]
    double* out;                                   // [batch * nc][5]: hd, hd_percentile, assd, surface_x, surface_y
    int bins;
    double q;                                      // percentile / 100
};

// Block per (volume, channel); direction 0 is X -> Y (the map of Y's surface at X's surface voxels), 1 is Y -> X.  Lane t owns the run
// of k [t * run, (t + 1) * run): its count, its sum of count[k] * sqrt(k) in ascending k, its largest occupied k.  Lane 0 adds the 256
// runs in ascending order and forms the ranks; a second walk of the runs, each from its exclusive prefix, finds the two order
// statistics.  percentile: numpy's default (linear) rule, operation by operation: r = (n - 1) * q, lo = floor(r), t = r - lo,
// a + (b - a) * t for t < 0.5 and b - (b - a) * (1 - t) from there.
__global__ __launch_bounds__(256) void mask_stat_kernel(const StatArgs p) {
    __shared__ unsigned long long cnt[256], pre[256];
    __shared__ double sum[256];
    __shared__ int top[256];
    __shared__ unsigned long long rank[2];
    __shared__ int kstat[2];
    __shared__ double res[2][4];                                                // per direction: n, max, percentile, sum
    const int bc = blockIdx.x, t = threadIdx.x;
    const int run = (p.bins + 255) / 256;
    const int k_lo = min(t * run, p.bins), k_hi = min(k_lo + run, p.bins);
    for (int dir = 0; dir < 2; ++dir) {
        const unsigned* h = p.hist + ((long)bc * 2 + dir) * (p.bins + 1);
        unsigned long long c = 0;
        double s = 0.0;
        int mx = -1;
        for (int k = k_lo; k < k_hi; ++k) {
            const unsigned ck = h[k];
            if (ck) {
                c += ck;
                s += (double)ck * sqrt((double)k);
                mx = k;
            }
        }
        cnt[t] = c; sum[t] = s; top[t] = mx;
        __syncthreads();
        if (t == 0) {
            unsigned long long n = 0;
            double tot = 0.0;
            int m = -1;
            for (int i = 0; i < 256; ++i) {
                pre[i] = n;
                n += cnt[i];
                tot += sum[i];
                m = top[i] >= 0 ? top[i] : m;
            }
            const unsigned long long far = h[p.bins];                           // voxels whose map is INT32_MAX: the other surface is empty
            res[dir][0] = (double)(n + far);
            res[dir][1] = far || !n ? NAN : sqrt((double)m);
            res[dir][3] = far || !n ? NAN : tot;
            const double r = (double)(n ? n - 1 : 0) * p.q;
            const double fl = floor(r);
            rank[0] = (unsigned long long)fl;
            rank[1] = n && rank[0] + 1 < n ? rank[0] + 1 : rank[0];
            res[dir][2] = far || !n ? NAN : r - fl;                             // t of the rule, replaced by the value below
            kstat[0] = kstat[1] = 0;
        }
        __syncthreads();
        {
            unsigned long long cum = pre[t];
            const unsigned long long r0 = rank[0], r1 = rank[1];
            for (int k = k_lo; k < k_hi; ++k) {
                const unsigned long long nxt = cum + h[k];
                if (cum <= r0 && r0 < nxt) kstat[0] = k;                        // one lane, one k: the ranks lie below n
                if (cum <= r1 && r1 < nxt) kstat[1] = k;
                cum = nxt;
            }
        }
        __syncthreads();
        if (t == 0 && !isnan(res[dir][2])) {
            const double a = sqrt((double)kstat[0]), b = sqrt((double)kstat[1]), g = res[dir][2], diff = b - a;
            res[dir][2] = g >= 0.5 ? b - diff * (1.0 - g) : a + diff * g;
        }
        __syncthreads();
    }
    if (t == 0) {
        double* o = p.out + (long)bc * 5;
        const double nx = res[0][0], ny = res[1][0];
        const bool ok = nx > 0.0 && ny > 0.0;
        o[0] = ok ? fmax(res[0][1], res[1][1]) : NAN;
        o[1] = ok ? fmax(res[0][2], res[1][2]) : NAN;
        o[2] = ok ? (res[0][3] + res[1][3]) / (nx + ny) : NAN;
        o[3] = nx;
        o[4] = ny;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
int check_common(const dm3d_mask_desc* d, const char* who, bool pair) {
    DM3D_REQUIRE(d != nullptr, "%s: null descriptor", who);
    DM3D_REQUIRE(d->x != nullptr, "%s: x must be non-null", who);
    DM3D_REQUIRE(!pair || d->y != nullptr, "%s: y must be non-null", who);
    int rc = dm3d_check_volume(who, d->batch, d->d, d->h, d->w, d->nc, MAXE, "DM3D_EDT_MAX_EXTENT");
    if (rc != DM3D_OK || (rc = dm3d_check_window(who, "x", d->x0c, d->nc, d->cx)) != DM3D_OK) return rc;
    if (pair && (rc = dm3d_check_window(who, "y", d->y0c, d->nc, d->cy)) != DM3D_OK) return rc;
    DM3D_REQUIRE(isfinite(d->threshold), "%s: threshold=%g (finite)", who, (double)d->threshold);
    return DM3D_OK;
}

int64_t voxels(const dm3d_mask_desc* d) { return (int64_t)d->batch * d->nc * d->d * d->h * d->w; }
int64_t bins_of(const dm3d_mask_desc* d) {
    return (int64_t)(d->d - 1) * (d->d - 1) + (int64_t)(d->h - 1) * (d->h - 1) + (int64_t)(d->w - 1) * (d->w - 1) + 1;
}

int launch_zero(void* p, int64_t words, hipStream_t st) {
    hipLaunchKernelGGL(mask_zero_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, static_cast<unsigned*>(p), (long)words);
    return dm3d_launch_check("mask_zero_kernel");
}

int launch_features(const dm3d_mask_desc* d, bool pair, int x_foreground, int64_t* counts, uint8_t* fx, uint8_t* fy, hipStream_t st) {
    FeatArgs a{};
    a.x = d->x; a.y = pair ? d->y : nullptr;
    a.d = d->d; a.h = d->h; a.w = d->w; a.cx = d->cx; a.cy = d->cy; a.x0c = d->x0c; a.y0c = d->y0c; a.nc = d->nc;
    a.thr = d->threshold; a.x_foreground = x_foreground;
    a.counts = reinterpret_cast<unsigned long long*>(counts); a.fx = fx; a.fy = fy;
    const int64_t vol = (int64_t)d->d * d->h * d->w;
    hipLaunchKernelGGL(mask_feature_kernel, dim3((unsigned)((vol + VOX - 1) / VOX), (unsigned)(d->batch * d->nc)), dim3(256), 0, st, a);
    return dm3d_launch_check("mask_feature_kernel");
}

// The three passes of the squared transform of `feat` [batch * nc][d][h][w] into `map` (same layout): along w from the features, then
// along h and along d in place.  Every pass runs, also along an axis of extent 1: the last one writes INT32_MAX for "no feature".
int launch_edt(const dm3d_mask_desc* d, const uint8_t* feat, int* map, hipStream_t st) {
    static std::atomic<bool> lds_set[64];
    const size_t lds_max = (size_t)2 * MAXE * LDT * sizeof(int);
    const int dev = dm3d_dyn_lds(lds_max, lds_set, "edt", edt_pass_kernel<true>, edt_pass_kernel<false>);
    if (dev < 0) return dev;
    static const char* const names[3] = {"edt_pass_kernel (w)", "edt_pass_kernel (h)", "edt_pass_kernel (d)"};
    PassArgs a{};
    a.feat = feat; a.map = map;
    for (int axis = 0; axis < 3; ++axis) {
        const int64_t blocks = dm3d_line_pass_fill(&a.line, axis, (int64_t)d->batch * d->nc, d->d, d->h, d->w);
        a.first = axis == 0; a.last = axis == 2;
        hipLaunchKernelGGL(axis == 0 ? edt_pass_kernel<true> : edt_pass_kernel<false>, dim3((unsigned)blocks), dim3(256),
                           (size_t)2 * a.line.n * LDT * sizeof(int), st, a);
        const int rc = dm3d_launch_check(names[axis]);
        if (rc != DM3D_OK) return rc;
    }
    return DM3D_OK;
}

int check_edt_grid(const dm3d_mask_desc* d, const char* who) {                  // cannot fail under the limits above; kept beside the launches
    int64_t blocks = 0;
    const int axis = dm3d_line_grid_fault((int64_t)d->batch * d->nc, d->d, d->h, d->w, &blocks);
    DM3D_REQUIRE(axis < 0, "%s: %lld blocks of the %s pass exceed the grid", who, (long long)blocks, dm3d_line_axis[axis < 0 ? 0 : axis]);
    return DM3D_OK;
}

}  // namespace

extern "C" int dm3d_mask_overlap(const dm3d_mask_desc* d, void* stream) {
    int rc = check_common(d, "mask_overlap", true);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->counts != nullptr, "mask_overlap: counts must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->counts, 8), "mask_overlap: counts must be 8-byte aligned");
    DM3D_REQUIRE((d->surf_x == nullptr) == (d->surf_y == nullptr), "mask_overlap: surf_x and surf_y must be both given or both null");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = launch_zero(d->counts, 6 * (int64_t)d->batch * d->nc, st)) != DM3D_OK) return rc;
    return launch_features(d, true, 0, d->counts, d->surf_x, d->surf_y, st);
}

extern "C" int dm3d_edt(const dm3d_mask_desc* d, void* stream) {
    int rc = check_common(d, "edt", false);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->map != nullptr && d->masks != nullptr, "edt: map and masks must be non-null");
    DM3D_REQUIRE(d->of == DM3D_EDT_SURFACE || d->of == DM3D_EDT_FOREGROUND, "edt: of=%d (DM3D_EDT_SURFACE or DM3D_EDT_FOREGROUND)", d->of);
    DM3D_REQUIRE(dm3d_aligned(d->map, 4), "edt: map must be 4-byte aligned");
    const int64_t V = voxels(d);
    DM3D_REQUIRE(d->masks_elems >= V, "edt: masks holds %lld bytes, %lld are needed (batch * nc * d * h * w)", (long long)d->masks_elems, (long long)V);
    if ((rc = check_edt_grid(d, "edt")) != DM3D_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = launch_features(d, false, d->of == DM3D_EDT_FOREGROUND, nullptr, d->masks, nullptr, st)) != DM3D_OK) return rc;
    return launch_edt(d, d->masks, d->map, st);
}

extern "C" int dm3d_surface_distance(const dm3d_mask_desc* d, void* stream) {
    int rc = check_common(d, "surface_distance", true);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->out != nullptr && d->masks != nullptr && d->work != nullptr, "surface_distance: out, masks and work must be non-null");
    DM3D_REQUIRE(d->percentile > 0.0 && d->percentile <= 100.0, "surface_distance: percentile=%g (in (0, 100])", d->percentile);
    DM3D_REQUIRE(dm3d_aligned(d->out, 8) && dm3d_aligned(d->counts, 8), "surface_distance: out and counts must be 8-byte aligned");
    DM3D_REQUIRE(dm3d_aligned(d->work, 4), "surface_distance: work must be 4-byte aligned");
    const int64_t V = voxels(d), bc = (int64_t)d->batch * d->nc, bins = bins_of(d);
    DM3D_REQUIRE(d->masks_elems >= 2 * V, "surface_distance: masks holds %lld bytes, %lld are needed (2 * batch * nc * d * h * w)",
                 (long long)d->masks_elems, (long long)(2 * V));
    const int64_t need = V + 2 * bc * (bins + 1);
    DM3D_REQUIRE(d->work_elems >= need, "surface_distance: work holds %lld int32, %lld are needed (batch * nc * (d * h * w + 2 * (%lld + 1)))",
                 (long long)d->work_elems, (long long)need, (long long)bins);
    if ((rc = check_edt_grid(d, "surface_distance")) != DM3D_OK) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    uint8_t* sx = d->masks;
    uint8_t* sy = d->masks + V;
    int* map = d->work;
    unsigned* hist = reinterpret_cast<unsigned*>(d->work + V);
    const int64_t vol = (int64_t)d->d * d->h * d->w;
    const dim3 grid((unsigned)((vol + VOX - 1) / VOX), (unsigned)bc);
    if ((rc = launch_zero(hist, 2 * bc * (bins + 1), st)) != DM3D_OK) return rc;
    if (d->counts && (rc = launch_zero(d->counts, 6 * bc, st)) != DM3D_OK) return rc;
    if ((rc = launch_features(d, true, 0, d->counts, sx, sy, st)) != DM3D_OK) return rc;
    for (int dir = 0; dir < 2; ++dir) {                                         // 0: the map of Y's surface read at X's; 1: the reverse
        if ((rc = launch_edt(d, dir ? sx : sy, map, st)) != DM3D_OK) return rc;
        hipLaunchKernelGGL(mask_hist_kernel, grid, dim3(256), 0, st, dir ? sy : sx, map, hist, (long)vol, (int)bins, dir);
        if ((rc = dm3d_launch_check("mask_hist_kernel")) != DM3D_OK) return rc;
    }
    StatArgs s{};
    s.hist = hist; s.out = d->out; s.bins = (int)bins; s.q = d->percentile / 100.0;
    hipLaunchKernelGGL(mask_stat_kernel, dim3((unsigned)bc), dim3(256), 0, st, s);
    return dm3d_launch_check("mask_stat_kernel");
}
