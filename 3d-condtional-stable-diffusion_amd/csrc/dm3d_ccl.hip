// dm3d_ccl.hip — 3-D connected components of binarised masks (include/dm3d.h, dm3d_ccl_desc): labels in scipy.ndimage.label's numbering,
// the component count, the largest component, and the three filters built on them (keep the largest, drop small ones, fill holes).
// The float32 NDHWC tensor is read in place through its channel window; everything written with a voxel axis is channel-planar.
//
// Union-find with "the parent is never above the child": a workgroup labels one BD x BH x BW brick in LDS, the seam kernel unites across
// brick faces with device-scope atomic min, and every later pass is a plain stream.  No workgroup waits for another one; every loop walks
// strictly falling indices or has a fixed trip count.  The root of a finished component is its smallest raster index, whatever order
// the unions arrived in, and sizes are integer sums, so the results are canonical: runs repeat bitwise.  Plain HIP, integer atomics only.
// The window and volume checks are dm3d_volume.h's.
#include "dm3d_volume.h"
#include <math.h>

namespace {

constexpr int BD = 8, BH = 8, BW = 64;             // the brick of the local pass: rows of 64 along w, one per wave and round
constexpr int BV = BD * BH * BW;                   // 4096 voxels, 16 per lane; lab and sz take 32 KiB of LDS
constexpr int VOX = DM3D_CCL_BLOCK_VOXELS;         // voxels a block of the streaming kernels walks (4 per lane, consecutive per lane)
constexpr int SIZE_MASK = 0x0fffffff;              // a size word: the voxel count (at most 2^27) ...
constexpr int FACE_FLAG = 0x40000000;              // ... and whether the component touches a face of the volume

// Parents in LDS, shared by the waves of one workgroup, and parents in memory, shared by every workgroup of a launch: relaxed atomic
// accesses at that scope, so no read is served from a register or from a stale L1 line.
struct LdsParents {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
    __device__ __forceinline__ int fetch_min(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
};
struct DeviceParents {
    int* p;
    __device__ __forceinline__ int load(int i) const { return __hip_atomic_load(p + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    __device__ __forceinline__ int fetch_min(int i, int v) const { return __hip_atomic_fetch_min(p + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
};
struct PlainParents {                              // a launch nobody writes parents in
    const int* p;
    __device__ __forceinline__ int load(int i) const { return p[i]; }
};

// The root of i.  A parent is never above its child, so the walk falls strictly; anything else (a parent above, the background sentinel)
// ends it at once.  A value read late is an older ancestor, still in i's tree.
template <class M>
__device__ __forceinline__ int ccl_find(const M& m, int i) {
    for (;;) {
        const int q = m.load(i);
        if ((unsigned)q >= (unsigned)i) return i;
        i = q;
    }
}

// Unites the trees of a and b: the larger root is attached to the smaller one by an atomic min on the larger root's own slot.  If that
// slot was no root any more (old != a), a's tree hangs under min(old, b) now and old and b remain to be united.  a + b falls in
// every round, so the loop ends.
template <class M>
__device__ __forceinline__ void ccl_unite(const M& m, int a, int b) {
    for (;;) {
        a = ccl_find(m, a);
        b = ccl_find(m, b);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = m.fetch_min(a, b);
        if ((unsigned)old >= (unsigned)a) return;
        a = old;
    }
}

// Whether (dz, dy, dx) is one of the neighbours of a K-axis connectivity (6, 18, 26 for K = 1, 2, 3) that lies before the voxel in
// raster order: each pair of neighbours is united once, from its later voxel.
template <int K>
__device__ __forceinline__ constexpr bool ccl_backward(int dz, int dy, int dx) {
    const int axes = (dz != 0) + (dy != 0) + (dx != 0);
    return axes >= 1 && axes <= K && (dz < 0 || (dz == 0 && (dy < 0 || (dy == 0 && dx < 0))));
}

struct CclArgs {
    const float* x;
    int* parent; int* size;                        // [batch * nc][d][h][w]
    int d, h, w, cx, x0c, nc;
    int nbx, nby;                                  // bricks along w and h
    float thr;
    int complement;                                // label the background (fill_holes)
};

// Grid (bricks of a volume, batch * nc).  parent[v] = raster index of the smallest voxel of v's component inside the brick, -1 at the
// background; size[v] = voxels (and the face flag) of that piece at its smallest voxel, 0 elsewhere.  Local and raster order agree
// (both are lexicographic in z, y, x), so the local root is also the smallest raster index of the piece.
template <int K>
__global__ __launch_bounds__(256) void ccl_local_kernel(const CclArgs p) {
    __shared__ int lab[BV];
    __shared__ int sz[BV];
    const LdsParents m{lab};
    const int bc = blockIdx.y, b = bc / p.nc, c = bc % p.nc;
    const int x0 = (int)(blockIdx.x % p.nbx) * BW, y0 = (int)((blockIdx.x / p.nbx) % p.nby) * BH, z0 = (int)(blockIdx.x / (p.nbx * p.nby)) * BD;
    const long vol = (long)p.d * p.h * p.w;
    const float* xs = p.x + b * vol * p.cx + p.x0c + c;
    const int lx = threadIdx.x & 63, r0 = threadIdx.x >> 6;
    const int x = x0 + lx;
#pragma unroll
    for (int k = 0; k < BV / 256; ++k) {
        const int row = k * 4 + r0, ly = row & 7, lz = row >> 3, l = row * BW + lx;
        const int y = y0 + ly, z = z0 + lz;
        bool fg = false;
        if (z < p.d && y < p.h && x < p.w) {
            fg = xs[(((long)z * p.h + y) * p.w + x) * p.cx] > p.thr;
            fg = p.complement ? !fg : fg;
        }
        lab[l] = fg ? l : -1;
        sz[l] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BV / 256; ++k) {
        const int row = k * 4 + r0, ly = row & 7, lz = row >> 3, l = row * BW + lx;
        if (m.load(l) < 0) continue;
#pragma unroll
        for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    if (!ccl_backward<K>(dz, dy, dx)) continue;
                    if ((unsigned)(lz + dz) >= (unsigned)BD || (unsigned)(ly + dy) >= (unsigned)BH || (unsigned)(lx + dx) >= (unsigned)BW) continue;
                    const int n = l + (dz * BH + dy) * BW + dx;
                    if (m.load(n) >= 0) ccl_unite(m, l, n);
                }
    }
    __syncthreads();
    int root[BV / 256];
#pragma unroll
    for (int k = 0; k < BV / 256; ++k) {
        const int row = k * 4 + r0, ly = row & 7, lz = row >> 3, l = row * BW + lx;
        const int y = y0 + ly, z = z0 + lz;
        const int r = lab[l] < 0 ? -1 : ccl_find(m, l);
        root[k] = r;
        const bool face = z == 0 || y == 0 || x == 0 || z == p.d - 1 || y == p.h - 1 || x == p.w - 1;
        // a wave holds one row: up to four roots shared by its lanes are added once per wave
        bool live = r >= 0;
        for (int round = 0; round < 4; ++round) {
            const unsigned long long act = __ballot(live);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const int rl = __shfl(r, leader, 64);
            const unsigned long long same = __ballot(live && r == rl), faces = __ballot(live && r == rl && face);
            if (lx == leader) {
                atomicAdd(&sz[rl], __popcll(same));
                if (faces) atomicOr(&sz[rl], FACE_FLAG);
            }
            if (r == rl) live = false;
        }
        if (live) {
            atomicAdd(&sz[r], 1);
            if (face) atomicOr(&sz[r], FACE_FLAG);
        }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < BV / 256; ++k) {
        const int row = k * 4 + r0, ly = row & 7, lz = row >> 3, l = row * BW + lx;
        const int y = y0 + ly, z = z0 + lz;
        if (z >= p.d || y >= p.h || x >= p.w) continue;
        const long v = bc * vol + ((long)z * p.h + y) * p.w + x;
        const int r = root[k];
        p.parent[v] = r < 0 ? -1 : ((z0 + (r >> 9)) * p.h + y0 + ((r >> 6) & 7)) * p.w + x0 + (r & 63);
        p.size[v] = r == l ? sz[l] : 0;
    }
}

// Grid (ceil(dhw / 256), batch * nc), a lane per voxel: a voxel on a brick face unites with its backward neighbours in other bricks.
template <int K>
__global__ __launch_bounds__(256) void ccl_seam_kernel(int* parent, int d, int h, int w) {
    const long vol = (long)d * h * w;
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= vol) return;
    const int x = (int)(v % w), y = (int)((v / w) % h), z = (int)(v / ((long)w * h));
    const int lx = x & (BW - 1), ly = y & (BH - 1), lz = z & (BD - 1);
    if (lx != 0 && lx != BW - 1 && ly != 0 && ly != BH - 1 && lz != 0) return;    // no backward neighbour leaves the brick (dz is never +1)
    const DeviceParents m{parent + blockIdx.y * vol};
    if (m.load((int)v) < 0) return;
#pragma unroll
    for (int dz = -1; dz <= 0; ++dz)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                if (!ccl_backward<K>(dz, dy, dx)) continue;
                const int nz = z + dz, ny = y + dy, nx = x + dx;
                if ((unsigned)nz >= (unsigned)d || (unsigned)ny >= (unsigned)h || (unsigned)nx >= (unsigned)w) continue;
                if (nz / BD == z / BD && ny / BH == y / BH && nx / BW == x / BW) continue;
                const int n = (nz * h + ny) * w + nx;
                if (m.load(n) >= 0) ccl_unite(m, (int)v, n);
            }
}

// Grid (ceil(dhw / 256), batch * nc): root[v] = the root of v, -1 at the background (parents are only read here); the smallest voxel
// of every brick piece that is not the root adds its piece's size and face flag to the root's slot.
__global__ __launch_bounds__(256) void ccl_flatten_kernel(const int* parent, int* size, int* root, long vol) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= vol) return;
    const long base = blockIdx.y * vol;
    const PlainParents m{parent + base};
    const int q = m.load((int)v);
    const int r = q < 0 ? -1 : ccl_find(m, q);
    root[base + v] = r;
    if (r < 0 || r == (int)v) return;
    const int s = size[base + v];                                               // v is no root: nobody adds to its slot
    if (s == 0) return;
    atomicAdd(&size[base + r], s & SIZE_MASK);
    if (s & FACE_FLAG) atomicOr(&size[base + r], FACE_FLAG);
}

// key of a root: its size above, INT32_MAX - index below, so the largest key is the largest component with the smallest root
__device__ __forceinline__ unsigned long long ccl_key(int size, int index) {
    return ((unsigned long long)(unsigned)(size & SIZE_MASK) << 32) | (unsigned)(0x7fffffff - index);
}

// Grid (ceil(dhw / VOX), batch * nc): the roots of a block's VOX voxels, counted, and the largest key among them.
__global__ __launch_bounds__(256) void ccl_count_kernel(const int* root, const int* size, int* block_count, unsigned long long* block_key, long vol) {
    __shared__ int cs[4];
    __shared__ unsigned long long ks[4];
    const long base = blockIdx.y * vol, v0 = (long)blockIdx.x * VOX + threadIdx.x * 4;
    int n = 0;
    unsigned long long key = 0ull;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long v = v0 + j;
        if (v < vol && root[base + v] == (int)v) {
            ++n;
            const unsigned long long kv = ccl_key(size[base + v], (int)v);
            key = kv > key ? kv : key;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        n += __shfl_xor(n, off, 64);
        const unsigned long long o = __shfl_xor(key, off, 64);
        key = o > key ? o : key;
    }
    if ((threadIdx.x & 63) == 0) { cs[threadIdx.x >> 6] = n; ks[threadIdx.x >> 6] = key; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const long slot = (long)blockIdx.y * gridDim.x + blockIdx.x;
        unsigned long long kk = ks[0];
        for (int i = 1; i < 4; ++i) kk = ks[i] > kk ? ks[i] : kk;
        block_count[slot] = cs[0] + cs[1] + cs[2] + cs[3];
        block_key[slot] = kk;
    }
}

// Block per (volume, channel): the block counts become their exclusive prefix sums in place; count[bc] (optional) and best[bc] leave.
// Lane t owns a run of ceil(nblk / 256) blocks; lane 0 scans the 256 run totals: fixed trip counts throughout.
__global__ __launch_bounds__(256) void ccl_scan_kernel(int* block_count, const unsigned long long* block_key, int nblk, int* count, unsigned long long* best) {
    __shared__ int tot[256];
    __shared__ unsigned long long ks[256];
    const int bc = blockIdx.x, t = threadIdx.x;
    int* cnt = block_count + (long)bc * nblk;
    const unsigned long long* keys = block_key + (long)bc * nblk;
    const int run = (nblk + 255) / 256, lo = min(t * run, nblk), hi = min(lo + run, nblk);
    int s = 0;
    unsigned long long key = 0ull;
    for (int i = lo; i < hi; ++i) {
        s += cnt[i];
        key = keys[i] > key ? keys[i] : key;
    }
    tot[t] = s; ks[t] = key;
    __syncthreads();
    if (t == 0) {
        int acc = 0;
        unsigned long long kk = 0ull;
        for (int i = 0; i < 256; ++i) {
            const int ti = tot[i];
            tot[i] = acc;
            acc += ti;
            kk = ks[i] > kk ? ks[i] : kk;
        }
        if (count) count[bc] = acc;
        best[bc] = kk;
    }
    __syncthreads();
    int acc = tot[t];
    for (int i = lo; i < hi; ++i) {
        const int ci = cnt[i];
        cnt[i] = acc;
        acc += ci;
    }
}

// Grid (ceil(dhw / VOX), batch * nc): rank[root] = 1 + the number of roots before it in raster order (a lane holds 4 consecutive voxels).
__global__ __launch_bounds__(256) void ccl_rank_kernel(const int* root, const int* block_offset, int* rank, long vol) {
    __shared__ int ws[4];
    const long base = blockIdx.y * vol, v0 = (long)blockIdx.x * VOX + threadIdx.x * 4;
    bool is[4];
    int n = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const long v = v0 + j;
        is[j] = v < vol && root[base + v] == (int)v;
        n += is[j];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    if (lane == 63) ws[wave] = inc;
    __syncthreads();
    int before = block_offset[(long)blockIdx.y * gridDim.x + blockIdx.x] + inc - n;
    for (int i = 0; i < wave; ++i) before += ws[i];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (is[j]) rank[base + v0 + j] = ++before;
}

// Grid (ceil(dhw / 256), batch * nc): labels[v] (the root on entry) = rank[root], 0 at the background; largest[bc] = (label, size).
__global__ __launch_bounds__(256) void ccl_label_kernel(int* labels, const int* rank, const unsigned long long* best, long long* largest, long vol) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    const long base = blockIdx.y * vol;
    if (v == 0) {
        const unsigned long long key = best[blockIdx.y];
        const int size = (int)(key >> 32), index = 0x7fffffff - (int)(unsigned)(key & 0xffffffffu);
        largest[2 * blockIdx.y] = size ? rank[base + index] : 0;
        largest[2 * blockIdx.y + 1] = size;
    }
    if (v >= vol) return;
    const int r = labels[base + v];
    labels[base + v] = r < 0 ? 0 : rank[base + r];
}

// Grid (ceil(dhw / 256), batch * nc): the float32 NDHWC mask of a filter mode.  fill_holes labelled the background: a voxel stays out
// only where its background component touches a face.
__global__ __launch_bounds__(256) void ccl_filter_kernel(const int* root, const int* size, const unsigned long long* best, float* out, long vol, int nc, int mode,
                                                         int min_size) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= vol) return;
    const int bc = blockIdx.y, b = bc / nc, c = bc % nc;
    const long base = bc * vol;
    const int r = root[base + v];
    bool keep;
    if (mode == DM3D_CCL_FILL_HOLES) {
        keep = r < 0 || !(size[base + r] & FACE_FLAG);
    } else if (mode == DM3D_CCL_MIN_SIZE) {
        keep = r >= 0 && (size[base + r] & SIZE_MASK) >= min_size;
    } else {
        const unsigned long long key = best[bc];
        keep = r >= 0 && (key >> 32) != 0 && r == 0x7fffffff - (int)(unsigned)(key & 0xffffffffu);
    }
    out[(b * vol + v) * nc + c] = keep ? 1.0f : 0.0f;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
struct Plan {
    int64_t bc, vol, V, nblk;
    int *parent, *size, *root, *block_count;
    unsigned long long *block_key, *best;
};

int64_t small_words(int64_t bc, int64_t nblk) { return bc * (3 * nblk + 2); }

int check_common(const dm3d_ccl_desc* d, const char* who) {
    DM3D_REQUIRE(d != nullptr, "%s: null descriptor", who);
    DM3D_REQUIRE(d->x != nullptr, "%s: x must be non-null", who);
    DM3D_REQUIRE(dm3d_aligned(d->x, 4), "%s: x must be 4-byte aligned", who);
    int rc = dm3d_check_volume(who, d->batch, d->d, d->h, d->w, d->nc, DM3D_CCL_MAX_EXTENT, "DM3D_CCL_MAX_EXTENT");
    if (rc != DM3D_OK || (rc = dm3d_check_window(who, "x", d->x0c, d->nc, d->cx)) != DM3D_OK) return rc;
    DM3D_REQUIRE(isfinite(d->threshold), "%s: threshold=%g (finite)", who, (double)d->threshold);
    DM3D_REQUIRE(d->connectivity == 6 || d->connectivity == 18 || d->connectivity == 26, "%s: connectivity=%d (6, 18 or 26)", who, d->connectivity);
    DM3D_REQUIRE(d->work != nullptr, "%s: work must be non-null", who);
    DM3D_REQUIRE(dm3d_aligned(d->work, 8), "%s: work must be 8-byte aligned", who);
    return DM3D_OK;
}

// The scratch of an entry that keeps `planes` int32 planes of the voxel count: checked, then laid out.
int make_plan(const dm3d_ccl_desc* d, const char* who, int planes, int* third, Plan* pl) {
    pl->bc = (int64_t)d->batch * d->nc;
    pl->vol = (int64_t)d->d * d->h * d->w;
    pl->V = pl->bc * pl->vol;
    pl->nblk = (pl->vol + VOX - 1) / VOX;
    const int64_t need = planes * pl->V + 1 + small_words(pl->bc, pl->nblk);
    DM3D_REQUIRE(d->work_elems >= need, "%s: work holds %lld int32, %lld are needed (%d * batch * nc * d * h * w + 1 + batch * nc * (3 * %lld + 2))", who,
                 (long long)d->work_elems, (long long)need, planes, (long long)pl->nblk);
    pl->parent = d->work;
    pl->size = d->work + pl->V;
    pl->root = third ? third : d->work + 2 * pl->V;
    int64_t at = (int64_t)planes * pl->V;
    at += at & 1;                                                               // the 64-bit keys sit on 8 bytes
    pl->block_key = reinterpret_cast<unsigned long long*>(d->work + at);
    pl->best = pl->block_key + pl->bc * pl->nblk;
    pl->block_count = d->work + at + 2 * pl->bc * pl->nblk + 2 * pl->bc;
    return DM3D_OK;
}

template <int K>
int launch_unions(const CclArgs& a, const Plan& pl, hipStream_t st) {
    const dim3 bricks((unsigned)(a.nbx * a.nby * ((a.d + BD - 1) / BD)), (unsigned)pl.bc);
    hipLaunchKernelGGL(ccl_local_kernel<K>, bricks, dim3(256), 0, st, a);
    int rc = dm3d_launch_check("ccl_local_kernel");
    if (rc != DM3D_OK) return rc;
    hipLaunchKernelGGL(ccl_seam_kernel<K>, dim3((unsigned)((pl.vol + 255) / 256), (unsigned)pl.bc), dim3(256), 0, st, a.parent, a.d, a.h, a.w);
    return dm3d_launch_check("ccl_seam_kernel");
}

// Labels the mask (or, complemented, its background) up to the roots: parent, size and root are final; with `reduce` also the block
// counts (scanned), count (optional) and best.
int launch_roots(const dm3d_ccl_desc* d, const Plan& pl, int connectivity, int complement, bool reduce, int* count, hipStream_t st) {
    CclArgs a{};
    a.x = d->x; a.parent = pl.parent; a.size = pl.size;
    a.d = d->d; a.h = d->h; a.w = d->w; a.cx = d->cx; a.x0c = d->x0c; a.nc = d->nc;
    a.nbx = (d->w + BW - 1) / BW; a.nby = (d->h + BH - 1) / BH;
    a.thr = d->threshold; a.complement = complement;
    int rc = connectivity == 6 ? launch_unions<1>(a, pl, st) : connectivity == 18 ? launch_unions<2>(a, pl, st) : launch_unions<3>(a, pl, st);
    if (rc != DM3D_OK) return rc;
    const dim3 per_voxel((unsigned)((pl.vol + 255) / 256), (unsigned)pl.bc), per_block((unsigned)pl.nblk, (unsigned)pl.bc);
    hipLaunchKernelGGL(ccl_flatten_kernel, per_voxel, dim3(256), 0, st, pl.parent, pl.size, pl.root, (long)pl.vol);
    if ((rc = dm3d_launch_check("ccl_flatten_kernel")) != DM3D_OK || !reduce) return rc;
    hipLaunchKernelGGL(ccl_count_kernel, per_block, dim3(256), 0, st, pl.root, pl.size, pl.block_count, pl.block_key, (long)pl.vol);
    if ((rc = dm3d_launch_check("ccl_count_kernel")) != DM3D_OK) return rc;
    hipLaunchKernelGGL(ccl_scan_kernel, dim3((unsigned)pl.bc), dim3(256), 0, st, pl.block_count, pl.block_key, (int)pl.nblk, count, pl.best);
    return dm3d_launch_check("ccl_scan_kernel");
}

}  // namespace

extern "C" int dm3d_components(const dm3d_ccl_desc* d, void* stream) {
    int rc = check_common(d, "components");
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->labels != nullptr && d->count != nullptr && d->largest != nullptr, "components: labels, count and largest must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->labels, 4) && dm3d_aligned(d->count, 4),
                 "components: labels and count must be 4-byte aligned");
    DM3D_REQUIRE(dm3d_aligned(d->largest, 8), "components: largest must be 8-byte aligned");
    Plan pl{};
    if ((rc = make_plan(d, "components", 2, d->labels, &pl)) != DM3D_OK) return rc;
    DM3D_REQUIRE(!dm3d_ranges_overlap(d->labels, (uint64_t)pl.V * 4, d->x, (uint64_t)d->batch * pl.vol * d->cx * 4), "components: labels overlaps x");
    hipStream_t st = static_cast<hipStream_t>(stream);
    if ((rc = launch_roots(d, pl, d->connectivity, 0, true, d->count, st)) != DM3D_OK) return rc;
    hipLaunchKernelGGL(ccl_rank_kernel, dim3((unsigned)pl.nblk, (unsigned)pl.bc), dim3(256), 0, st, pl.root, pl.block_count, pl.parent, (long)pl.vol);
    if ((rc = dm3d_launch_check("ccl_rank_kernel")) != DM3D_OK) return rc;
    hipLaunchKernelGGL(ccl_label_kernel, dim3((unsigned)((pl.vol + 255) / 256), (unsigned)pl.bc), dim3(256), 0, st, d->labels, pl.parent, pl.best,
                       reinterpret_cast<long long*>(d->largest), (long)pl.vol);
    return dm3d_launch_check("ccl_label_kernel");
}

extern "C" int dm3d_component_filter(const dm3d_ccl_desc* d, void* stream) {
    int rc = check_common(d, "component_filter");
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->mode == DM3D_CCL_LARGEST || d->mode == DM3D_CCL_MIN_SIZE || d->mode == DM3D_CCL_FILL_HOLES,
                 "component_filter: mode=%d (DM3D_CCL_LARGEST, DM3D_CCL_MIN_SIZE or DM3D_CCL_FILL_HOLES)", d->mode);
    DM3D_REQUIRE(d->mode != DM3D_CCL_MIN_SIZE || d->min_size >= 1, "component_filter: min_size=%d (at least 1)", d->min_size);
    DM3D_REQUIRE(d->out != nullptr, "component_filter: out must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->out, 4), "component_filter: out must be 4-byte aligned");
    Plan pl{};
    if ((rc = make_plan(d, "component_filter", 3, nullptr, &pl)) != DM3D_OK) return rc;
    DM3D_REQUIRE(!dm3d_ranges_overlap(d->out, (uint64_t)pl.V * 4, d->x, (uint64_t)d->batch * pl.vol * d->cx * 4), "component_filter: out overlaps x");
    hipStream_t st = static_cast<hipStream_t>(stream);
    const bool fill = d->mode == DM3D_CCL_FILL_HOLES;
    if ((rc = launch_roots(d, pl, fill ? 6 : d->connectivity, fill, d->mode == DM3D_CCL_LARGEST, nullptr, st)) != DM3D_OK) return rc;
    hipLaunchKernelGGL(ccl_filter_kernel, dim3((unsigned)((pl.vol + 255) / 256), (unsigned)pl.bc), dim3(256), 0, st, pl.root, pl.size, pl.best, d->out,
                       (long)pl.vol, d->nc, d->mode, d->min_size);
    return dm3d_launch_check("ccl_filter_kernel");
}
