// dm3d_dist.hip — the all-pairs passes of the distribution metrics (include/dm3d.h, dm3d_dist_desc): feature moments for the Frechet
// distance, k-th-neighbour radii and the precision / recall / density / coverage counts, and the cubic-kernel sums of KID.
//
// One tiled kernel serves all four: a workgroup of 256 lanes owns T = 64 rows and walks the columns in tiles of 64; both tiles are staged
// in LDS one chunk of 32 contraction indices at a time, and a lane keeps 4 x 4 pairs in registers and runs the contraction over them in
// index order, so every pair's sum is the sequential float64 sum the header promises (multiply and add rounded separately).  A finished
// 64 x 64 tile of values is laid over the staging buffer, and one lane per row (one per column for the density counts) folds it into
// what the row keeps across column tiles: its k + 1 smallest, its minimum and flags, its running sum.  No n x m matrix reaches memory, no
// workgroup waits for another one, and the only atomics add integers.  Plain HIP, float64 on the vector ALU.
#include "dm3d_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int T = DM3D_DIST_TILE;                  // rows and columns of a tile
constexpr int DC = DM3D_DIST_CHUNK;                // contraction indices staged at a time
constexpr int LD = DC + 1;                         // leading dimension of a staged tile: odd, so a column of rows spreads over the banks
constexpr int TL = T + 1;                          // leading dimension of the value tile, stored column-major: val[c * TL + r]
constexpr int K1 = DM3D_DIST_MAX_K + 1;            // the longest list a row keeps
static_assert(2 * T * LD >= T * TL, "the value tile lies over the two staged tiles");

enum { OP_KNN = 0, OP_PRDC = 1, OP_MMD = 2, OP_COV = 3 };

struct DistArgs {
    const double *x, *y;                           // row matrix and column matrix (the same for knn, the within sums and cov)
    const int *rows_x, *rows_y;                    // tables of this launch, or null
    int n, m, nx, ny, dim, k;
    const double *radius_x, *radius_y, *mean;
    double* out;                                   // knn: radius [n]; mmd: row sums [subsets][n | m | n]; cov: [dim, dim]
    int *count_y, *near_x, *cover_x;
};

// Matrix row of position p: the table's entry clamped into the matrix, or p.
__device__ __forceinline__ int dist_row(const int* table, int p, int rows) {
    int r = table ? table[p] : p;
    r = r < 0 ? 0 : r;
    return r >= rows ? rows - 1 : r;
}

// Stages tile[r][f] = mat[row(r)][f0 + f] for f < flen, r < T; rows past the set (ridx < 0) and the tail of the chunk hold 0.
__device__ __forceinline__ void stage_rows(double* tile, const double* mat, const int* ridx, int dim, int f0, int flen) {
    const int f = threadIdx.x & (DC - 1);
    for (int r = threadIdx.x / DC; r < T; r += 256 / DC) {
        const int row = ridx[r];
        tile[r * LD + f] = (row >= 0 && f < flen) ? mat[(size_t)row * dim + f0 + f] : 0.0;
    }
}

// Covariance: the "rows" of the tile are features i0 .. i0 + T - 1 and the contraction runs over set positions p0 .. p0 + plen - 1:
// tile[i][p] = x[row(p0 + p)][i0 + i] - mean[i0 + i].
__device__ __forceinline__ void stage_centered(double* tile, const DistArgs& a, int i0, int p0, int plen) {
    const int i = threadIdx.x & (T - 1);
    const bool live = i0 + i < a.dim;
    const double mu = live ? a.mean[i0 + i] : 0.0;
    for (int p = threadIdx.x / T; p < DC; p += 256 / T) {
        double v = 0.0;
        if (live && p < plen) v = a.x[(size_t)dist_row(a.rows_x, p0 + p, a.nx) * a.dim + i0 + i] - mu;
        tile[i * LD + p] = v;
    }
}

template <int OP>
__global__ __launch_bounds__(256) void dist_tile_kernel(DistArgs a) {
    bool skip_diagonal = false;
    if (OP == OP_MMD) {                            // blockIdx.y = 3 * subset + {x with x, y with y, x with y}: the launch's sets become this sum's
        const int s = blockIdx.y / 3, w = blockIdx.y - 3 * s;
        const int* tx = a.rows_x ? a.rows_x + (size_t)s * a.n : nullptr;
        const int* ty = a.rows_y ? a.rows_y + (size_t)s * a.m : nullptr;
        a.out += (size_t)s * (2 * a.n + a.m) + (w == 0 ? 0 : w == 1 ? a.n : a.n + a.m);
        a.rows_x = tx; a.rows_y = ty;
        if (w == 0) { a.y = a.x; a.rows_y = tx; a.m = a.n; a.ny = a.nx; }
        if (w == 1) { a.x = a.y; a.rows_x = ty; a.n = a.m; a.nx = a.ny; }
        skip_diagonal = w < 2;
    }
    __shared__ double stage[2 * T * LD];           // xs | ys while a chunk is contracted, then the 64 x 64 values of the tile
    __shared__ double best[OP == OP_KNN ? T * K1 : 1];
    __shared__ double rad_x[OP == OP_PRDC ? T : 1], rad_y[OP == OP_PRDC ? T : 1];
    __shared__ int rix[T], riy[T];
    double* xs = stage;
    double* ys = stage + T * LD;
    double* val = stage;

    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const int row0 = blockIdx.x * T;
    const int nrows = OP == OP_COV ? a.dim : a.n;  // what the tile's rows and columns count
    const int ncols = OP == OP_COV ? a.dim : a.m;
    const int depth = OP == OP_COV ? a.n : a.dim;  // the contraction length
    if (row0 >= nrows) return;                     // mmd launches max(n, m) rows' worth of blocks for all three sums

    if (OP != OP_COV && tid < T) rix[tid] = row0 + tid < a.n ? dist_row(a.rows_x, row0 + tid, a.nx) : -1;
    if (OP == OP_KNN) {
        for (int i = tid; i < T * K1; i += 256) best[i] = INFINITY;
    }
    if (OP == OP_PRDC && tid < T) rad_x[tid] = row0 + tid < a.n ? a.radius_x[row0 + tid] : 0.0;
    double row_min = INFINITY, row_sum = 0.0;      // lane r < T: what row r keeps
    int row_near = 0;

    // cov: only the tiles on and above the diagonal; everything else: every column tile
    const int first = OP == OP_COV ? blockIdx.x : 0;
    const int tiles = (ncols + T - 1) / T;
    for (int ct = first; ct < tiles; ++ct) {
        const int col0 = ct * T;
        __syncthreads();                           // the previous tile's values are folded
        if (OP != OP_COV && tid < T) riy[tid] = col0 + tid < a.m ? dist_row(a.rows_y, col0 + tid, a.ny) : -1;
        if (OP == OP_PRDC && tid >= T && tid < 2 * T) rad_y[tid - T] = col0 + tid - T < a.m ? a.radius_y[col0 + tid - T] : 0.0;
        double acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0.0;

        for (int f0 = 0; f0 < depth; f0 += DC) {
            const int flen = depth - f0 < DC ? depth - f0 : DC;
            __syncthreads();                       // the previous chunk is contracted (first round: rix, riy are written)
            if (OP == OP_COV) {
                stage_centered(xs, a, row0, f0, flen);
                stage_centered(ys, a, col0, f0, flen);
            } else {
                stage_rows(xs, a.x, rix, a.dim, f0, flen);
                stage_rows(ys, a.y, riy, a.dim, f0, flen);
            }
            __syncthreads();
#pragma unroll 4
            for (int f = 0; f < flen; ++f) {       // in index order: this loop is the sequential sum
                double u[4], v[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) u[i] = xs[(ty + 16 * i) * LD + f];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = ys[(tx + 16 * j) * LD + f];
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (OP == OP_KNN || OP == OP_PRDC) {
                            const double t = u[i] - v[j];
                            const double q = t * t;
                            acc[i][j] = acc[i][j] + q;
                        } else {
                            const double q = u[i] * v[j];
                            acc[i][j] = acc[i][j] + q;
                        }
                    }
            }
        }

        if (OP == OP_COV) {                        // the triangle i <= j, mirrored
            const double denom = (double)(a.n - 1);
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int gi = row0 + ty + 16 * i, gj = col0 + tx + 16 * j;
                    if (gi < a.dim && gj < a.dim && gi <= gj) {
                        const double c = acc[i][j] / denom;
                        a.out[(size_t)gi * a.dim + gj] = c;
                        a.out[(size_t)gj * a.dim + gi] = c;
                    }
                }
            continue;
        }

        __syncthreads();                           // the last chunk is contracted: the staging buffer becomes the value tile
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                double v = acc[i][j];
                if (OP == OP_MMD) {
                    const double t = v / (double)a.dim + 1.0;
                    const double t2 = t * t;
                    v = t2 * t;
                }
                val[(tx + 16 * j) * TL + ty + 16 * i] = v;
            }
        __syncthreads();
        const int clen = a.m - col0 < T ? a.m - col0 : T;
        if (tid < T && row0 + tid < a.n) {         // one lane per row, the columns in index order
            const int r = tid;
            if (OP == OP_KNN) {
                double* list = best + r * K1;      // ascending; list[k] is the (k + 1)-th smallest so far
                for (int c = 0; c < clen; ++c) {
                    const double v = val[c * TL + r];
                    if (v < list[a.k]) {
                        int p = a.k;
                        while (p > 0 && list[p - 1] > v) { list[p] = list[p - 1]; --p; }
                        list[p] = v;
                    }
                }
            } else if (OP == OP_PRDC) {
                for (int c = 0; c < clen; ++c) {
                    const double v = val[c * TL + r];
                    row_min = v < row_min ? v : row_min;
                    row_near |= v < rad_y[c] ? 1 : 0;
                }
            } else {
                for (int c = 0; c < clen; ++c) {
                    if (skip_diagonal && row0 + r == col0 + c) continue;
                    row_sum = row_sum + val[c * TL + r];
                }
            }
        }
        if (OP == OP_PRDC && tid >= T && tid < T + clen) {   // one lane per column: how many rows of this block hold it inside their ball
            const int c = tid - T;
            const int rlen = a.n - row0 < T ? a.n - row0 : T;
            int cnt = 0;
            for (int r = 0; r < rlen; ++r) cnt += val[c * TL + r] < rad_x[r] ? 1 : 0;
            if (cnt) atomicAdd(a.count_y + col0 + c, cnt);
        }
    }

    if (OP == OP_COV) return;
    if (tid < T && row0 + tid < a.n) {
        if (OP == OP_KNN) a.out[row0 + tid] = best[tid * K1 + a.k];
        if (OP == OP_MMD) a.out[row0 + tid] = row_sum;
        if (OP == OP_PRDC) {
            a.near_x[row0 + tid] = row_near;
            a.cover_x[row0 + tid] = row_min < rad_x[tid] ? 1 : 0;
        }
    }
}

// mean[f] = (x[0][f] + x[1][f] + ..) / n, the rows in order; a lane per feature.
__global__ __launch_bounds__(256) void dist_mean_kernel(const double* x, const int* rows, int n, int nx, int dim, double* mean) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    if (f >= dim) return;
    double s = 0.0;
#pragma unroll 8
    for (int p = 0; p < n; ++p) s = s + x[(size_t)dist_row(rows, p, nx) * dim + f];
    mean[f] = s / (double)n;
}

// sums[s][w] = rowsum[0] + rowsum[1] + .., in order; a lane per (subset, sum).  The row sums of subset s lie as [x: n | y: m | xy: n].
__global__ __launch_bounds__(64) void dist_total_kernel(const double* rowsums, int subsets, int n, int m, double* sums) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= subsets * 3) return;
    const int s = i / 3, w = i - 3 * s;
    const double* r = rowsums + (size_t)s * (2 * n + m) + (w == 0 ? 0 : w == 1 ? n : n + m);
    const int len = w == 1 ? m : n;
    double t = 0.0;
#pragma unroll 8
    for (int p = 0; p < len; ++p) t = t + r[p];
    sums[i] = t;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------
bool aligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// What every entry checks of the row matrix; `two` also of the column matrix.
int check_common(const dm3d_dist_desc* d, const char* who, bool two, int min_m) {
    DM3D_REQUIRE(d != nullptr, "%s: null descriptor", who);
    DM3D_REQUIRE(d->x != nullptr, "%s: x must be non-null", who);
    DM3D_REQUIRE(aligned(d->x, 8), "%s: x must be 8-byte aligned", who);
    DM3D_REQUIRE(aligned(d->rows_x, 4), "%s: rows_x must be 4-byte aligned", who);
    DM3D_REQUIRE(d->dim >= 1, "%s: dim=%d (at least 1)", who, d->dim);
    DM3D_REQUIRE(d->dim <= DM3D_DIST_MAX_DIM, "%s: dim=%d exceeds DM3D_DIST_MAX_DIM=%d", who, d->dim, DM3D_DIST_MAX_DIM);
    DM3D_REQUIRE(d->n >= 2, "%s: n=%d (at least 2 rows)", who, d->n);
    DM3D_REQUIRE(d->nx >= 1, "%s: nx=%d (at least 1)", who, d->nx);
    DM3D_REQUIRE(d->n <= DM3D_DIST_MAX_ROWS && d->nx <= DM3D_DIST_MAX_ROWS, "%s: n=%d nx=%d exceeds DM3D_DIST_MAX_ROWS=%d", who, d->n, d->nx,
                 DM3D_DIST_MAX_ROWS);
    DM3D_REQUIRE(d->rows_x != nullptr || d->n <= d->nx, "%s: n=%d rows are read without a table, x holds nx=%d", who, d->n, d->nx);
    if (!two) return DM3D_OK;
    DM3D_REQUIRE(d->y != nullptr, "%s: y must be non-null", who);
    DM3D_REQUIRE(aligned(d->y, 8), "%s: y must be 8-byte aligned", who);
    DM3D_REQUIRE(aligned(d->rows_y, 4), "%s: rows_y must be 4-byte aligned", who);
    DM3D_REQUIRE(d->m >= min_m, "%s: m=%d (at least %d)", who, d->m, min_m);
    DM3D_REQUIRE(d->ny >= 1, "%s: ny=%d (at least 1)", who, d->ny);
    DM3D_REQUIRE(d->m <= DM3D_DIST_MAX_ROWS && d->ny <= DM3D_DIST_MAX_ROWS, "%s: m=%d ny=%d exceeds DM3D_DIST_MAX_ROWS=%d", who, d->m, d->ny,
                 DM3D_DIST_MAX_ROWS);
    DM3D_REQUIRE(d->rows_y != nullptr || d->m <= d->ny, "%s: m=%d rows are read without a table, y holds ny=%d", who, d->m, d->ny);
    return DM3D_OK;
}

// Whether an output of `bytes` bytes shares a byte with x (or, with `two`, y).
bool hits_input(const dm3d_dist_desc* d, bool two, const void* out, uint64_t bytes) {
    return dm3d_ranges_overlap(out, bytes, d->x, (uint64_t)d->nx * d->dim * 8) ||
           (two && dm3d_ranges_overlap(out, bytes, d->y, (uint64_t)d->ny * d->dim * 8));
}

DistArgs base_args(const dm3d_dist_desc* d) {
    DistArgs a{};
    a.x = d->x; a.rows_x = d->rows_x; a.n = d->n; a.nx = d->nx; a.dim = d->dim;
    return a;
}

unsigned tiles_of(int rows) { return (unsigned)((rows + T - 1) / T); }

}  // namespace

extern "C" int dm3d_feature_moments(const dm3d_dist_desc* d, void* stream) {
    int rc = check_common(d, "feature_moments", false, 0);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->mean != nullptr && d->cov != nullptr, "feature_moments: mean and cov must be non-null");
    DM3D_REQUIRE(aligned(d->mean, 8) && aligned(d->cov, 8), "feature_moments: mean and cov must be 8-byte aligned");
    const uint64_t mean_bytes = (uint64_t)d->dim * 8, cov_bytes = (uint64_t)d->dim * d->dim * 8;
    DM3D_REQUIRE(!hits_input(d, false, d->mean, mean_bytes), "feature_moments: mean overlaps x");
    DM3D_REQUIRE(!hits_input(d, false, d->cov, cov_bytes), "feature_moments: cov overlaps x");
    DM3D_REQUIRE(!dm3d_ranges_overlap(d->mean, mean_bytes, d->cov, cov_bytes), "feature_moments: mean overlaps cov");
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(dist_mean_kernel, dim3((unsigned)((d->dim + 255) / 256)), dim3(256), 0, st, d->x, d->rows_x, d->n, d->nx, d->dim, d->mean);
    if ((rc = dm3d_launch_check("dist_mean_kernel")) != DM3D_OK) return rc;
    DistArgs a = base_args(d);
    a.y = d->x; a.rows_y = d->rows_x; a.m = d->n; a.ny = d->nx;
    a.mean = d->mean; a.out = d->cov;
    hipLaunchKernelGGL(dist_tile_kernel<OP_COV>, dim3(tiles_of(d->dim)), dim3(256), 0, st, a);
    return dm3d_launch_check("dist_tile_kernel<cov>");
}

extern "C" int dm3d_knn_radius(const dm3d_dist_desc* d, void* stream) {
    int rc = check_common(d, "knn_radius", false, 0);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->k >= 1, "knn_radius: k=%d (at least 1)", d->k);
    DM3D_REQUIRE(d->k <= DM3D_DIST_MAX_K, "knn_radius: k=%d exceeds DM3D_DIST_MAX_K=%d", d->k, DM3D_DIST_MAX_K);
    DM3D_REQUIRE(d->k < d->n, "knn_radius: k=%d needs more than k rows, n=%d", d->k, d->n);
    DM3D_REQUIRE(d->radius != nullptr, "knn_radius: radius must be non-null");
    DM3D_REQUIRE(aligned(d->radius, 8), "knn_radius: radius must be 8-byte aligned");
    DM3D_REQUIRE(!hits_input(d, false, d->radius, (uint64_t)d->n * 8), "knn_radius: radius overlaps x");
    DistArgs a = base_args(d);
    a.y = d->x; a.rows_y = d->rows_x; a.m = d->n; a.ny = d->nx;
    a.k = d->k; a.out = d->radius;
    hipLaunchKernelGGL(dist_tile_kernel<OP_KNN>, dim3(tiles_of(d->n)), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check("dist_tile_kernel<knn>");
}

extern "C" int dm3d_prdc_counts(const dm3d_dist_desc* d, void* stream) {
    int rc = check_common(d, "prdc_counts", true, 1);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->radius_x != nullptr && d->radius_y != nullptr, "prdc_counts: radius_x and radius_y must be non-null");
    DM3D_REQUIRE(aligned(d->radius_x, 8) && aligned(d->radius_y, 8), "prdc_counts: radius_x and radius_y must be 8-byte aligned");
    DM3D_REQUIRE(d->count_y != nullptr && d->near_x != nullptr && d->cover_x != nullptr, "prdc_counts: count_y, near_x and cover_x must be non-null");
    DM3D_REQUIRE(aligned(d->count_y, 4) && aligned(d->near_x, 4) && aligned(d->cover_x, 4), "prdc_counts: count_y, near_x and cover_x must be 4-byte aligned");
    const struct { const void* p; uint64_t bytes; const char* name; } outs[3] = {
        {d->count_y, (uint64_t)d->m * 4, "count_y"}, {d->near_x, (uint64_t)d->n * 4, "near_x"}, {d->cover_x, (uint64_t)d->n * 4, "cover_x"}};
    for (const auto& o : outs) {
        DM3D_REQUIRE(!hits_input(d, true, o.p, o.bytes), "prdc_counts: %s overlaps x or y", o.name);
        DM3D_REQUIRE(!dm3d_ranges_overlap(o.p, o.bytes, d->radius_x, (uint64_t)d->n * 8) && !dm3d_ranges_overlap(o.p, o.bytes, d->radius_y, (uint64_t)d->m * 8),
                     "prdc_counts: %s overlaps a radius vector", o.name);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    DM3D_HIP(hipMemsetAsync(d->count_y, 0, (size_t)d->m * 4, st));
    DistArgs a = base_args(d);
    a.y = d->y; a.rows_y = d->rows_y; a.m = d->m; a.ny = d->ny;
    a.radius_x = d->radius_x; a.radius_y = d->radius_y;
    a.count_y = d->count_y; a.near_x = d->near_x; a.cover_x = d->cover_x;
    hipLaunchKernelGGL(dist_tile_kernel<OP_PRDC>, dim3(tiles_of(d->n)), dim3(256), 0, st, a);
    return dm3d_launch_check("dist_tile_kernel<prdc>");
}

extern "C" int dm3d_poly_mmd(const dm3d_dist_desc* d, void* stream) {
    int rc = check_common(d, "poly_mmd", true, 2);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->subsets >= 1, "poly_mmd: subsets=%d (at least 1)", d->subsets);
    DM3D_REQUIRE(d->subsets <= DM3D_DIST_MAX_SUBSETS, "poly_mmd: subsets=%d exceeds DM3D_DIST_MAX_SUBSETS=%d", d->subsets, DM3D_DIST_MAX_SUBSETS);
    DM3D_REQUIRE(d->sums != nullptr, "poly_mmd: sums must be non-null");
    DM3D_REQUIRE(aligned(d->sums, 8), "poly_mmd: sums must be 8-byte aligned");
    DM3D_REQUIRE(d->work != nullptr, "poly_mmd: work must be non-null");
    DM3D_REQUIRE(aligned(d->work, 8), "poly_mmd: work must be 8-byte aligned");
    const int64_t need = d->subsets * (2 * (int64_t)d->n + d->m);
    DM3D_REQUIRE(d->work_elems >= need, "poly_mmd: work holds %lld float64, %lld are needed (subsets * (2 * n + m))", (long long)d->work_elems,
                 (long long)need);
    DM3D_REQUIRE(!hits_input(d, true, d->sums, (uint64_t)d->subsets * 24), "poly_mmd: sums overlaps x or y");
    DM3D_REQUIRE(!hits_input(d, true, d->work, (uint64_t)need * 8), "poly_mmd: work overlaps x or y");
    DM3D_REQUIRE(!dm3d_ranges_overlap(d->sums, (uint64_t)d->subsets * 24, d->work, (uint64_t)need * 8), "poly_mmd: sums overlaps work");
    hipStream_t st = static_cast<hipStream_t>(stream);
    DistArgs a = base_args(d);
    a.y = d->y; a.rows_y = d->rows_y; a.m = d->m; a.ny = d->ny;
    a.out = d->work;
    hipLaunchKernelGGL(dist_tile_kernel<OP_MMD>, dim3(tiles_of(d->n > d->m ? d->n : d->m), (unsigned)(3 * d->subsets)), dim3(256), 0, st, a);
    if ((rc = dm3d_launch_check("dist_tile_kernel<mmd>")) != DM3D_OK) return rc;
    hipLaunchKernelGGL(dist_total_kernel, dim3((unsigned)((d->subsets * 3 + 63) / 64)), dim3(64), 0, st, d->work, d->subsets, d->n, d->m, d->sums);
    return dm3d_launch_check("dist_total_kernel");
}
