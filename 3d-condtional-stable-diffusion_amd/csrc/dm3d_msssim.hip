// dm3d_msssim.hip — 3-D multi-scale SSIM of pairs of volumes (include/dm3d.h, dm3d_ms_ssim_desc).  Per scale one fused pass: a
// workgroup owns TD x TH x TW points of the valid map of one (pair, channel) and walks the input planes along d; each plane of x and y
// is staged in LDS once, the w pass goes into LDS, the h pass into registers, and the d pass is a delay line of F accumulators per map
// and point in registers, so no filtered map ever reaches memory.  A pooling launch per tensor makes the next scale's volumes; a last
// launch combines tiles, scales, powers and channels.  Plain HIP: no MFMA, no atomics.  Every sum is float64 in a fixed order (a thread
// over its points in plane order, the block by dm3d_block_sum_f64, tiles in index order): runs repeat bitwise.
// The channel-window check is dm3d_volume.h's.
#include "dm3d_volume.h"
#include <math.h>

namespace {

constexpr int TD = DM3D_MSSSIM_TD, TH = DM3D_MSSSIM_TH, TW = DM3D_MSSSIM_TW;
constexpr int MAXF = 11, MAXS = 5;
constexpr int ROWS = TH * TW / 256;                                            // output rows of a plane per thread
static_assert(TW == 32 && ROWS * 256 == TH * TW, "a wave half walks one row of the tile");

struct ScaleArgs {
    const float* x; const float* y;                // this scale's tensors: the caller's, or the pooled ones (then cx = cy = nc, x0c = y0c = 0)
    const int* x_index; const int* y_index;
    int nx, ny, d, h, w, cx, cy, x0c, y0c;
    int tiles_h, tiles_w;
    int tiles;                                     // tiles of this scale per (pair, channel)
    int tile0, tiles_all;                          // first slot of this scale and slots of all scales per (pair, channel)
    const float* max_val;
    double* partials;
    float g[MAXF];
};

// Block (tile, channel, pair).  LDS at F = 11: two halos 2 x 26 x 43 floats, four row-filtered maps 4 x 26 x 32 floats, 22 KB.  Lanes
// 0..31 and 32..63 of a wave each walk one row, so every LDS access is 32 consecutive banks per lane group.
template <int F>
__global__ __launch_bounds__(256) void msssim_tile_kernel(const ScaleArgs p) {
    constexpr int HH = TH + F - 1, HW = TW + F - 1, HLD = HW + 1;
    __shared__ float xs[HH][HLD], ys[HH][HLD];
    __shared__ float hm[4][HH][TW];                                           // w pass of x, y, x*y, x*x + y*y
    __shared__ double red[4][2];
    __shared__ float gs[F];
    const int tile = blockIdx.x, c = blockIdx.y, pair = blockIdx.z;
    const int tw = tile % p.tiles_w, th = (tile / p.tiles_w) % p.tiles_h, td = tile / (p.tiles_w * p.tiles_h);
    const int z0 = td * TD, y0 = th * TH, x0 = tw * TW;
    const int oh = p.h - (F - 1), ow = p.w - (F - 1);
    const int vx = p.x_index ? p.x_index[pair] : pair, vy = p.y_index ? p.y_index[pair] : pair;
    if (vx < 0 || vx >= p.nx || vy < 0 || vy >= p.ny) {                        // uniform over the block: a bad table entry reads nothing
        if (threadIdx.x == 0) {
            double* dst = p.partials + (((long)pair * gridDim.y + c) * p.tiles_all + p.tile0 + tile) * 2;
            dst[0] = NAN; dst[1] = NAN;
        }
        return;
    }
    const long plane = (long)p.h * p.w;
    const float* xsrc = p.x + (long)vx * p.d * plane * p.cx + p.x0c + c;
    const float* ysrc = p.y + (long)vy * p.d * plane * p.cy + p.y0c + c;
    const float L = p.max_val[pair];
    const float k1 = __fmul_rn(0.01f, L), k2 = __fmul_rn(0.03f, L);
    const float c1 = __fmul_rn(k1, k1), c2 = __fmul_rn(k2, k2);
    const int q = threadIdx.x & (TW - 1), r0 = (threadIdx.x / TW) * ROWS;
    // the taps go through LDS into vector registers: as scalars each would be copied once per packed operand it feeds
    if (threadIdx.x < F) gs[threadIdx.x] = p.g[threadIdx.x];
    __syncthreads();
    float g[F];
#pragma unroll
    for (int k = 0; k < F; ++k) g[k] = gs[k];

    float acc[4][ROWS][F];                                                     // the d pass: acc[..][j] has taps 0..j of output plane z - j
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int o = 0; o < ROWS; ++o)
#pragma unroll
            for (int j = 0; j < F; ++j) acc[m][o][j] = 0.f;
    double s[2] = {0.0, 0.0};

    const int planes = min(TD + F - 1, p.d - z0);                              // input planes z0 .. z0 + planes - 1
    for (int sz = 0; sz < planes; ++sz) {
        const long zoff = (long)(z0 + sz) * plane;
        // 1. the halo of this plane, zero past the volume (outputs that would read those are not counted)
        for (int i = threadIdx.x; i < HH * HW; i += 256) {
            const int r = i / HW, k = i % HW;
            const int gy = y0 + r, gx = x0 + k;
            float xv = 0.f, yv = 0.f;
            if (gy < p.h && gx < p.w) {
                const long pix = zoff + (long)gy * p.w + gx;
                xv = xsrc[pix * p.cx];
                yv = ysrc[pix * p.cy];
            }
            xs[r][k] = xv;
            ys[r][k] = yv;
        }
        __syncthreads();
        // 2. the w pass: taps in index order, acc = fma(g[i], v[i], acc) from 0
        for (int i = threadIdx.x; i < HH * TW; i += 256) {
            const int r = i / TW, k0 = i % TW;
            float ax = 0.f, ay = 0.f, axy = 0.f, asq = 0.f;
#pragma unroll
            for (int k = 0; k < F; ++k) {
                const float xv = xs[r][k0 + k], yv = ys[r][k0 + k];
                ax = __fmaf_rn(g[k], xv, ax);
                ay = __fmaf_rn(g[k], yv, ay);
                axy = __fmaf_rn(g[k], __fmul_rn(xv, yv), axy);
                asq = __fmaf_rn(g[k], __fadd_rn(__fmul_rn(xv, xv), __fmul_rn(yv, yv)), asq);
            }
            hm[0][r][k0] = ax; hm[1][r][k0] = ay; hm[2][r][k0] = axy; hm[3][r][k0] = asq;
        }
        __syncthreads();
        // 3. the h pass: this thread's column q, output rows r0 .. r0 + ROWS - 1, from rows r0 .. r0 + ROWS + F - 2 of the four maps
        float v[4][ROWS];
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int o = 0; o < ROWS; ++o) v[m][o] = 0.f;
#pragma unroll
        for (int j = 0; j < F + ROWS - 1; ++j) {
            float t[4];
#pragma unroll
            for (int m = 0; m < 4; ++m) t[m] = hm[m][r0 + j][q];
#pragma unroll
            for (int o = 0; o < ROWS; ++o) {
                const int k = j - o;                                           // compile-time: ascending per output row as j ascends
                if (k >= 0 && k < F) {
#pragma unroll
                    for (int m = 0; m < 4; ++m) v[m][o] = __fmaf_rn(g[k], t[m], v[m][o]);
                }
            }
        }
        // 4. the d pass: output plane z - j takes tap j of this plane; descending j turns the update into the shift of the delay line
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
            for (int o = 0; o < ROWS; ++o) {
#pragma unroll
                for (int j = F - 1; j > 0; --j) acc[m][o][j] = __fmaf_rn(g[j], v[m][o], acc[m][o][j - 1]);
                acc[m][o][0] = __fmaf_rn(g[0], v[m][o], 0.f);
            }
        // 5. output plane z0 + sz - (F-1) is complete: the formula in float32, the sums in float64
        if (sz >= F - 1) {
#pragma unroll
            for (int o = 0; o < ROWS; ++o) {
                const float mx = acc[0][o][F - 1], my = acc[1][o][F - 1], sxy = acc[2][o][F - 1], sq = acc[3][o][F - 1];
                const float n0 = __fmul_rn(__fmul_rn(mx, my), 2.f);
                const float d0 = __fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my));
                const float lum = __fdiv_rn(__fadd_rn(n0, c1), __fadd_rn(d0, c1));
                const float cs = __fdiv_rn(__fadd_rn(__fsub_rn(__fmul_rn(sxy, 2.f), n0), c2), __fadd_rn(__fsub_rn(sq, d0), c2));
                if (y0 + r0 + o < oh && x0 + q < ow) {
                    s[0] += (double)cs;
                    s[1] += (double)__fmul_rn(lum, cs);
                }
            }
        }
        // the next plane's staging writes xs / ys, which nobody reads after barrier 2; its w pass writes hm behind its barrier 1
    }
    dm3d_block_sum_f64(s, red);
    if (threadIdx.x == 0) {
        double* dst = p.partials + (((long)pair * gridDim.y + c) * p.tiles_all + p.tile0 + tile) * 2;
        dst[0] = s[0]; dst[1] = s[1];
    }
}

// Thread per output element (volume, z, y, x, channel) of dst [n, d/2, h/2, w/2, nc]: the eight inputs in (dz, dy, dx) order.
__global__ __launch_bounds__(256) void msssim_pool_kernel(const float* src, float* dst, long total, int d, int h, int w, int cs, int c0, int nc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int d2 = d >> 1, h2 = h >> 1, w2 = w >> 1;
    long r = i;
    const int c = (int)(r % nc); r /= nc;
    const int x = (int)(r % w2); r /= w2;
    const int y = (int)(r % h2); r /= h2;
    const int z = (int)(r % d2);
    const long n = r / d2;
    const float* s0 = src + ((((n * d + 2 * z) * h + 2 * y) * w + 2 * x) * cs + c0 + c);
    float sum = 0.f;
#pragma unroll
    for (int dz = 0; dz < 2; ++dz)
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                const float t = s0[(((long)dz * h + dy) * w + dx) * cs];
                sum = (dz | dy | dx) ? __fadd_rn(sum, t) : t;
            }
    dst[i] = __fmul_rn(sum, 0.125f);
}

struct SumArgs {
    const double* partials;
    float* out;
    int pairs, nc, scales, tiles_all;
    int tile0[MAXS + 1];
    double points[MAXS];
    float power[MAXS];
};

// Thread per pair: channels in order, scales in order, each scale's tiles in order.
__global__ __launch_bounds__(256) void msssim_sum_kernel(const SumArgs p) {
    const int pair = blockIdx.x * 256 + threadIdx.x;
    if (pair >= p.pairs) return;
    double total = 0.0;
    for (int c = 0; c < p.nc; ++c) {
        const double* src = p.partials + ((long)pair * p.nc + c) * p.tiles_all * 2;
        double prod = 1.0;
        for (int j = 0; j < p.scales; ++j) {
            double cs = 0.0, ss = 0.0;
            for (int k = p.tile0[j]; k < p.tile0[j + 1]; ++k) {
                cs += src[2 * k];
                ss += src[2 * k + 1];
            }
            const double term = (j == p.scales - 1 ? ss : cs) / p.points[j];
            prod *= pow(term < 0.0 ? 0.0 : term, (double)p.power[j]);           // max(term, 0) that lets a NaN through
        }
        total += prod;
    }
    p.out[pair] = (float)(total / (double)p.nc);
}

template <int F>
void launch_tile(const ScaleArgs& a, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(msssim_tile_kernel<F>, grid, dim3(256), 0, st, a);
}

}  // namespace

extern "C" int dm3d_ms_ssim(const dm3d_ms_ssim_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "ms_ssim: null descriptor");
    DM3D_REQUIRE(d->x && d->y && d->max_val && d->out && d->partials, "ms_ssim: x/y/max_val/out/partials must be non-null");
    DM3D_REQUIRE(d->scales >= 1 && d->scales <= MAXS, "ms_ssim: scales=%d (in [1, %d])", d->scales, MAXS);
    DM3D_REQUIRE(d->scales == 1 || d->scratch, "ms_ssim: scratch must be non-null when scales=%d", d->scales);
    DM3D_REQUIRE(d->pairs >= 1 && d->pairs <= 65535, "ms_ssim: pairs=%d (in [1, 65535])", d->pairs);
    DM3D_REQUIRE(d->nx >= 1 && d->ny >= 1, "ms_ssim: nx=%d ny=%d volumes (both at least 1)", d->nx, d->ny);
    DM3D_REQUIRE(d->x_index || d->pairs <= d->nx, "ms_ssim: pairs=%d exceeds nx=%d and no x_index is given", d->pairs, d->nx);
    DM3D_REQUIRE(d->y_index || d->pairs <= d->ny, "ms_ssim: pairs=%d exceeds ny=%d and no y_index is given", d->pairs, d->ny);
    DM3D_REQUIRE(d->d >= 1 && d->h >= 1 && d->w >= 1, "ms_ssim: d=%d h=%d w=%d (all at least 1)", d->d, d->h, d->w);
    DM3D_REQUIRE(d->nc >= 1 && d->nc <= 65535, "ms_ssim: nc=%d (in [1, 65535])", d->nc);
    int rc = dm3d_check_window("ms_ssim", "x", d->x0c, d->nc, d->cx);
    if (rc != DM3D_OK || (rc = dm3d_check_window("ms_ssim", "y", d->y0c, d->nc, d->cy)) != DM3D_OK) return rc;
    const int F = d->filter_size;
    DM3D_REQUIRE(F >= 3 && F <= MAXF && (F & 1), "ms_ssim: filter_size=%d (odd, in [3, %d])", F, MAXF);
    DM3D_REQUIRE(d->filter_sigma > 0.f, "ms_ssim: filter_sigma=%g (positive)", (double)d->filter_sigma);
    for (int j = 0; j < d->scales; ++j)
        DM3D_REQUIRE(d->power_factors[j] > 0.f, "ms_ssim: power_factors[%d]=%g (positive)", j, (double)d->power_factors[j]);
    const int edge = d->d < d->h ? (d->d < d->w ? d->d : d->w) : (d->h < d->w ? d->h : d->w);
    int fit = 0;
    while (fit < MAXS && (edge >> fit) >= F) ++fit;
    DM3D_REQUIRE(d->scales <= fit, "ms_ssim: %d scales of a %d x %d x %d volume leave an edge smaller than filter_size=%d; at most %d scales fit",
                 d->scales, d->d, d->h, d->w, F, fit);
    DM3D_REQUIRE(dm3d_aligned(d->partials, 8), "ms_ssim: partials must be 8-byte aligned");

    SumArgs sa{};
    int64_t tiles[MAXS], tiles_all = 0, pooled = 0;
    for (int j = 0; j < d->scales; ++j) {
        const int64_t dj = d->d >> j, hj = d->h >> j, wj = d->w >> j;
        const int64_t od = dj - (F - 1), oh = hj - (F - 1), ow = wj - (F - 1);
        tiles[j] = ((od + TD - 1) / TD) * ((oh + TH - 1) / TH) * ((ow + TW - 1) / TW);
        sa.tile0[j] = (int)tiles_all;
        tiles_all += tiles[j];
        sa.points[j] = (double)od * (double)oh * (double)ow;
        sa.power[j] = d->power_factors[j];
        if (j) pooled += dj * hj * wj;
    }
    DM3D_REQUIRE(tiles_all <= 0x3fffffffLL, "ms_ssim: %lld tiles exceed the grid", (long long)tiles_all);
    sa.tile0[d->scales] = (int)tiles_all;
    const int64_t need_p = 2 * (int64_t)d->pairs * d->nc * tiles_all;
    DM3D_REQUIRE(d->partials_elems >= need_p, "ms_ssim: partials holds %lld doubles, %lld are needed (2 * pairs * nc * %lld tiles)",
                 (long long)d->partials_elems, (long long)need_p, (long long)tiles_all);
    const int64_t need_s = ((int64_t)d->nx + d->ny) * d->nc * pooled;
    DM3D_REQUIRE(d->scratch_elems >= need_s, "ms_ssim: scratch holds %lld floats, %lld are needed ((nx + ny) * nc * %lld pooled voxels)",
                 (long long)d->scratch_elems, (long long)need_s, (long long)pooled);
    DM3D_REQUIRE((need_s + 255) / 256 <= 0x7fffffffLL, "ms_ssim: %lld pooled elements exceed the grid", (long long)need_s);

    ScaleArgs a{};
    {   // the window: float64, normalised, rounded to float32
        double g[MAXF], sum = 0.0;
        const double sigma = (double)d->filter_sigma, mid = 0.5 * (F - 1);
        for (int i = 0; i < F; ++i) sum += g[i] = exp(-(i - mid) * (i - mid) / (2.0 * sigma * sigma));
        for (int i = 0; i < F; ++i) a.g[i] = (float)(g[i] / sum);
    }
    a.x = d->x; a.y = d->y; a.x_index = d->x_index; a.y_index = d->y_index; a.nx = d->nx; a.ny = d->ny;
    a.cx = d->cx; a.cy = d->cy; a.x0c = d->x0c; a.y0c = d->y0c;
    a.max_val = d->max_val; a.partials = d->partials; a.tiles_all = (int)tiles_all;
    hipStream_t st = static_cast<hipStream_t>(stream);
    float* next = d->scratch;
    for (int j = 0; j < d->scales; ++j) {
        a.d = d->d >> j; a.h = d->h >> j; a.w = d->w >> j;
        a.tiles_h = (a.h - (F - 1) + TH - 1) / TH;
        a.tiles_w = (a.w - (F - 1) + TW - 1) / TW;
        a.tiles = (int)tiles[j];
        a.tile0 = sa.tile0[j];
        const dim3 grid((unsigned)tiles[j], (unsigned)d->nc, (unsigned)d->pairs);
        switch (F) {
            case 3: launch_tile<3>(a, grid, st); break;
            case 5: launch_tile<5>(a, grid, st); break;
            case 7: launch_tile<7>(a, grid, st); break;
            case 9: launch_tile<9>(a, grid, st); break;
            default: launch_tile<11>(a, grid, st); break;
        }
        rc = dm3d_launch_check("msssim_tile_kernel");
        if (rc != DM3D_OK) return rc;
        if (j + 1 == d->scales) break;
        // the next scale's volumes: every volume of x, then every volume of y, the compared channels only
        const long vox = (long)(a.d >> 1) * (a.h >> 1) * (a.w >> 1) * d->nc;
        float* px = next;
        float* py = next + (long)d->nx * vox;
        next = py + (long)d->ny * vox;
        const long tx = (long)d->nx * vox, ty = (long)d->ny * vox;
        hipLaunchKernelGGL(msssim_pool_kernel, dim3((unsigned)((tx + 255) / 256)), dim3(256), 0, st, a.x, px, tx, a.d, a.h, a.w, a.cx, a.x0c, d->nc);
        if ((rc = dm3d_launch_check("msssim_pool_kernel")) != DM3D_OK) return rc;
        hipLaunchKernelGGL(msssim_pool_kernel, dim3((unsigned)((ty + 255) / 256)), dim3(256), 0, st, a.y, py, ty, a.d, a.h, a.w, a.cy, a.y0c, d->nc);
        if ((rc = dm3d_launch_check("msssim_pool_kernel")) != DM3D_OK) return rc;
        a.x = px; a.y = py; a.cx = a.cy = d->nc; a.x0c = a.y0c = 0;
    }
    sa.partials = d->partials; sa.out = d->out; sa.pairs = d->pairs; sa.nc = d->nc; sa.scales = d->scales; sa.tiles_all = (int)tiles_all;
    hipLaunchKernelGGL(msssim_sum_kernel, dim3((unsigned)((d->pairs + 255) / 256)), dim3(256), 0, st, sa);
    return dm3d_launch_check("msssim_sum_kernel");
}
