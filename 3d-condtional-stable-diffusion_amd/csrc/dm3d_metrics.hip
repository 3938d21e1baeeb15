// dm3d_metrics.hip — how well a reconstruction y matches the truth x (include/dm3d.h, dm3d_metric_desc): the per-slice squared error and
// the per-volume range of y in one streaming pass, tf.image.ssim per depth slice as one fused kernel (halo of x and y staged in LDS once,
// the 11-tap row pass into LDS, the column pass in registers, the formula, one float64 partial per tile), and tf.image.psnr from the
// squared error.  Plain HIP: no MFMA, no atomics.  Every sum is float64 in a fixed order: a thread over its elements in index order, the
// block by dm3d_block_sum_f64, blocks through a partials buffer in block order by a second launch: runs repeat bitwise.
// The channel-window check and the block min / max are dm3d_volume.h's.
#include "dm3d_volume.h"

namespace {

constexpr int PARTS = DM3D_PAIR_PARTIAL_BLOCKS;
constexpr int TILE = DM3D_SSIM_TILE, TAPS = 11, HALO = TILE + TAPS - 1;      // 32 x 32 outputs read 42 x 42 inputs
constexpr int HLD = HALO + 1;                                                 // row stride of the staged halo, in floats
constexpr int PAIR_PIXELS = 4096;                                             // pixels of a slice per block of dm3d_pair_stats

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, float64 rounded to float32
__device__ constexpr float G[TAPS] = {0.001028380123898387f, 0.0075987582094967365f, 0.036000773310661316f, 0.10936068743467331f,
                                      0.21300554275512695f,  0.26601171493530273f,   0.21300554275512695f,  0.10936068743467331f,
                                      0.036000773310661316f, 0.0075987582094967365f, 0.001028380123898387f};

struct MetricArgs {
    const float* x; const float* y;
    int d, h, w, cx, cy, x0c, y0c, nc;
    double* partials;
    float* y_min; float* y_max; float* y_range; double* sse;
    const float* max_val; float* out;
    int blocks;                                    // pair_stats: blocks per slice; ssim: tiles per (slice, channel)
    int tiles_x;                                   // ssim: tiles along w
};

// Block (blk, z, b): pixels [blk*n/P, (blk+1)*n/P) of slice (b, z), every compared channel.  partials[(slice*P + blk)*3 ..] = (sum of
// squared differences, min y, max y).
__global__ __launch_bounds__(256) void pair_stats_kernel(const MetricArgs p) {
    __shared__ double red[4][1];
    __shared__ float mm[4][2];
    const long slice = (long)blockIdx.z * p.d + blockIdx.y;
    const long npix = (long)p.h * p.w;
    const long lo = npix * blockIdx.x / gridDim.x, hi = npix * (blockIdx.x + 1) / gridDim.x;
    const float* xs = p.x + slice * npix * p.cx + p.x0c;
    const float* ys = p.y + slice * npix * p.cy + p.y0c;
    double s[1] = {0.0};
    float mn = INFINITY, mx = -INFINITY;
    for (long i = lo + threadIdx.x; i < hi; i += 256) {
        for (int c = 0; c < p.nc; ++c) {
            const float xv = xs[i * p.cx + c], yv = ys[i * p.cy + c];
            const double e = (double)xv - (double)yv;
            s[0] += e * e;
            mn = fminf(mn, yv);
            mx = fmaxf(mx, yv);
        }
    }
    dm3d_block_minmax_put(mn, mx, mm);
    dm3d_block_sum_f64(s, red);                                               // its barrier also publishes mm
    if (threadIdx.x == 0) {
        double* dst = p.partials + (slice * gridDim.x + blockIdx.x) * 3;
        dm3d_block_minmax_get(mn, mx, mm);
        dst[0] = s[0]; dst[1] = (double)mn; dst[2] = (double)mx;
    }
}

// Block b: thread t adds the partials of slices t, t + 256, .. of volume b in block order and keeps their min / max; the volume's
// min / max is that of the 256 threads.
__global__ __launch_bounds__(256) void pair_stats_sum_kernel(const MetricArgs p) {
    __shared__ float mm[4][2];
    const int b = blockIdx.x;
    float mn = INFINITY, mx = -INFINITY;
    for (int z = threadIdx.x; z < p.d; z += 256) {
        const long slice = (long)b * p.d + z;
        const double* src = p.partials + slice * p.blocks * 3;
        double s = 0.0;
        for (int k = 0; k < p.blocks; ++k) {
            s += src[3 * k];
            mn = fminf(mn, (float)src[3 * k + 1]);
            mx = fmaxf(mx, (float)src[3 * k + 2]);
        }
        p.sse[slice] = s;
    }
    dm3d_block_minmax(mn, mx, mm);
    if (threadIdx.x == 0) {
        p.y_min[b] = mn;
        p.y_max[b] = mx;
        if (p.y_range) p.y_range[b] = __fsub_rn(mx, mn);
    }
}

// Block (tile + tiles*channel, z, b).  LDS: the two halos 2 x 42 x 43 floats, the four row-filtered maps 4 x 42 x 32 floats, 36 KB in
// all: four blocks a CU.  Lanes of a wave walk a row of either image, so every LDS access is 32 consecutive banks per lane group.
__global__ __launch_bounds__(256) void ssim_tile_kernel(const MetricArgs p) {
    __shared__ float xs[HALO][HLD], ys[HALO][HLD];
    __shared__ float hm[4][HALO][TILE];                                       // row pass of x, y, x*y, x*x + y*y
    __shared__ double red[4][1];
    const int tile = blockIdx.x % p.blocks, c = blockIdx.x / p.blocks;
    const int ty = tile / p.tiles_x, tx = tile % p.tiles_x;
    const long slice = (long)blockIdx.z * p.d + blockIdx.y;
    const int oh = p.h - (TAPS - 1), ow = p.w - (TAPS - 1);
    const int y0 = ty * TILE, x0 = tx * TILE;
    const float* xsrc = p.x + slice * p.h * p.w * p.cx + p.x0c + c;
    const float* ysrc = p.y + slice * p.h * p.w * p.cy + p.y0c + c;
    // 1. the halo, zero past the image (outputs that would read those are not counted)
    for (int i = threadIdx.x; i < HALO * HALO; i += 256) {
        const int r = i / HALO, q = i % HALO;
        const int gy = y0 + r, gx = x0 + q;
        float xv = 0.f, yv = 0.f;
        if (gy < p.h && gx < p.w) {
            const long pix = (long)gy * p.w + gx;
            xv = xsrc[pix * p.cx];
            yv = ysrc[pix * p.cy];
        }
        xs[r][q] = xv;
        ys[r][q] = yv;
    }
    __syncthreads();
    // 2. the row pass: taps in index order, acc = fma(g[i], v[i], acc) from 0
    for (int i = threadIdx.x; i < HALO * TILE; i += 256) {
        const int r = i / TILE, q = i % TILE;
        float ax = 0.f, ay = 0.f, axy = 0.f, asq = 0.f;
#pragma unroll
        for (int k = 0; k < TAPS; ++k) {
            const float xv = xs[r][q + k], yv = ys[r][q + k];
            ax = __fmaf_rn(G[k], xv, ax);
            ay = __fmaf_rn(G[k], yv, ay);
            axy = __fmaf_rn(G[k], __fmul_rn(xv, yv), axy);
            asq = __fmaf_rn(G[k], __fadd_rn(__fmul_rn(xv, xv), __fmul_rn(yv, yv)), asq);
        }
        hm[0][r][q] = ax; hm[1][r][q] = ay; hm[2][r][q] = axy; hm[3][r][q] = asq;
    }
    __syncthreads();
    // 3. the column pass: this thread's column q, output rows r0 .. r0+3, from rows r0 .. r0+13 of the four maps
    const int q = threadIdx.x & (TILE - 1), r0 = (threadIdx.x / TILE) * 4;
    float acc[4][4];                                                           // [map][output row]
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int o = 0; o < 4; ++o) acc[m][o] = 0.f;
#pragma unroll
    for (int j = 0; j < TAPS + 3; ++j) {
        float v[4];
#pragma unroll
        for (int m = 0; m < 4; ++m) v[m] = hm[m][r0 + j][q];
#pragma unroll
        for (int o = 0; o < 4; ++o) {
            const int k = j - o;                                               // compile-time: ascending per output row as j ascends
            if (k >= 0 && k < TAPS) {
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[m][o] = __fmaf_rn(G[k], v[m], acc[m][o]);
            }
        }
    }
    // 4. the formula, float32 in TensorFlow's order; the tile's sum in float64
    const float L = p.max_val[blockIdx.z];
    const float k1 = __fmul_rn(0.01f, L), k2 = __fmul_rn(0.03f, L);
    const float c1 = __fmul_rn(k1, k1), c2 = __fmul_rn(k2, k2);
    double s[1] = {0.0};
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        const float mx = acc[0][o], my = acc[1][o], sxy = acc[2][o], sq = acc[3][o];
        const float n0 = __fmul_rn(__fmul_rn(mx, my), 2.f);
        const float d0 = __fadd_rn(__fmul_rn(mx, mx), __fmul_rn(my, my));
        const float lum = __fdiv_rn(__fadd_rn(n0, c1), __fadd_rn(d0, c1));
        const float cs = __fdiv_rn(__fadd_rn(__fsub_rn(__fmul_rn(sxy, 2.f), n0), c2), __fadd_rn(__fsub_rn(sq, d0), c2));
        if (y0 + r0 + o < oh && x0 + q < ow) s[0] += (double)__fmul_rn(lum, cs);
    }
    dm3d_block_sum_f64(s, red);
    if (threadIdx.x == 0) p.partials[(slice * p.nc + c) * p.blocks + tile] = s[0];
}

// Thread per slice: channels in order, each channel's tiles in order.
__global__ __launch_bounds__(256) void ssim_sum_kernel(const MetricArgs p, long slices) {
    const long slice = (long)blockIdx.x * 256 + threadIdx.x;
    if (slice >= slices) return;
    const double n = (double)(p.h - (TAPS - 1)) * (double)(p.w - (TAPS - 1));
    double total = 0.0;
    for (int c = 0; c < p.nc; ++c) {
        const double* src = p.partials + (slice * p.nc + c) * p.blocks;
        double s = 0.0;
        for (int k = 0; k < p.blocks; ++k) s += src[k];
        total += s / n;
    }
    p.out[slice] = (float)(total / (double)p.nc);
}

__global__ __launch_bounds__(256) void psnr_kernel(const MetricArgs p, long slices) {
    const long slice = (long)blockIdx.x * 256 + threadIdx.x;
    if (slice >= slices) return;
    const float L = p.max_val[slice / p.d];
    const float mse = (float)(p.sse[slice] / ((double)p.h * (double)p.w * (double)p.nc));
    p.out[slice] = __fsub_rn((float)(20.0 * log10((double)L)), (float)(10.0 * log10((double)mse)));
}

// The checks the three entries share; `who` names the entry in the message.
int check_common(const dm3d_metric_desc* d, const char* who, int min_edge) {
    DM3D_REQUIRE(d != nullptr, "%s: null descriptor", who);
    DM3D_REQUIRE(d->batch >= 1 && d->batch <= 65535 && d->d >= 1 && d->d <= 65535, "%s: batch=%d d=%d (both in [1, 65535])", who, d->batch,
                 d->d);
    DM3D_REQUIRE(d->h >= min_edge && d->w >= min_edge, "%s: h=%d w=%d (both at least %d%s)", who, d->h, d->w, min_edge,
                 min_edge > 1 ? ", the 11 x 11 window" : "");
    DM3D_REQUIRE(d->nc >= 1, "%s: nc=%d (at least one channel is compared)", who, d->nc);
    return DM3D_OK;
}

int check_channels(const dm3d_metric_desc* d, const char* who) {
    const int rc = dm3d_check_window(who, "x", d->x0c, d->nc, d->cx);
    return rc != DM3D_OK ? rc : dm3d_check_window(who, "y", d->y0c, d->nc, d->cy);
}

MetricArgs make_args(const dm3d_metric_desc* d) {
    MetricArgs a{};
    a.x = d->x; a.y = d->y; a.d = d->d; a.h = d->h; a.w = d->w; a.cx = d->cx; a.cy = d->cy; a.x0c = d->x0c; a.y0c = d->y0c; a.nc = d->nc;
    a.partials = d->partials; a.y_min = d->y_min; a.y_max = d->y_max; a.y_range = d->y_range; a.sse = d->sse;
    a.max_val = d->max_val; a.out = d->out;
    return a;
}

}  // namespace

extern "C" int dm3d_pair_stats(const dm3d_metric_desc* d, void* stream) {
    int rc = check_common(d, "pair_stats", 1);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->x && d->y && d->partials && d->y_min && d->y_max && d->sse, "pair_stats: x/y/partials/y_min/y_max/sse must be non-null");
    if ((rc = check_channels(d, "pair_stats")) != DM3D_OK) return rc;
    DM3D_REQUIRE(dm3d_aligned(d->partials, 8) && dm3d_aligned(d->sse, 8), "pair_stats: partials/sse must be 8-byte aligned");
    const int64_t npix = (int64_t)d->h * d->w, want = (npix + PAIR_PIXELS - 1) / PAIR_PIXELS;
    const int blocks = (int)(want > PARTS ? PARTS : want);
    const int64_t need = 3 * (int64_t)d->batch * d->d * blocks;
    DM3D_REQUIRE(d->partials_elems >= need, "pair_stats: partials holds %lld doubles, %lld are needed (3 * batch * d * %d blocks)",
                 (long long)d->partials_elems, (long long)need, blocks);
    MetricArgs a = make_args(d);
    a.blocks = blocks;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(pair_stats_kernel, dim3((unsigned)blocks, (unsigned)d->d, (unsigned)d->batch), dim3(256), 0, st, a);
    if ((rc = dm3d_launch_check("pair_stats_kernel")) != DM3D_OK) return rc;
    hipLaunchKernelGGL(pair_stats_sum_kernel, dim3((unsigned)d->batch), dim3(256), 0, st, a);
    return dm3d_launch_check("pair_stats_sum_kernel");
}

extern "C" int dm3d_ssim(const dm3d_metric_desc* d, void* stream) {
    int rc = check_common(d, "ssim", TAPS);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->x && d->y && d->partials && d->max_val && d->out, "ssim: x/y/partials/max_val/out must be non-null");
    if ((rc = check_channels(d, "ssim")) != DM3D_OK) return rc;
    DM3D_REQUIRE(dm3d_aligned(d->partials, 8), "ssim: partials must be 8-byte aligned");
    const int64_t tiles_y = (d->h - (TAPS - 1) + TILE - 1) / TILE, tiles_x = (d->w - (TAPS - 1) + TILE - 1) / TILE;
    const int64_t tiles = tiles_y * tiles_x, need = (int64_t)d->batch * d->d * d->nc * tiles;
    DM3D_REQUIRE(tiles * d->nc <= 0x7fffffffLL, "ssim: %lld tiles x %d channels exceed the grid", (long long)tiles, d->nc);
    DM3D_REQUIRE(d->partials_elems >= need, "ssim: partials holds %lld doubles, %lld are needed (batch * d * nc * %lld tiles)",
                 (long long)d->partials_elems, (long long)need, (long long)tiles);
    MetricArgs a = make_args(d);
    a.blocks = (int)tiles;
    a.tiles_x = (int)tiles_x;
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(ssim_tile_kernel, dim3((unsigned)(tiles * d->nc), (unsigned)d->d, (unsigned)d->batch), dim3(256), 0, st, a);
    if ((rc = dm3d_launch_check("ssim_tile_kernel")) != DM3D_OK) return rc;
    const long slices = (long)d->batch * d->d;
    hipLaunchKernelGGL(ssim_sum_kernel, dim3((unsigned)((slices + 255) / 256)), dim3(256), 0, st, a, slices);
    return dm3d_launch_check("ssim_sum_kernel");
}

extern "C" int dm3d_psnr_finalize(const dm3d_metric_desc* d, void* stream) {
    int rc = check_common(d, "psnr_finalize", 1);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->sse && d->max_val && d->out, "psnr_finalize: sse/max_val/out must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->sse, 8), "psnr_finalize: sse must be 8-byte aligned");
    MetricArgs a = make_args(d);
    const long slices = (long)d->batch * d->d;
    hipLaunchKernelGGL(psnr_kernel, dim3((unsigned)((slices + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), a, slices);
    return dm3d_launch_check("psnr_kernel");
}
