// dm3d_deform.hip — device-side spatial augmentation (include/dm3d.h, "Spatial augmentation"): the separable Gaussian filter by
// scipy.ndimage.gaussian_filter's rules, the uniform draw behind a random elastic displacement field, and the resample at per-voxel
// coordinates (an affine table plus a displacement field, scipy.ndimage.map_coordinates).  Sums and coordinates are float64 in one fixed
// order, the stores float32; no kernel here uses an atomic, so runs repeat bitwise.  Plain HIP: no MFMA, no inline assembly.
// The tiling of the Gaussian passes is dm3d_volume.h's, the taps and the tap sum of the warp are dm3d_interp.h's.
#include "dm3d_volume.h"
#include "dm3d_interp.h"
#include "dm3d_philox.h"
#include <math.h>

namespace {

constexpr int MAXE = DM3D_SPLINE_MAX_EXTENT;       // longest line staged in LDS
constexpr int MAXR = DM3D_GAUSS_MAX_RADIUS;
constexpr int LDT = DM3D_LINE_LDT;                 // LDS row of one line position
constexpr int BX = DM3D_BRICK_X, BY = DM3D_BRICK_Y, BZ = DM3D_BRICK_Z;
constexpr uint32_t STREAM_ELASTIC = DM3D_STREAM_ELASTIC;

// ---- the Gaussian filter -------------------------------------------------------------------------------------------------------------
struct GaussArgs {
    const float* in;                               // the first pass that runs reads x, the later ones out
    float* out;
    dm3d_line_pass line;                           // length 1 .. MAXE
    int r, mode;
    double cval;
    double w[MAXR + 1];                            // w[0] the centre, w[k] = w[-k]: the host's float64 values
};

// Where tap i of a line of n lies in the staged line, by scipy's extension rules; -1: it reads cval.  Any i, any n >= 1.
__device__ __forceinline__ int gauss_tap(int i, int n, int mode) {
    if (i >= 0 && i < n) return i;
    if (mode == DM3D_GAUSS_NEAREST) return i < 0 ? 0 : n - 1;
    if (mode == DM3D_GAUSS_CONSTANT) return -1;
    if (mode == DM3D_GAUSS_MIRROR) return mirror_tap(i, n);
    const int period = 2 * n;                      // reflect: the edge is repeated
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - 1 - i;
}

// One pass of scipy.ndimage.correlate1d with a symmetric kernel over each of LANES neighbouring lines of one group: the lines are staged
// in LDS as [n][LDT] float32 by all 256 lanes in the order of memory (dm3d_line_walk), and the same walk then forms every output,
//     t = x[l] w[0];   t += (x[l - k] + x[l + k]) w[k]   for k = r .. 1,
// in float64 and stores it as float32.  No halo is staged: a tap outside the line maps into it (gauss_tap), so r may exceed n.  A block
// reads its lines whole before it writes any of them, so out may be in.
template <bool ALONG>
__global__ __launch_bounds__(256) void gauss_pass_kernel(const GaussArgs p) {
    extern __shared__ float staged[];
    const int n = p.line.n, r = p.r;
    const dm3d_line_block blk = dm3d_line_block_of(p.line);
    dm3d_line_walk<ALONG>(p.line, blk, [&](int at, long off, bool live) {
        if (live) staged[at] = p.in[off];
    });
    __syncthreads();
    dm3d_line_walk<ALONG>(p.line, blk, [&](int at, long off, bool live) {
        if (!live) return;
        const int j = at / LDT;
        const float* c = staged + (at - j * LDT);
        double t = (double)c[j * LDT] * p.w[0];
        if (j >= r && j + r < n) {
            for (int k = r; k >= 1; --k) t += ((double)c[(j - k) * LDT] + (double)c[(j + k) * LDT]) * p.w[k];
        } else {
            for (int k = r; k >= 1; --k) {
                const int a = gauss_tap(j - k, n, p.mode), b = gauss_tap(j + k, n, p.mode);
                const double va = a < 0 ? p.cval : (double)c[a * LDT], vb = b < 0 ? p.cval : (double)c[b * LDT];
                t += (va + vb) * p.w[k];
            }
        }
        p.out[off] = (float)t;
    });
}

// out[v][i] = in[v][i] * gain[v % gains] in float32 (gains = 0: a copy), over [volumes][n] flat; out may be in.
__global__ __launch_bounds__(256) void gauss_gain_kernel(const float* in, float* out, long n, long total, int gains, float g0, float g1, float g2) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int k = gains ? (int)((i / n) % gains) : 0;
        out[i] = gains ? in[i] * (k == 0 ? g0 : k == 1 ? g1 : g2) : in[i];
    }
}

// ---- the uniform field ---------------------------------------------------------------------------------------------------------------
// One lane per Philox block: elements 4b .. 4b + 3 take the words of counter (lo32(b), hi32(b), draw, STREAM_ELASTIC) under the key seed,
// v = (float)word * 2^-32 (aug_draw_kernel's rule), then 2 v - 1 in float32.
__global__ __launch_bounds__(256) void uniform_field_kernel(float* out, long n, uint32_t draw, uint64_t seed) {
    const long b = (long)blockIdx.x * 256 + threadIdx.x;
    if (b * 4 >= n) return;
    uint32_t c[4] = {(uint32_t)b, (uint32_t)((uint64_t)b >> 32), draw, STREAM_ELASTIC};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (b * 4 + k < n) out[b * 4 + k] = 2.0f * ((float)c[k] * 2.3283064365386963e-10f) - 1.0f;
}

// ---- the warp ------------------------------------------------------------------------------------------------------------------------
struct WarpArgs {
    const void* in;                                // [volumes][id][ih][iw] float32 or float64
    const double* table;                           // [volumes][12]: the matrix row by row, then the offset
    const void* field;                             // [fields][3][od][oh][ow] float32 or float64, or null
    float* out;                                    // [volumes][od][oh][ow]
    int id, ih, iw, od, oh, ow;
    int tx, ty;                                    // bricks along x and y
    int per_field, field_f64;
    float cval;
};

// Grid (bricks, volumes), the brick of resample_kernel.  c[h] = (((oz m[3h] + oy m[3h+1]) + ox m[3h+2]) + m[9+h]) + (double)u[h][o] in
// float64; the three reads of u are coalesced along x like the store.  Everything after the coordinate is dm3d_interp_store.
template <int ORDER, typename T>
__global__ __launch_bounds__(256) void warp_kernel(const WarpArgs p) {
    const int v = blockIdx.y;
    int oz, oy, ox;
    if (!dm3d_brick_voxel(p.tx, p.ty, p.od, p.oh, p.ow, oz, oy, ox)) return;
    const double* m = p.table + (long)v * 12;
    const long vox = (long)p.od * p.oh * p.ow, o = ((long)oz * p.oh + oy) * p.ow + ox;
    const long u0 = (long)(v / p.per_field) * 3 * vox + o;
    double c[3];
#pragma unroll
    for (int h = 0; h < 3; ++h) {
        c[h] = (((double)oz * m[3 * h] + (double)oy * m[3 * h + 1]) + (double)ox * m[3 * h + 2]) + m[9 + h];
        if (p.field) c[h] += p.field_f64 ? static_cast<const double*>(p.field)[u0 + h * vox] : (double)static_cast<const float*>(p.field)[u0 + h * vox];
    }
    dm3d_interp_store<ORDER, T>(static_cast<const T*>(p.in) + (long)v * p.id * p.ih * p.iw, p.id, p.ih, p.iw, c, p.cval, p.out + (long)v * vox + o);
}

template <int ORDER>
int launch_warp(const dm3d_warp_desc* d, const WarpArgs& a, dim3 grid, hipStream_t st) {
    if (d->in_f64) hipLaunchKernelGGL((warp_kernel<ORDER, double>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((warp_kernel<ORDER, float>), grid, dim3(256), 0, st, a);
    return dm3d_launch_check("warp_kernel");
}

}  // namespace

extern "C" int dm3d_gaussian_filter(const dm3d_gauss_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "gaussian_filter: null descriptor");
    DM3D_REQUIRE(d->x != nullptr && d->out != nullptr, "gaussian_filter: x and out must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->x, 4) && dm3d_aligned(d->out, 4), "gaussian_filter: x and out must be 4-byte aligned");
    DM3D_REQUIRE(d->volumes >= 1, "gaussian_filter: volumes=%d (at least 1)", d->volumes);
    DM3D_REQUIRE(d->d >= 1 && d->h >= 1 && d->w >= 1, "gaussian_filter: extent d=%d h=%d w=%d (all at least 1)", d->d, d->h, d->w);
    DM3D_REQUIRE(d->d <= MAXE && d->h <= MAXE && d->w <= MAXE, "gaussian_filter: d=%d h=%d w=%d exceeds DM3D_SPLINE_MAX_EXTENT=%d per axis", d->d, d->h,
                 d->w, MAXE);
    const int radius[3] = {d->rd, d->rh, d->rw};
    DM3D_REQUIRE(d->rd >= -1 && d->rh >= -1 && d->rw >= -1 && d->rd <= MAXR && d->rh <= MAXR && d->rw <= MAXR,
                 "gaussian_filter: radius rd=%d rh=%d rw=%d (-1, an axis left out, to DM3D_GAUSS_MAX_RADIUS=%d)", d->rd, d->rh, d->rw, MAXR);
    DM3D_REQUIRE(d->weights != nullptr || (d->rd < 0 && d->rh < 0 && d->rw < 0), "gaussian_filter: weights must be non-null where an axis is filtered");
    DM3D_REQUIRE(d->mode >= DM3D_GAUSS_REFLECT && d->mode <= DM3D_GAUSS_CONSTANT, "gaussian_filter: mode=%d (DM3D_GAUSS_REFLECT, _MIRROR, _NEAREST or _CONSTANT)",
                 d->mode);
    DM3D_REQUIRE(isfinite(d->cval), "gaussian_filter: cval=%g (finite)", d->cval);
    for (int a = 0; a < 3; ++a)
        for (int k = 0; k <= radius[a]; ++k)
            DM3D_REQUIRE(isfinite(d->weights[a * (MAXR + 1) + k]), "gaussian_filter: weights[%d][%d]=%g (finite)", a, k, d->weights[a * (MAXR + 1) + k]);
    DM3D_REQUIRE(d->gains == 0 || d->gains == 1 || d->gains == 3, "gaussian_filter: gains=%d (0, 1 or 3)", d->gains);
    DM3D_REQUIRE(d->gains == 0 || (isfinite(d->gain0) && isfinite(d->gain1) && isfinite(d->gain2)), "gaussian_filter: gain (%g, %g, %g) (finite)",
                 (double)d->gain0, (double)d->gain1, (double)d->gain2);
    const uint64_t bytes = (uint64_t)d->volumes * d->d * d->h * d->w * 4;
    DM3D_REQUIRE(d->x == d->out || !dm3d_ranges_overlap(d->x, bytes, d->out, bytes), "gaussian_filter: out must be x itself or share no byte with it");
    int64_t blocks = 0;
    DM3D_REQUIRE(dm3d_line_grid_fault(d->volumes, d->d, d->h, d->w, &blocks) < 0, "gaussian_filter: %lld volumes exceed the grid", (long long)d->volumes);
    static std::atomic<bool> lds_set[64];
    const int dev = dm3d_dyn_lds((size_t)MAXE * LDT * sizeof(float), lds_set, "gaussian_filter", gauss_pass_kernel<true>, gauss_pass_kernel<false>);
    if (dev < 0) return dev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    static const char* const names[3] = {"gauss_pass_kernel (d)", "gauss_pass_kernel (h)", "gauss_pass_kernel (w)"};
    GaussArgs a{};
    a.in = d->x; a.out = d->out; a.mode = d->mode; a.cval = d->cval;
    int rc;
    for (int axis = 0; axis < 3; ++axis) {                                      // scipy's order: d, h, w; the tiler counts its axes from w
        if (radius[axis] < 0) continue;
        blocks = dm3d_line_pass_fill(&a.line, 2 - axis, d->volumes, d->d, d->h, d->w);
        a.r = radius[axis];
        for (int k = 0; k <= a.r; ++k) a.w[k] = d->weights[axis * (MAXR + 1) + k];
        hipLaunchKernelGGL(axis == 2 ? gauss_pass_kernel<true> : gauss_pass_kernel<false>, dim3((unsigned)blocks), dim3(256),
                           (size_t)a.line.n * LDT * sizeof(float), st, a);
        if ((rc = dm3d_launch_check(names[axis])) != DM3D_OK) return rc;
        a.in = d->out;
    }
    if (d->gains || (a.in == d->x && d->x != d->out)) {                         // the gain of a field, or the copy when no axis was filtered
        const int64_t n = (int64_t)d->d * d->h * d->w, total = n * d->volumes, want = (total + 255) / 256;
        hipLaunchKernelGGL(gauss_gain_kernel, dim3((unsigned)(want < 65536 ? want : 65536)), dim3(256), 0, st, a.in, d->out, (long)n, (long)total,
                           (int)d->gains, d->gain0, d->gain1, d->gain2);
        if ((rc = dm3d_launch_check("gauss_gain_kernel")) != DM3D_OK) return rc;
    }
    return DM3D_OK;
}

extern "C" int dm3d_uniform_field(const dm3d_field_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "uniform_field: null descriptor");
    DM3D_REQUIRE(d->out != nullptr, "uniform_field: out must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->out, 4), "uniform_field: out must be 4-byte aligned");
    DM3D_REQUIRE(d->n >= 1, "uniform_field: n=%lld (at least 1)", (long long)d->n);
    DM3D_REQUIRE(d->draw >= 0, "uniform_field: draw=%d (at least 0)", d->draw);
    const int64_t blocks = ((d->n + 3) / 4 + 255) / 256;
    DM3D_REQUIRE(blocks <= 0x7fffffffLL, "uniform_field: n=%lld exceeds the grid", (long long)d->n);
    hipLaunchKernelGGL(uniform_field_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), d->out, (long)d->n, (uint32_t)d->draw,
                       (uint64_t)d->seed);
    return dm3d_launch_check("uniform_field_kernel");
}

extern "C" int dm3d_warp(const dm3d_warp_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "warp: null descriptor");
    DM3D_REQUIRE(d->src != nullptr && d->table != nullptr && d->out != nullptr, "warp: src, table and out must be non-null");
    DM3D_REQUIRE(d->in_f64 == DM3D_RESAMPLE_F32 || d->in_f64 == DM3D_RESAMPLE_F64, "warp: in_f64=%d (DM3D_RESAMPLE_F32 or DM3D_RESAMPLE_F64)", d->in_f64);
    DM3D_REQUIRE(d->field_f64 == DM3D_RESAMPLE_F32 || d->field_f64 == DM3D_RESAMPLE_F64, "warp: field_f64=%d (DM3D_RESAMPLE_F32 or DM3D_RESAMPLE_F64)",
                 d->field_f64);
    DM3D_REQUIRE(dm3d_aligned(d->src, d->in_f64 ? 8 : 4) && dm3d_aligned(d->table, 8) && dm3d_aligned(d->field, d->field_f64 ? 8 : 4) && dm3d_aligned(d->out, 4),
                 "warp: src and field must be aligned to their element, table 8-byte and out 4-byte aligned");
    DM3D_REQUIRE(d->order == 0 || d->order == 1 || d->order == 3, "warp: order=%d (0, 1 or 3; orders 2, 4 and 5 are not offered)", d->order);
    DM3D_REQUIRE(d->volumes >= 1 && d->volumes <= 65535, "warp: volumes=%d (1 to 65535)", d->volumes);
    DM3D_REQUIRE(d->vols_per_field >= 1 && d->volumes % d->vols_per_field == 0, "warp: vols_per_field=%d (at least 1, a divisor of volumes=%d)",
                 d->vols_per_field, d->volumes);
    DM3D_REQUIRE(d->id >= 1 && d->ih >= 1 && d->iw >= 1, "warp: input d=%d h=%d w=%d (all at least 1)", d->id, d->ih, d->iw);
    DM3D_REQUIRE(d->od >= 1 && d->oh >= 1 && d->ow >= 1, "warp: output d=%d h=%d w=%d (all at least 1)", d->od, d->oh, d->ow);
    DM3D_REQUIRE(isfinite(d->cval), "warp: cval=%g (finite)", (double)d->cval);
    DM3D_REQUIRE((int64_t)d->id * d->ih * d->iw <= 0x7fffffffLL, "warp: an input volume of %lld voxels (at most 2^31 - 1)", (long long)d->id * d->ih * d->iw);
    DM3D_REQUIRE(!dm3d_ranges_overlap(d->src, (uint64_t)d->volumes * d->id * d->ih * d->iw * (d->in_f64 ? 8 : 4), d->out,
                                      (uint64_t)d->volumes * d->od * d->oh * d->ow * 4), "warp: out must not overlap src (a warp is not in place)");
    WarpArgs a{};
    a.in = d->src; a.table = d->table; a.field = d->field; a.out = d->out;
    a.id = d->id; a.ih = d->ih; a.iw = d->iw; a.od = d->od; a.oh = d->oh; a.ow = d->ow;
    a.tx = (d->ow + BX - 1) / BX; a.ty = (d->oh + BY - 1) / BY;
    a.per_field = d->vols_per_field; a.field_f64 = d->field_f64;
    a.cval = d->cval;
    const int64_t bricks = (int64_t)a.tx * a.ty * ((d->od + BZ - 1) / BZ);
    DM3D_REQUIRE(bricks <= 0x7fffffffLL, "warp: %lld output bricks exceed the grid", (long long)bricks);
    const dim3 grid((unsigned)bricks, (unsigned)d->volumes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->order == 0) return launch_warp<0>(d, a, grid, st);
    if (d->order == 1) return launch_warp<1>(d, a, grid, st);
    return launch_warp<3>(d, a, grid, st);
}
