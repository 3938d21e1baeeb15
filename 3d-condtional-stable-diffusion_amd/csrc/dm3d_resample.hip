// dm3d_resample.hip — device-side volume preprocessing (include/dm3d.h, "Volume preprocessing"): the cubic B-spline prefilter, the affine
// resample at orders 0, 1 and 3 by scipy.ndimage's rules, fold-and-min-max normalisation and the flip / brightness / contrast
// augmentation.  Coordinates, weights, coefficients and every sum are float64 in one fixed order, the stores float32 (float64 for the
// coefficients); no kernel here uses an atomic, so runs repeat bitwise.  Plain HIP: no MFMA, no inline assembly.
// The tiling of the three prefilter passes and the block min / max are dm3d_volume.h's, the taps and the tap sum dm3d_interp.h's.
#include "dm3d_volume.h"
#include "dm3d_interp.h"
#include "dm3d_philox.h"
#include <math.h>

namespace {

constexpr int MAXE = DM3D_SPLINE_MAX_EXTENT;       // longest line staged in LDS
constexpr int LDT = DM3D_LINE_LDT;                 // LDS row of one line position
constexpr int BX = DM3D_BRICK_X, BY = DM3D_BRICK_Y, BZ = DM3D_BRICK_Z;
constexpr int NORM_BLOCKS = DM3D_NORM_PARTIAL_BLOCKS;
constexpr int AUG_BLOCKS = DM3D_AUG_PARTIAL_BLOCKS;
constexpr uint32_t STREAM_AUGMENT = DM3D_STREAM_AUGMENT;

// ---- the prefilter -------------------------------------------------------------------------------------------------------------------
struct FilterArgs {
    const float* x;                                // first pass: the float32 input
    double* c;                                     // in place (first pass: out only)
    dm3d_line_pass line;                           // length 1 .. MAXE; 1: the pass only copies
    int first;
    double z, gain, zn1;                           // the pole sqrt(3) - 2, (1 - z)(1 - 1/z), z^(n-1) by n - 1 products: the host's values
};

// One causal and one anti-causal recursion over each of LANES neighbouring lines of one group, in place: scipy.ndimage.spline_filter1d
// (order 3, mode "mirror") operation by operation.  The lines are staged in LDS as [n][LDT] float64 by all 256 lanes, in the order of
// memory (dm3d_line_walk).  Lane l < LANES then owns line l; its LDS reads and writes are LANES consecutive float64.  A line of length
// 1 is left as it is.
template <bool ALONG>
__global__ __launch_bounds__(256) void spline_pass_kernel(const FilterArgs p) {
    extern __shared__ double col[];
    const int n = p.line.n;
    const dm3d_line_block blk = dm3d_line_block_of(p.line);
    const double gain = n > 1 ? p.gain : 1.0;
    dm3d_line_walk<ALONG>(p.line, blk, [&](int at, long off, bool live) {
        if (live) col[at] = (p.first ? (double)p.x[off] : p.c[off]) * gain;
    });
    __syncthreads();
    if ((int)threadIdx.x < blk.nl && n > 1) {
        double* c = col + threadIdx.x;
        const double z = p.z, zn1 = p.zn1;
        double c0 = c[0] + zn1 * c[(n - 1) * LDT], zi = z;
        for (int i = 1; i < n - 1; ++i) {
            c0 += zi * (c[i * LDT] + zn1 * c[(n - 1 - i) * LDT]);
            zi *= z;
        }
        c0 /= 1.0 - zn1 * zn1;
        c[0] = c0;
        double prev = c0;
        for (int i = 1; i < n; ++i) {
            prev = c[i * LDT] + z * prev;
            c[i * LDT] = prev;
        }
        prev = (z * c[(n - 2) * LDT] + prev) * z / (z * z - 1.0);
        c[(n - 1) * LDT] = prev;
        for (int i = n - 2; i >= 0; --i) {
            prev = z * (prev - c[i * LDT]);
            c[i * LDT] = prev;
        }
    }
    __syncthreads();
    dm3d_line_walk<ALONG>(p.line, blk, [&](int at, long off, bool live) {
        if (live) p.c[off] = col[at];
    });
}

// ---- the resample --------------------------------------------------------------------------------------------------------------------
struct ResArgs {
    const void* in;                                // [volumes][id][ih][iw] float32 or float64
    const double* table;                           // [volumes][12]: the matrix row by row, then the offset
    float* out;                                    // [volumes][od][oh][ow]
    int id, ih, iw, od, oh, ow;
    int tx, ty;                                    // bricks along x and y
    float cval;
};

// Grid (bricks, volumes); a block owns a brick of BZ x BY x BX outputs, a wave one z-slice of it: BX = 16 neighbours along x read 16
// (times the x scale) neighbouring input elements per tap row, one 128-byte line of float64 at unit scale, and the BY rows and BZ
// slices share three of their four tap rows and planes with their neighbours.  out = sum over the taps, axis 0 outermost, of
// ((in * w0) * w1) * w2 in float64, stored as float32; a coordinate outside [0, n - 1] on any axis (or not a number) gives cval.
template <int ORDER, typename T>
__global__ __launch_bounds__(256) void resample_kernel(const ResArgs p) {
    const int v = blockIdx.y;
    int oz, oy, ox;
    if (!dm3d_brick_voxel(p.tx, p.ty, p.od, p.oh, p.ow, oz, oy, ox)) return;
    const double* m = p.table + (long)v * 12;
    double c[3];
#pragma unroll
    for (int h = 0; h < 3; ++h) c[h] = (((double)oz * m[3 * h] + (double)oy * m[3 * h + 1]) + (double)ox * m[3 * h + 2]) + m[9 + h];
    dm3d_interp_store<ORDER, T>(static_cast<const T*>(p.in) + (long)v * p.id * p.ih * p.iw, p.id, p.ih, p.iw, c, p.cval,
                                p.out + (((long)v * p.od + oz) * p.oh + oy) * p.ow + ox);
}

// ---- fold and min-max normalise --------------------------------------------------------------------------------------------------------
struct NormArgs {
    const float* x; float* out;                    // [volumes][n]
    long n;
    int blocks;                                    // blocks a volume: min(ceil(n / 1024), NORM_BLOCKS)
    float* partials;                               // [volumes][NORM_BLOCKS][2]
    float* minmax;                                 // [volumes][2]
    int* flag;                                     // [volumes]
};

// Grid (blocks, volumes): partials[v][block] = min and max of |x| over the block's share.
__global__ __launch_bounds__(256) void norm_minmax_kernel(const NormArgs p) {
    __shared__ float red[4][2];
    const float* x = p.x + (long)blockIdx.y * p.n;
    float mn = INFINITY, mx = -INFINITY;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)p.blocks * 256) {
        const float a = fabsf(x[i]);
        mn = fminf(mn, a);
        mx = fmaxf(mx, a);
    }
    dm3d_block_minmax(mn, mx, red);
    if (threadIdx.x == 0) {
        float* o = p.partials + ((long)blockIdx.y * NORM_BLOCKS + blockIdx.x) * 2;
        o[0] = mn; o[1] = mx;
    }
}

// Grid (blocks, volumes): every block folds the volume's partials again (the same values whatever the order), block 0 leaves them and
// the flag, and all of them write (|x| - min) / (max - min), float64 rounded once; zeros where max = min.
__global__ __launch_bounds__(256) void norm_apply_kernel(const NormArgs p) {
    __shared__ float red[4][2];
    const int v = blockIdx.y;
    float mn = INFINITY, mx = -INFINITY;
    if ((int)threadIdx.x < p.blocks) {
        const float* q = p.partials + ((long)v * NORM_BLOCKS + threadIdx.x) * 2;
        mn = q[0]; mx = q[1];
    }
    dm3d_block_minmax(mn, mx, red);
    const bool constant = !(mx > mn);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        p.minmax[2 * v] = mn; p.minmax[2 * v + 1] = mx;
        p.flag[v] = constant;
    }
    const float* x = p.x + (long)v * p.n;
    float* out = p.out + (long)v * p.n;
    const double lo = mn, range = (double)mx - (double)mn;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.n; i += (long)p.blocks * 256)
        out[i] = constant ? 0.0f : (float)(((double)fabsf(x[i]) - lo) / range);
}

// ---- augmentation ----------------------------------------------------------------------------------------------------------------------
struct AugArgs {
    const float* x; float* out;                    // [batch][d][plane]
    const float* mask; float* mask_out;            // [batch][d][mplane] or null
    int d;
    long plane, mplane;                            // h * w * c, h * w * cm
    int blocks;                                    // blocks a sample: min(ceil(d * plane / 1024), AUG_BLOCKS)
    int* flip; float* brightness; float* contrast; // [batch]
    double* partials;                              // [batch][AUG_BLOCKS]
};

// One lane per sample: counter (sample, 0, 0, STREAM_AUGMENT) under the key seed; words 0, 1, 2 of the block are the uniforms
// (float)word * 2^-32 of the flip, the brightness and the contrast.
__global__ __launch_bounds__(256) void aug_draw_kernel(int batch, int draw, uint64_t seed, float flip_chance, float b_lo, float b_hi, float c_lo,
                                                       float c_hi, int* flip, float* brightness, float* contrast) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= batch) return;
    uint32_t c[4] = {(uint32_t)b, 0u, 0u, STREAM_AUGMENT};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    const float u0 = (float)c[0] * 2.3283064365386963e-10f, u1 = (float)c[1] * 2.3283064365386963e-10f, u2 = (float)c[2] * 2.3283064365386963e-10f;
    if (draw & 1) flip[b] = u0 < flip_chance ? 0 : 1;
    if (draw & 2) brightness[b] = b_lo + (b_hi - b_lo) * u1;
    if (draw & 4) contrast[b] = c_lo + (c_hi - c_lo) * u2;
}

__device__ __forceinline__ double aug_bright(float x, double b) { return fmin(fmax((double)x * b, 0.0), 1.0); }

// Grid (blocks, batch): partials[b][block] = the float64 sum of clip(x * brightness, 0, 1) over the block's share, each lane in index
// order, the lanes by the fixed tree.
__global__ __launch_bounds__(256) void aug_sum_kernel(const AugArgs p) {
    __shared__ double red[4][1];
    const int b = blockIdx.y;
    const long n = (long)p.d * p.plane;
    const float* x = p.x + b * n;
    const double bright = p.brightness[b];
    double s[1] = {0.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)p.blocks * 256) s[0] += aug_bright(x[i], bright);
    dm3d_block_sum_f64<1>(s, red);
    if (threadIdx.x == 0) p.partials[(long)b * AUG_BLOCKS + blockIdx.x] = s[0];
}

// Grid (blocks, batch): every block adds the sample's partials in the one fixed order, then writes its share of
// clip((1 + contrast) * (clip(x * brightness, 0, 1) - mean) + mean, 0, 1) read at the flipped position, and of the flipped mask.
__global__ __launch_bounds__(256) void aug_apply_kernel(const AugArgs p) {
    __shared__ double red[4][1];
    const int b = blockIdx.y;
    const long n = (long)p.d * p.plane;
    double s[1] = {(int)threadIdx.x < p.blocks ? p.partials[(long)b * AUG_BLOCKS + threadIdx.x] : 0.0};
    dm3d_block_sum_f64<1>(s, red);
    const double mean = s[0] / (double)n, bright = p.brightness[b], gain = 1.0 + (double)p.contrast[b];
    const bool flip = p.flip[b] != 0;
    const float* x = p.x + b * n;
    float* out = p.out + b * n;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)p.blocks * 256) {
        const long z = i / p.plane, r = i - z * p.plane;
        const long src = flip ? (p.d - 1 - z) * p.plane + r : i;
        out[i] = (float)fmin(fmax(gain * (aug_bright(x[src], bright) - mean) + mean, 0.0), 1.0);
    }
    if (!p.mask) return;
    const long nm = (long)p.d * p.mplane;
    const float* mk = p.mask + b * nm;
    float* mo = p.mask_out + b * nm;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nm; i += (long)p.blocks * 256) {
        const long z = i / p.mplane, r = i - z * p.mplane;
        mo[i] = mk[flip ? (p.d - 1 - z) * p.mplane + r : i];
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------
int check_extents(const char* who, const char* what, int d, int h, int w) {
    DM3D_REQUIRE(d >= 1 && h >= 1 && w >= 1, "%s: %s d=%d h=%d w=%d (all at least 1)", who, what, d, h, w);
    return DM3D_OK;
}

template <int ORDER>
int launch_resample(const dm3d_resample_desc* d, const ResArgs& a, dim3 grid, hipStream_t st) {
    if (d->in_f64) hipLaunchKernelGGL((resample_kernel<ORDER, double>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((resample_kernel<ORDER, float>), grid, dim3(256), 0, st, a);
    return dm3d_launch_check("resample_kernel");
}

}  // namespace

extern "C" int dm3d_spline_filter(const dm3d_spline_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "spline_filter: null descriptor");
    DM3D_REQUIRE(d->x != nullptr && d->coeff != nullptr, "spline_filter: x and coeff must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->x, 4) && dm3d_aligned(d->coeff, 8), "spline_filter: x must be 4-byte and coeff 8-byte aligned");
    DM3D_REQUIRE(d->volumes >= 1, "spline_filter: volumes=%d (at least 1)", d->volumes);
    int rc = check_extents("spline_filter", "extent", d->d, d->h, d->w);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->d <= MAXE && d->h <= MAXE && d->w <= MAXE, "spline_filter: d=%d h=%d w=%d exceeds DM3D_SPLINE_MAX_EXTENT=%d per axis", d->d, d->h,
                 d->w, MAXE);
    int64_t blocks = 0;
    DM3D_REQUIRE(dm3d_line_grid_fault(d->volumes, d->d, d->h, d->w, &blocks) < 0, "spline_filter: %lld volumes exceed the grid", (long long)d->volumes);
    static std::atomic<bool> lds_set[64];
    const int dev = dm3d_dyn_lds((size_t)MAXE * LDT * sizeof(double), lds_set, "spline_filter", spline_pass_kernel<true>, spline_pass_kernel<false>);
    if (dev < 0) return dev;
    hipStream_t st = static_cast<hipStream_t>(stream);
    static const char* const names[3] = {"spline_pass_kernel (w)", "spline_pass_kernel (h)", "spline_pass_kernel (d)"};
    FilterArgs a{};
    a.x = d->x; a.c = d->coeff;
    a.z = sqrt(3.0) - 2.0;
    a.gain = (1.0 - a.z) * (1.0 - 1.0 / a.z);
    for (int axis = 0; axis < 3; ++axis) {                                      // w always (it makes the float64 copy); h and d where they filter
        blocks = dm3d_line_pass_fill(&a.line, axis, d->volumes, d->d, d->h, d->w);
        if (axis > 0 && a.line.n == 1) continue;
        a.first = axis == 0;
        a.zn1 = 1.0;
        for (int i = 0; i < a.line.n - 1; ++i) a.zn1 *= a.z;
        hipLaunchKernelGGL(axis == 0 ? spline_pass_kernel<true> : spline_pass_kernel<false>, dim3((unsigned)blocks), dim3(256),
                           (size_t)a.line.n * LDT * sizeof(double), st, a);
        if ((rc = dm3d_launch_check(names[axis])) != DM3D_OK) return rc;
    }
    return DM3D_OK;
}

extern "C" int dm3d_affine_resample(const dm3d_resample_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "affine_resample: null descriptor");
    DM3D_REQUIRE(d->src != nullptr && d->table != nullptr && d->out != nullptr, "affine_resample: src, table and out must be non-null");
    DM3D_REQUIRE(d->in_f64 == DM3D_RESAMPLE_F32 || d->in_f64 == DM3D_RESAMPLE_F64, "affine_resample: in_f64=%d (DM3D_RESAMPLE_F32 or DM3D_RESAMPLE_F64)",
                 d->in_f64);
    DM3D_REQUIRE(dm3d_aligned(d->src, d->in_f64 ? 8 : 4) && dm3d_aligned(d->table, 8) && dm3d_aligned(d->out, 4),
                 "affine_resample: src must be aligned to its element, table 8-byte and out 4-byte aligned");
    DM3D_REQUIRE(d->order == 0 || d->order == 1 || d->order == 3, "affine_resample: order=%d (0, 1 or 3; orders 2, 4 and 5 are not offered)", d->order);
    DM3D_REQUIRE(d->volumes >= 1 && d->volumes <= 65535, "affine_resample: volumes=%d (1 to 65535)", d->volumes);
    int rc = check_extents("affine_resample", "input", d->id, d->ih, d->iw);
    if (rc != DM3D_OK) return rc;
    if ((rc = check_extents("affine_resample", "output", d->od, d->oh, d->ow)) != DM3D_OK) return rc;
    DM3D_REQUIRE(isfinite(d->cval), "affine_resample: cval=%g (finite)", (double)d->cval);
    DM3D_REQUIRE((int64_t)d->id * d->ih * d->iw <= 0x7fffffffLL, "affine_resample: an input volume of %lld voxels (at most 2^31 - 1)",
                 (long long)d->id * d->ih * d->iw);
    ResArgs a{};
    a.in = d->src; a.table = d->table; a.out = d->out;
    a.id = d->id; a.ih = d->ih; a.iw = d->iw; a.od = d->od; a.oh = d->oh; a.ow = d->ow;
    a.tx = (d->ow + BX - 1) / BX; a.ty = (d->oh + BY - 1) / BY;
    a.cval = d->cval;
    const int64_t bricks = (int64_t)a.tx * a.ty * ((d->od + BZ - 1) / BZ);
    DM3D_REQUIRE(bricks <= 0x7fffffffLL, "affine_resample: %lld output bricks exceed the grid", (long long)bricks);
    const dim3 grid((unsigned)bricks, (unsigned)d->volumes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->order == 0) return launch_resample<0>(d, a, grid, st);
    if (d->order == 1) return launch_resample<1>(d, a, grid, st);
    return launch_resample<3>(d, a, grid, st);
}

extern "C" int dm3d_volume_normalize(const dm3d_normalize_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "volume_normalize: null descriptor");
    DM3D_REQUIRE(d->x != nullptr && d->out != nullptr && d->partials != nullptr && d->minmax != nullptr && d->flag != nullptr,
                 "volume_normalize: x, out, partials, minmax and flag must be non-null");
    DM3D_REQUIRE(dm3d_aligned(d->x, 4) && dm3d_aligned(d->out, 4) && dm3d_aligned(d->partials, 4) && dm3d_aligned(d->minmax, 4) && dm3d_aligned(d->flag, 4),
                 "volume_normalize: every buffer must be 4-byte aligned");
    DM3D_REQUIRE(d->volumes >= 1 && d->volumes <= 65535, "volume_normalize: volumes=%d (1 to 65535)", d->volumes);
    DM3D_REQUIRE(d->n >= 1, "volume_normalize: n=%lld (at least 1)", (long long)d->n);
    NormArgs a{};
    a.x = d->x; a.out = d->out; a.n = d->n; a.partials = d->partials; a.minmax = d->minmax; a.flag = d->flag;
    const int64_t blocks = (d->n + 1023) / 1024;
    a.blocks = (int)(blocks < NORM_BLOCKS ? blocks : NORM_BLOCKS);
    const dim3 grid((unsigned)a.blocks, (unsigned)d->volumes);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(norm_minmax_kernel, grid, dim3(256), 0, st, a);
    int rc = dm3d_launch_check("norm_minmax_kernel");
    if (rc != DM3D_OK) return rc;
    hipLaunchKernelGGL(norm_apply_kernel, grid, dim3(256), 0, st, a);
    return dm3d_launch_check("norm_apply_kernel");
}

extern "C" int dm3d_augment(const dm3d_augment_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "augment: null descriptor");
    DM3D_REQUIRE(d->x != nullptr && d->out != nullptr && d->flip != nullptr && d->brightness != nullptr && d->contrast != nullptr && d->partials != nullptr,
                 "augment: x, out, flip, brightness, contrast and partials must be non-null");
    DM3D_REQUIRE((d->mask == nullptr) == (d->mask_out == nullptr), "augment: mask and mask_out must be both given or both null");
    DM3D_REQUIRE(dm3d_aligned(d->x, 4) && dm3d_aligned(d->out, 4) && dm3d_aligned(d->mask, 4) && dm3d_aligned(d->mask_out, 4) && dm3d_aligned(d->flip, 4) &&
                     dm3d_aligned(d->brightness, 4) && dm3d_aligned(d->contrast, 4) && dm3d_aligned(d->partials, 8),
                 "augment: partials must be 8-byte and every other buffer 4-byte aligned");
    DM3D_REQUIRE(d->batch >= 1 && d->batch <= 65535, "augment: batch=%d (1 to 65535)", d->batch);
    int rc = check_extents("augment", "extent", d->d, d->h, d->w);
    if (rc != DM3D_OK) return rc;
    DM3D_REQUIRE(d->c >= 1, "augment: c=%d (at least 1)", d->c);
    DM3D_REQUIRE(d->mask == nullptr || d->cm >= 1, "augment: cm=%d (at least 1 with a mask)", d->cm);
    DM3D_REQUIRE(d->draw >= 0 && d->draw <= 7, "augment: draw=%d (bits 1, 2, 4)", d->draw);
    {                                                                           // a flipped read is not in place: no output may share a byte with an input
        const uint64_t vox = (uint64_t)d->batch * d->d * d->h * d->w, xb = vox * d->c * 4, mb = d->mask ? vox * d->cm * 4 : 0;
        DM3D_REQUIRE(!dm3d_ranges_overlap(d->x, xb, d->out, xb), "augment: out must not overlap x (a flipped read is not in place)");
        DM3D_REQUIRE(!dm3d_ranges_overlap(d->mask, mb, d->mask_out, mb), "augment: mask_out must not overlap mask (a flipped read is not in place)");
        DM3D_REQUIRE(!dm3d_ranges_overlap(d->mask, mb, d->out, xb), "augment: out must not overlap mask");
        DM3D_REQUIRE(!dm3d_ranges_overlap(d->x, xb, d->mask_out, mb), "augment: mask_out must not overlap x");
        DM3D_REQUIRE(!dm3d_ranges_overlap(d->out, xb, d->mask_out, mb), "augment: out and mask_out must not overlap");
    }
    if (d->draw) {
        DM3D_REQUIRE(d->flip_chance >= 0.0f && d->flip_chance <= 1.0f, "augment: flip_chance=%g (in [0, 1])", (double)d->flip_chance);
        DM3D_REQUIRE(isfinite(d->brightness_lo) && isfinite(d->brightness_hi) && d->brightness_lo <= d->brightness_hi,
                     "augment: brightness range (%g, %g) (finite, ascending)", (double)d->brightness_lo, (double)d->brightness_hi);
        DM3D_REQUIRE(isfinite(d->contrast_lo) && isfinite(d->contrast_hi) && d->contrast_lo <= d->contrast_hi,
                     "augment: contrast range (%g, %g) (finite, ascending)", (double)d->contrast_lo, (double)d->contrast_hi);
    }
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (d->draw) {
        hipLaunchKernelGGL(aug_draw_kernel, dim3((unsigned)((d->batch + 255) / 256)), dim3(256), 0, st, (int)d->batch, (int)d->draw, (uint64_t)d->seed,
                           d->flip_chance, d->brightness_lo, d->brightness_hi, d->contrast_lo, d->contrast_hi, d->flip, d->brightness, d->contrast);
        if ((rc = dm3d_launch_check("aug_draw_kernel")) != DM3D_OK) return rc;
    }
    AugArgs a{};
    a.x = d->x; a.out = d->out; a.mask = d->mask; a.mask_out = d->mask_out;
    a.d = d->d; a.plane = (long)d->h * d->w * d->c; a.mplane = d->mask ? (long)d->h * d->w * d->cm : 0;
    a.flip = d->flip; a.brightness = d->brightness; a.contrast = d->contrast; a.partials = d->partials;
    const int64_t blocks = ((int64_t)d->d * a.plane + 1023) / 1024;
    a.blocks = (int)(blocks < AUG_BLOCKS ? blocks : AUG_BLOCKS);
    const dim3 grid((unsigned)a.blocks, (unsigned)d->batch);
    hipLaunchKernelGGL(aug_sum_kernel, grid, dim3(256), 0, st, a);
    if ((rc = dm3d_launch_check("aug_sum_kernel")) != DM3D_OK) return rc;
    hipLaunchKernelGGL(aug_apply_kernel, grid, dim3(256), 0, st, a);
    return dm3d_launch_check("aug_apply_kernel");
}
