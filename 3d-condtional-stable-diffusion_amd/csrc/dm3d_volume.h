// dm3d_volume.h — what the volume kernels share (dm3d_metrics, dm3d_msssim, dm3d_mask, dm3d_ccl, dm3d_resample, dm3d_deform): the host checks of an
// NDHWC channel window and of a mask volume, the line-pass tiler of the separable passes (the distance transform's and the spline
// prefilter's), and the block min / max.  A new volume kernel starts here.
#pragma once
#include "dm3d_common.h"

// ---- host checks: the words are part of the ABI's behaviour, callers and tests read them ---------------------------------------------------
// The channel window [c0, c0 + nc) of tensor `name` ("x" or "y") with c channels.
static inline int dm3d_check_window(const char* who, const char* name, int c0, int nc, int c) {
    DM3D_REQUIRE(c0 >= 0 && c >= 1 && (int64_t)c0 + nc <= c, "%s: channels [%d, %d + %d) are outside %s's c%s=%d", who, c0, c0, nc, name, name, c);
    return DM3D_OK;
}
// The volumes of a mask entry: batch * nc of them ride grid.y, no axis is longer than what a kernel stages (`max_name` is the macro's name).
static inline int dm3d_check_volume(const char* who, int batch, int d, int h, int w, int nc, int max_extent, const char* max_name) {
    DM3D_REQUIRE(batch >= 1, "%s: batch=%d (at least 1)", who, batch);
    DM3D_REQUIRE(d >= 1 && h >= 1 && w >= 1, "%s: d=%d h=%d w=%d (all at least 1)", who, d, h, w);
    DM3D_REQUIRE(d <= max_extent && h <= max_extent && w <= max_extent, "%s: d=%d h=%d w=%d exceeds %s=%d per axis", who, d, h, w, max_name, max_extent);
    DM3D_REQUIRE(nc >= 1, "%s: nc=%d (at least 1)", who, nc);
    DM3D_REQUIRE((int64_t)batch * nc <= 65535, "%s: batch * nc = %lld (at most 65535)", who, (long long)batch * nc);
    return DM3D_OK;
}

// ---- the line pass: one separable pass along w, h or d of [volumes][D][H][W], in place ------------------------------------------------------
// A block stages LANES neighbouring lines of one group in LDS as [n][LDT] (the pad keeps the transposed stores of the w pass off one
// bank), works on them there and writes them back; the kernel keeps its element type and its step, the tiling is this one.
constexpr int DM3D_LINE_LANES = 32, DM3D_LINE_LDT = DM3D_LINE_LANES + 1;
static_assert(DM3D_LINE_LANES == DM3D_EDT_LANES && DM3D_LINE_LANES == DM3D_SPLINE_LANES, "the public macros name this tiler's lane count");

struct dm3d_line_pass {
    long gs, ls, cs;                               // strides of a group of lines, of neighbouring lines, along a line
    long lanes;                                    // lines of a group
    int tiles;                                     // blocks of a group: ceil(lanes / LANES)
    int n;                                         // line length
};
static const char* const dm3d_line_axis[3] = {"w", "h", "d"};
// Pass `axis` (0: w, every row of the tensor is a line; 1: h, a group is one plane, its lines the w positions; 2: d, a group is one
// volume, its lines the h * w positions of a plane).  Returns the blocks of the launch, which the caller holds against the grid limit.
static inline int64_t dm3d_line_pass_fill(dm3d_line_pass* p, int axis, int64_t volumes, int64_t D, int64_t H, int64_t W) {
    int64_t groups;
    if (axis == 0) { p->gs = 0; p->ls = W; p->cs = 1; p->lanes = volumes * D * H; p->n = (int)W; groups = 1; }
    else if (axis == 1) { p->gs = H * W; p->ls = 1; p->cs = W; p->lanes = W; p->n = (int)H; groups = volumes * D; }
    else { p->gs = D * H * W; p->ls = 1; p->cs = H * W; p->lanes = H * W; p->n = (int)D; groups = volumes; }
    p->tiles = (int)((p->lanes + DM3D_LINE_LANES - 1) / DM3D_LINE_LANES);
    return groups * ((p->lanes + DM3D_LINE_LANES - 1) / DM3D_LINE_LANES);
}
// The first axis whose pass would not fit the grid, with its block count, or -1.
static inline int dm3d_line_grid_fault(int64_t volumes, int64_t D, int64_t H, int64_t W, int64_t* blocks) {
    dm3d_line_pass p;
    for (int axis = 0; axis < 3; ++axis)
        if ((*blocks = dm3d_line_pass_fill(&p, axis, volumes, D, H, W)) > 0x7fffffffLL) return axis;
    return -1;
}

// This block's lines: the offset of line 0 at position 0, and how many of the LANES lines exist.
struct dm3d_line_block { long base; int nl; };
__device__ __forceinline__ dm3d_line_block dm3d_line_block_of(const dm3d_line_pass& p) {
    const long group = blockIdx.x / p.tiles, lane0 = (long)(blockIdx.x % p.tiles) * DM3D_LINE_LANES;
    const int nl = p.lanes - lane0 < DM3D_LINE_LANES ? (int)(p.lanes - lane0) : DM3D_LINE_LANES;
    return {group * p.gs + lane0 * p.ls, nl};
}
// f(lds_index, memory_offset, lane_is_live) over the [n][LDT] image, by all 256 lanes in the order of memory: ALONG (the w pass, a line
// is contiguous) walks a line with consecutive lanes, the h and d passes walk the LANES neighbours.  A dead lane's offset is no line's.
template <bool ALONG, class F>
__device__ __forceinline__ void dm3d_line_walk(const dm3d_line_pass& p, const dm3d_line_block& b, F f) {
    const int n = p.n;
    for (int i = threadIdx.x; i < n * DM3D_LINE_LANES; i += 256) {
        const int j = ALONG ? i % n : i / DM3D_LINE_LANES, l = ALONG ? i / n : i % DM3D_LINE_LANES;
        f(j * DM3D_LINE_LDT + l, b.base + l * p.ls + j * p.cs, l < b.nl);
    }
}

// ---- min and max of a block of 256 lanes, exact whatever the order: _put folds each wave's pair into red, _get reads the block's after a
// barrier; a kernel with a barrier of its own in between (a dm3d_block_sum_f64) calls the two halves, every other one dm3d_block_minmax ----
__device__ __forceinline__ void dm3d_block_minmax_put(float& mn, float& mx, float (&red)[4][2]) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = fminf(mn, __shfl_xor(mn, off, 64));
        mx = fmaxf(mx, __shfl_xor(mx, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { red[threadIdx.x >> 6][0] = mn; red[threadIdx.x >> 6][1] = mx; }
}
__device__ __forceinline__ void dm3d_block_minmax_get(float& mn, float& mx, const float (&red)[4][2]) {
    mn = fminf(fminf(red[0][0], red[1][0]), fminf(red[2][0], red[3][0]));
    mx = fmaxf(fmaxf(red[0][1], red[1][1]), fmaxf(red[2][1], red[3][1]));
}
__device__ __forceinline__ void dm3d_block_minmax(float& mn, float& mx, float (&red)[4][2]) {
    dm3d_block_minmax_put(mn, mx, red);
    __syncthreads();
    dm3d_block_minmax_get(mn, mx, red);
}
