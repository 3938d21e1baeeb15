// dm3d_interp.h — the interpolation the resampling kernels share (dm3d_resample.hip: resample_kernel; dm3d_deform.hip: warp_kernel): the
// output brick, scipy.ndimage's tap rules at orders 0, 1 and 3 and the tap sum, in scipy's operation order.  A kernel forms its float64
// coordinate and hands it over; the inside test, the taps, the order of the sum and the float32 store are these.
#pragma once
#include "dm3d_common.h"
#include <math.h>

constexpr int DM3D_BRICK_X = 16, DM3D_BRICK_Y = 4, DM3D_BRICK_Z = 4;    // the output brick of a resample block (x, y, z): 256 lanes

// This lane's output voxel (z, y, x) in the grid of bricks (tx, ty bricks along x and y), and whether it exists.
__device__ __forceinline__ bool dm3d_brick_voxel(int tx, int ty, int od, int oh, int ow, int& oz, int& oy, int& ox) {
    const int bx = blockIdx.x % tx, by = (blockIdx.x / tx) % ty, bz = blockIdx.x / (tx * ty);
    ox = bx * DM3D_BRICK_X + (threadIdx.x & (DM3D_BRICK_X - 1));
    oy = by * DM3D_BRICK_Y + ((threadIdx.x / DM3D_BRICK_X) & (DM3D_BRICK_Y - 1));
    oz = bz * DM3D_BRICK_Z + threadIdx.x / (DM3D_BRICK_X * DM3D_BRICK_Y);
    return ox < ow && oy < oh && oz < od;
}

// scipy's mirror of a tap index: period 2n - 2, no repeated edge
__device__ __forceinline__ int mirror_tap(int i, int n) {
    if (n == 1) return 0;
    const int period = 2 * n - 2;
    i %= period;
    if (i < 0) i += period;
    return i < n ? i : period - i;
}

// The taps of one axis for an inside coordinate c: their (mirrored) indices and weights, as scipy forms them.
template <int ORDER>
__device__ __forceinline__ void axis_taps(double c, int n, int (&idx)[ORDER + 1], double (&w)[ORDER + 1]) {
    if (ORDER == 0) {
        idx[0] = (int)floor(c + 0.5);
        w[0] = 1.0;
        return;
    }
    const double fl = floor(c), x = c - fl;
    const int start = (int)fl - ORDER / 2;
#pragma unroll
    for (int k = 0; k <= ORDER; ++k) idx[k] = mirror_tap(start + k, n);
    if (ORDER == 1) {
        w[0] = 1.0 - x;
        w[1] = 1.0 - w[0];
    } else {
        const double y = 1.0 - x;
        w[1] = (x * x * (x - 2.0) * 3.0 + 4.0) / 6.0;
        w[2] = (y * y * (y - 2.0) * 3.0 + 4.0) / 6.0;
        w[0] = y * y * y / 6.0;
        w[ORDER] = ((1.0 - w[0]) - w[1]) - w[2];
    }
}

// *out = the volume `in` [id][ih][iw] at the coordinate c: the sum over the taps, axis 0 outermost, of ((in * w0) * w1) * w2 in float64,
// stored as float32; a coordinate outside [0, n - 1] on any axis (or not a number) gives cval.  No read leaves the volume.
template <int ORDER, typename T>
__device__ __forceinline__ void dm3d_interp_store(const T* in, int id, int ih, int iw, const double (&c)[3], float cval, float* out) {
    const int n[3] = {id, ih, iw};
    bool inside = true;
#pragma unroll
    for (int h = 0; h < 3; ++h) inside = inside && c[h] >= 0.0 && c[h] <= (double)(n[h] - 1);
    if (!inside) {
        *out = cval;
        return;
    }
    int iz[ORDER + 1], iy[ORDER + 1], ix[ORDER + 1];
    double wz[ORDER + 1], wy[ORDER + 1], wx[ORDER + 1];
    axis_taps<ORDER>(c[0], n[0], iz, wz);
    axis_taps<ORDER>(c[1], n[1], iy, wy);
    axis_taps<ORDER>(c[2], n[2], ix, wx);
    double t = 0.0;
#pragma unroll
    for (int i = 0; i <= ORDER; ++i)
#pragma unroll
        for (int j = 0; j <= ORDER; ++j) {
            const T* row = in + ((long)iz[i] * ih + iy[j]) * iw;
#pragma unroll
            for (int k = 0; k <= ORDER; ++k) t += (((double)row[ix[k]] * wz[i]) * wy[j]) * wx[k];
        }
    *out = (float)t;
}
