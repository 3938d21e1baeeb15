// dm3d_edit.hip — the known-latent step of inpainting and image-to-image editing: forward-noising of a known latent x0 to a level
// (q_sample, conditional_dm3d.py:484-491's order) and RePaint's replacement step (Lugmayr et al. 2022), x <- w known_t + (1-w) x,
// with a per-voxel keep weight w broadcast over channels.  Every per-step constant comes from a level table the host writes once
// per chain (include/dm3d.h, dm3d_edit_desc); the row of each sample is read from device memory, so the step is graph-capturable.
// A pure HBM stream like ddim_kernel: 16 B per lane; lanes whose weights are all 0 read nothing but w and write nothing.
#include "dm3d_common.h"
#include "dm3d_philox.h"

namespace {

struct EditArgs {
    float* x; const float* x0; const float* w; const float* noise; float* out;
    long per4;                                     // float4 per sample
    int channels; long vox;                        // w holds vox = per_sample / channels weights per sample
    const float* levels; int rows; const int* pos;
    uint64_t seed; const uint64_t* seed_dev; int mode;
};

__global__ __launch_bounds__(256) void edit_kernel(const EditArgs p) {
    const int b = blockIdx.y;
    const int r = min(max(p.pos[b], 0), p.rows - 1);
    const f32x4 lv = reinterpret_cast<const f32x4*>(p.levels)[r];           // sqrt(a'), sqrt(1-a'), level, -
    const float sq = lv[0], sq1 = lv[1];
    const bool clean = sq1 == 0.f;                                           // a' = 1: known_t = x0, no draw
    const uint32_t level = (uint32_t)(int)lv[2];
    const uint64_t seed = p.seed_dev ? *p.seed_dev : p.seed;
    const long base = (long)b * p.per4;
    const bool vec = (p.channels & 3) == 0;                                  // the 4 elements of a lane share one voxel
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < p.per4; i += (long)gridDim.x * 256) {
        f32x4 w = {1.f, 1.f, 1.f, 1.f};
        if (p.mode == 1) {
            const float* wb = p.w + (long)b * p.vox;
            if (vec) {
                const float v = wb[4 * i / p.channels];
                w = f32x4{v, v, v, v};
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) w[k] = wb[(4 * i + k) / p.channels];
            }
            if (w[0] == 0.f && w[1] == 0.f && w[2] == 0.f && w[3] == 0.f) continue;     // regenerated: x untouched
        }
        const f32x4 x0 = reinterpret_cast<const f32x4*>(p.x0)[base + i];
        f32x4 kn = x0;
        if (!clean) {
            const f32x4 z = p.noise ? reinterpret_cast<const f32x4*>(p.noise)[base + i]
                                    : philox_normal4((uint64_t)(base + i), level, 0xed17u, seed);
#pragma unroll
            for (int k = 0; k < 4; ++k) kn[k] = __fadd_rn(__fmul_rn(sq, x0[k]), __fmul_rn(sq1, z[k]));
        }
        if (p.mode == 0) {
            reinterpret_cast<f32x4*>(p.out)[base + i] = kn;
            continue;
        }
        if (!(w[0] == 1.f && w[1] == 1.f && w[2] == 1.f && w[3] == 1.f)) {
            const f32x4 x = reinterpret_cast<const f32x4*>(p.x)[base + i];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (w[k] == 0.f) kn[k] = x[k];
                else if (w[k] != 1.f) kn[k] = __fadd_rn(__fmul_rn(w[k], kn[k]), __fmul_rn(__fsub_rn(1.0f, w[k]), x[k]));
            }
        }
        reinterpret_cast<f32x4*>(p.x)[base + i] = kn;
    }
}

}  // namespace

extern "C" int dm3d_edit_update(const dm3d_edit_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "edit: null descriptor");
    DM3D_REQUIRE(d->x0 && d->levels && d->pos, "edit: x0/levels/pos must be non-null");
    DM3D_REQUIRE(d->mode == 0 || d->mode == 1, "edit: mode %d not in {0,1}", d->mode);
    DM3D_REQUIRE(d->mode == 1 || d->out, "edit: mode 0 needs out");
    DM3D_REQUIRE(d->mode == 0 || (d->x && d->w), "edit: mode 1 needs x and w");
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0,
                 "edit: batch=%d per_sample=%lld (batch in [1, 65535], per_sample a positive multiple of 4)", d->batch,
                 (long long)d->per_sample);
    DM3D_REQUIRE(d->channels > 0 && d->per_sample % d->channels == 0, "edit: channels=%d does not divide per_sample=%lld",
                 d->channels, (long long)d->per_sample);
    DM3D_REQUIRE(d->rows > 0, "edit: rows=%d", d->rows);
    DM3D_REQUIRE(dm3d_aligned16(d->x) && dm3d_aligned16(d->x0) && dm3d_aligned16(d->noise) && dm3d_aligned16(d->out) &&
                 dm3d_aligned16(d->levels), "edit: pointers must be 16-byte aligned");
    EditArgs a{};
    a.x = d->x; a.x0 = d->x0; a.w = d->w; a.noise = d->noise; a.out = d->out; a.per4 = d->per_sample / 4;
    a.channels = d->channels; a.vox = d->per_sample / d->channels;
    a.levels = d->levels; a.rows = d->rows; a.pos = d->pos;
    a.seed = d->seed; a.seed_dev = d->seed_dev; a.mode = d->mode;
    hipLaunchKernelGGL(edit_kernel, dm3d_stream_grid(a.per4, d->batch), dim3(256), 0, static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check("edit_kernel");
}
