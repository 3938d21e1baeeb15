// dm3d_objective.hip — what the network's output means (include/dm3d.h, dm3d_pred_desc / dm3d_loss_desc): the conversion of a v- or
// x0-prediction to the eps every solver reads, and the training loss against the matching target with a per-sample weight (min-SNR).
// Two pure HBM streams like q_sample_kernel, 16 B per lane, every float32 operation rounded on its own.  The loss is summed in float64
// in a fixed order: the block by dm3d_block_sum_f64, blocks through a partials buffer in block order by a second one-block launch (no
// atomics): runs repeat bitwise, and the caller gets one loss per sample.
#include "dm3d_common.h"

namespace {

constexpr int PARTS = DM3D_LOSS_PARTIAL_BLOCKS;

// eps = c_p*pred + c_x*x with (c_p, c_x) = table[clamp(t_idx[b])]: mul, mul, add.  dst may be pred (in place) or x: a lane reads its
// own float4 of both before it stores.
__global__ __launch_bounds__(256) void pred_to_eps_kernel(const float* pred, const float* x, float* dst, const float* __restrict__ table,
                                                          const int* __restrict__ t_idx, int timesteps, long per4) {
    const int b = blockIdx.y;
    const int t = min(max(t_idx[b], 0), timesteps - 1);
    const float cp = table[2 * t], cx = table[2 * t + 1];
    const long base = (long)b * per4;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per4; i += (long)gridDim.x * 256) {
        const f32x4 p = reinterpret_cast<const f32x4*>(pred)[base + i], xv = reinterpret_cast<const f32x4*>(x)[base + i];
        f32x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = __fadd_rn(__fmul_rn(cp, p[e]), __fmul_rn(cx, xv[e]));
        reinterpret_cast<f32x4*>(dst)[base + i] = o;
    }
}

// d = pred - (a_z*noise + a_0*x0); dpred = d*scale; the block's float64 sum of d^2 goes to partials[b][blockIdx.x].
__global__ __launch_bounds__(256) void objective_loss_kernel(const float* __restrict__ pred, const float* __restrict__ noise,
                                                             const float* __restrict__ x0, const float* __restrict__ coef, double inv,
                                                             float* __restrict__ dpred, double* __restrict__ partials, long per4) {
    __shared__ double red[4][1];
    const int b = blockIdx.y;
    const float az = coef[4 * b], a0 = coef[4 * b + 1];
    const float scale = (float)(2.0 * inv * (double)coef[4 * b + 2]);
    const long base = (long)b * per4;
    double s[1] = {0.0};
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < per4; i += (long)gridDim.x * 256) {
        const f32x4 p = reinterpret_cast<const f32x4*>(pred)[base + i], z = reinterpret_cast<const f32x4*>(noise)[base + i];
        const f32x4 c = reinterpret_cast<const f32x4*>(x0)[base + i];
        f32x4 g;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = __fsub_rn(p[e], __fadd_rn(__fmul_rn(az, z[e]), __fmul_rn(a0, c[e])));
            s[0] += (double)d * (double)d;
            g[e] = __fmul_rn(d, scale);
        }
        if (dpred) reinterpret_cast<f32x4*>(dpred)[base + i] = g;
    }
    dm3d_block_sum_f64(s, red);
    if (threadIdx.x == 0) partials[(long)b * PARTS + blockIdx.x] = s[0];
}

// One block: loss_rows[b] = w*inv*(partials[b][0] + ... + partials[b][nblocks-1]), then loss[0] = loss_rows[0] + ... in index order.
__global__ __launch_bounds__(256) void objective_sum_kernel(const double* __restrict__ partials, const float* __restrict__ coef, double inv,
                                                            int nblocks, int batch, double* __restrict__ loss_rows, double* __restrict__ loss) {
    for (int b = threadIdx.x; b < batch; b += 256) {
        double s = 0.0;
        for (int k = 0; k < nblocks; ++k) s += partials[(long)b * PARTS + k];
        loss_rows[b] = (double)coef[4 * b + 2] * inv * s;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int b = 0; b < batch; ++b) s += loss_rows[b];
        loss[0] = s;
    }
}

// Two byte ranges of `bytes` each that share bytes: at all, or without being the same range (in place is allowed).
bool overlap(const void* a, const void* b, uint64_t bytes) { return dm3d_ranges_overlap(a, bytes, b, bytes); }
bool partial_overlap(const void* a, const void* b, uint64_t bytes) { return a != b && overlap(a, b, bytes); }

}  // namespace

extern "C" int dm3d_pred_to_eps(const dm3d_pred_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "pred_to_eps: null descriptor");
    DM3D_REQUIRE(d->pred && d->x && d->table && d->t_idx, "pred_to_eps: pred/x/table/t_idx must be non-null");
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0,
                 "pred_to_eps: batch=%d per_sample=%lld (batch in [1, 65535], per_sample a positive multiple of 4)", d->batch,
                 (long long)d->per_sample);
    DM3D_REQUIRE(d->timesteps > 0, "pred_to_eps: timesteps=%d must be positive", d->timesteps);
    DM3D_REQUIRE(dm3d_aligned16(d->pred) && dm3d_aligned16(d->x) && dm3d_aligned16(d->out), "pred_to_eps: pred/x/out must be 16-byte aligned");
    DM3D_REQUIRE((reinterpret_cast<uintptr_t>(d->table) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d->t_idx) & 3u) == 0,
                 "pred_to_eps: table / t_idx are not aligned to their element");
    const uint64_t bytes = (uint64_t)d->batch * (uint64_t)d->per_sample * sizeof(float);
    DM3D_REQUIRE(!d->out || (!partial_overlap(d->out, d->pred, bytes) && !partial_overlap(d->out, d->x, bytes)),
                 "pred_to_eps: out overlaps pred or x partially (it may be either of them, or apart from both)");
    DM3D_REQUIRE(!partial_overlap(d->pred, d->x, bytes) || d->out, "pred_to_eps: in place, pred overlaps x partially");
    const long per4 = d->per_sample / 4, blocks = (per4 + 255) / 256;
    dim3 grid((unsigned)(blocks > PARTS ? PARTS : blocks), (unsigned)d->batch);
    hipLaunchKernelGGL(pred_to_eps_kernel, grid, dim3(256), 0, static_cast<hipStream_t>(stream), d->pred, d->x, d->out ? d->out : d->pred,
                       d->table, d->t_idx, d->timesteps, per4);
    return dm3d_launch_check("pred_to_eps_kernel");
}

extern "C" int dm3d_objective_loss_grad(const dm3d_loss_desc* d, void* stream) {
    DM3D_REQUIRE(d != nullptr, "objective_loss_grad: null descriptor");
    DM3D_REQUIRE(d->pred && d->noise && d->x0 && d->coef && d->partials && d->loss_rows && d->loss,
                 "objective_loss_grad: pred/noise/x0/coef/partials/loss_rows/loss must be non-null");
    DM3D_REQUIRE(d->batch > 0 && d->batch <= 65535 && d->per_sample > 0 && d->per_sample % 4 == 0,
                 "objective_loss_grad: batch=%d per_sample=%lld (batch in [1, 65535], per_sample a positive multiple of 4)", d->batch,
                 (long long)d->per_sample);
    DM3D_REQUIRE(d->inv_divisor == d->inv_divisor && d->inv_divisor - d->inv_divisor == 0.0, "objective_loss_grad: inv_divisor must be finite");
    DM3D_REQUIRE(dm3d_aligned16(d->pred) && dm3d_aligned16(d->noise) && dm3d_aligned16(d->x0) && dm3d_aligned16(d->dpred) &&
                 dm3d_aligned16(d->coef), "objective_loss_grad: pred/noise/x0/dpred/coef must be 16-byte aligned");
    DM3D_REQUIRE((reinterpret_cast<uintptr_t>(d->partials) & 7u) == 0 && (reinterpret_cast<uintptr_t>(d->loss_rows) & 7u) == 0 &&
                 (reinterpret_cast<uintptr_t>(d->loss) & 7u) == 0, "objective_loss_grad: partials/loss_rows/loss must be 8-byte aligned");
    const uint64_t bytes = (uint64_t)d->batch * (uint64_t)d->per_sample * sizeof(float);
    DM3D_REQUIRE(!d->dpred || (!overlap(d->dpred, d->pred, bytes) && !overlap(d->dpred, d->noise, bytes) && !overlap(d->dpred, d->x0, bytes)),
                 "objective_loss_grad: dpred overlaps pred, noise or x0");
    const long per4 = d->per_sample / 4, blocks = (per4 + 255) / 256;
    const int nblocks = (int)(blocks > PARTS ? PARTS : blocks);
    hipStream_t st = static_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(objective_loss_kernel, dim3((unsigned)nblocks, (unsigned)d->batch), dim3(256), 0, st, d->pred, d->noise, d->x0, d->coef,
                       d->inv_divisor, d->dpred, d->partials, per4);
    int rc = dm3d_launch_check("objective_loss_kernel");
    if (rc != DM3D_OK) return rc;
    hipLaunchKernelGGL(objective_sum_kernel, dim3(1), dim3(256), 0, st, d->partials, d->coef, d->inv_divisor, nblocks, d->batch,
                       d->loss_rows, d->loss);
    return dm3d_launch_check("objective_sum_kernel");
}
