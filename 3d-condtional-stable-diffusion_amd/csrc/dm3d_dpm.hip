// dm3d_dpm.hip — the DPM-Solver++(2M) update (Lu et al. 2022, "DPM-Solver++", Algorithm 2): a second-order multistep solver of the
// sampling ODE in the data-prediction form.  Every per-step constant comes from a coefficient table the host writes once per chain
// (include/dm3d.h, dm3d_dpm_desc), so first-order rows (the DDIM eta = 0 step), second-order rows and the step to the clean sample
// share one kernel.  A pure HBM stream like ddim_kernel: 16 B per lane, read x, eps and (second-order rows only) the previous x0
// estimate, write x and this step's x0 estimate.  No noise term: no Philox.
// The body and its arguments are dm3d_update.h's, shared with the SDE form (dm3d_dpm_sde.hip); these two kernels are its SDE = false
// instantiations.
#include "dm3d_update.h"

namespace {

// FRAME: `eps` holds the network's output in its own frame.  Two kernels, chosen by the host, so that the eps kernel is the one it always was.
__global__ __launch_bounds__(256) void dpm_kernel(const dm3d_dpm_args p) { dm3d_dpm_block<false, false>(p); }
__global__ __launch_bounds__(256) void dpm_frame_kernel(const dm3d_dpm_args p) { dm3d_dpm_block<true, false>(p); }

}  // namespace

extern "C" int dm3d_dpm_update_frame(const dm3d_dpm_desc* d, const float* frame, void* stream) {
    DM3D_REQUIRE(d != nullptr, "dpm: null descriptor");
    dm3d_dpm_args a{};
    if (int rc = dm3d_dpm_args_of("dpm", d, frame, true, "", nullptr, a)) return rc;
    hipLaunchKernelGGL(frame ? dpm_frame_kernel : dpm_kernel, dm3d_stream_grid(a.per4, d->batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check(frame ? "dpm_frame_kernel" : "dpm_kernel");
}

extern "C" int dm3d_dpm_update(const dm3d_dpm_desc* d, void* stream) { return dm3d_dpm_update_frame(d, nullptr, stream); }
