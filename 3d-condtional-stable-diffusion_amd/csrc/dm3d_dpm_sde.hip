// dm3d_dpm_sde.hip — the stochastic DPM-Solver++(2M) update (Lu et al. 2022, "DPM-Solver++", the SDE form of the appendix; k-diffusion's
// dpmpp_2m_sde): dpm_kernel's multistep update of the data-prediction form plus one noise term per step.  Every per-step constant comes
// from a coefficient table the host writes once per chain (include/dm3d.h, dm3d_dpm_sde_desc), so first-order rows, second-order rows,
// the step to the clean sample and rows without noise (eta = 0: dpm_kernel's result bitwise) share one kernel.  A pure HBM stream like
// dpm_kernel: 16 B per lane, read x, eps and (second-order rows only) the previous x0 estimate, write x and this step's x0 estimate;
// z is an injected tensor or ddim_kernel's in-kernel Philox draw under a stream constant of this kernel's own.
// The body and its arguments are dm3d_update.h's, shared with dpm_kernel; these two kernels are its SDE = true instantiations.
#include "dm3d_update.h"

namespace {

// FRAME: `eps` holds the network's output in its own frame.  Two kernels, chosen by the host, as dpm_kernel / dpm_frame_kernel.
__global__ __launch_bounds__(256) void dpm_sde_kernel(const dm3d_dpm_sde_args p) { dm3d_dpm_block<false, true>(p); }
__global__ __launch_bounds__(256) void dpm_sde_frame_kernel(const dm3d_dpm_sde_args p) { dm3d_dpm_block<true, true>(p); }

}  // namespace

extern "C" int dm3d_dpm_sde_update_frame(const dm3d_dpm_sde_desc* d, const float* frame, void* stream) {
    DM3D_REQUIRE(d != nullptr, "dpm_sde: null descriptor");
    dm3d_dpm_sde_args a{};
    if (int rc = dm3d_dpm_args_of("dpm_sde", d, frame, d->tau != nullptr, "/tau", d->noise, a)) return rc;
    a.noise = d->noise; a.tau = d->tau; a.seed = d->seed; a.seed_dev = d->seed_dev;
    hipLaunchKernelGGL(frame ? dpm_sde_frame_kernel : dpm_sde_kernel, dm3d_stream_grid(a.per4, d->batch), dim3(256), 0,
                       static_cast<hipStream_t>(stream), a);
    return dm3d_launch_check(frame ? "dpm_sde_frame_kernel" : "dpm_sde_kernel");
}

extern "C" int dm3d_dpm_sde_update(const dm3d_dpm_sde_desc* d, void* stream) { return dm3d_dpm_sde_update_frame(d, nullptr, stream); }
