// The instant-ngp loop's per-iteration log sums (include/xrnerf_mi355_ngprun.h).
//   k_ngp_log_add      one iteration's loss and psnr times n_rays, added into the double sums of a log window (xr_optim.hip's layout) from
//                      the two fp32 scalars the step leaves.  Launched by the native loop behind every step (xr_step.hip,
//                      xr_ngp_loop_run_logged) and by the per-iteration path behind its train_step, so a logger's interval average is one
//                      read per interval whichever path ran the iterations.  Thread 0 owns the loss slot, thread 1 the psnr slot: plain
//                      loads and stores, the stream's order is the summation order.
// The psnr is formed in double from the fp32 sum: -10 log10(sum / (3 n)).  Compiled without fused multiply-adds, so the host build of this
// source (tests/hip_emu) rounds the products and sums alike.
#include "xr_common.h"
#include "../../include/xrnerf_mi355_ngprun.h"

static __global__ __launch_bounds__(XR_WAVE) void k_ngp_log_add(const float* __restrict__ loss_mse, uint32_t n_rays, double* __restrict__ window,
                                                                uint32_t slot_loss, uint32_t slot_psnr) {
    const uint32_t t = threadIdx.x;
    if (t > 1) return;
    const double n = (double)n_rays;
    double v;
    uint32_t slot;
    if (t == 0) {
        v = (double)loss_mse[0];
        slot = slot_loss;
    } else {
        v = -10.0 * log10((double)loss_mse[1] / (3.0 * n));
        slot = slot_psnr;
    }
    window[slot] += v * n;                                     // loss: an exact product (24 + 29 bits)
    window[XR_LOG_WINDOW_SLOTS + slot] += n;
}

extern "C" int xr_ngp_log_add(const float* loss_mse, uint32_t n_rays, double* window, uint32_t slot_loss, uint32_t slot_psnr, void* stream_) {
    XR_REQUIRE(loss_mse && window, "null pointer");
    XR_REQUIRE(((uintptr_t)loss_mse & 3) == 0 && ((uintptr_t)window & 7) == 0, "loss_mse must be 4-byte aligned, window 8-byte aligned");
    XR_REQUIRE(slot_loss < XR_LOG_WINDOW_SLOTS && slot_psnr < XR_LOG_WINDOW_SLOTS && slot_loss != slot_psnr,
               "two different slots inside the window");
    XR_REQUIRE(n_rays >= 1 && n_rays < (1u << 29), "n_rays is 1 .. 2^29 - 1");
    hipLaunchKernelGGL(k_ngp_log_add, dim3(1), dim3(XR_WAVE), 0, (hipStream_t)stream_, loss_mse, n_rays, window, slot_loss, slot_psnr);
    XR_LAUNCH_CHECK();
    return XR_OK;
}
