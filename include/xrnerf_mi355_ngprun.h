/* The instant-ngp training loop as a config-driven runner needs it (xrnerf_amd/csrc/xr_ngprun.hip, xr_step.hip): every
 * iteration's `loss` and `psnr` go into a log window on the device from inside the native loop, so that a logger's interval average never
 * makes the loop return to the interpreter.  A header of its own, bound by its own ctypes table (xrnerf_amd/_lib.py NGPRUN_SIGNATURES).
 * Conventions of xrnerf_mi355.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw device
 * pointers; the launches go to `stream`.  XR_EINVAL launches nothing and leaves every output untouched. */
#ifndef XRNERF_MI355_NGPRUN_H
#define XRNERF_MI355_NGPRUN_H
#include <stddef.h>
#include <stdint.h>
#include "xrnerf_mi355.h"
#include "xrnerf_mi355_optim.h"
#ifdef __cplusplus
extern "C" {
#endif

/* One training iteration's two log values into a log window (xr_log_window_add's layout: 2 * XR_LOG_WINDOW_SLOTS doubles, sums in
 * [0, SLOTS), sample counts in [SLOTS, 2 SLOTS)), one launch of one workgroup:
 *   window[slot_loss] += (double)loss_mse[0] * n_rays                                  (exact: 24 + 29 bits)
 *   window[slot_psnr] += psnr * n_rays,   psnr = -10 log10((double)loss_mse[1] / (3.0 * n_rays))
 *   window[XR_LOG_WINDOW_SLOTS + slot] += (double)n_rays                               for both slots
 * loss_mse: the two fp32 scalars a training step leaves (xr_train_loss_scalars: the loss, and the sum over rays and channels of the squared
 * difference of the alpha-masked images); psnr is mse2psnr(img2mse(rgb alpha, target alpha)) of networks/hashnerf.py:40-42 taken from that
 * sum, formed in double.  One thread owns one slot and the calls of a stream run in order, so a slot's sums are taken in call order.
 * Refused (XR_EINVAL): a null pointer, a misaligned pointer (4 bytes for loss_mse, 8 for window), equal slots, a slot outside
 * [0, XR_LOG_WINDOW_SLOTS), n_rays of 0 or >= 2^29. */
int xr_ngp_log_add(const float* loss_mse, uint32_t n_rays, double* window, uint32_t slot_loss, uint32_t slot_psnr, void* stream);

/* xr_ngp_loop_run with one xr_ngp_log_add launch behind each iteration's step, on the loop's stream, reading that iteration's step set
 * (desc->step[...].loss_mse).  The other launches are xr_ngp_loop_run's, in the same order; log_window == NULL is xr_ngp_loop_run
 * (the slots are then not looked at).  The slot checks are made before anything is enqueued. */
int xr_ngp_loop_run_logged(const xr_ngp_loop_desc* desc, xr_ngp_loop_state* state, uint32_t k, uint32_t n_rays, const float* lr,
                           const float* ema_momentum, double* log_window, uint32_t slot_loss, uint32_t slot_psnr, const char* timed_entry,
                           void* const* timing_events, void* const* iter_events);

#ifdef __cplusplus
}
#endif
#endif
