/* The optimiser step for any number of tensors and the device-side log window: the entry points of libxrnerf_mi355.so that the training
 * runner calls once per iteration (xrnerf_amd/csrc/xr_optim.hip).  A header of its own, bound by its own ctypes table
 * (xrnerf_amd/_lib.py OPTIM_SIGNATURES).
 * Conventions of xrnerf_mi355.h: 0 or a negative XR_E* code (message: xr_last_error()); never throws, syncs or allocates; raw device
 * pointers; the launches go to `stream`.  XR_EINVAL launches nothing and leaves every output untouched. */
#ifndef XRNERF_MI355_OPTIM_H
#define XRNERF_MI355_OPTIM_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define XR_ADAM_LIST_CAPACITY 64u        /* tensors per launch: the by-value work list (5 pointers, a length and a block prefix per tensor =
                                          * 3076 bytes) and the constants stay under HIP's 4-KiB kernel-argument limit */
#define XR_ADAM_LIST_SEGMENT 1024u       /* floats per segment: 256 threads x one 16-byte access */
#define XR_ADAM_LIST_SEGMENTS_PER_GROUP 4u /* consecutive segments one workgroup walks, whichever tensors they belong to */
#define XR_LOG_WINDOW_SLOTS 16u          /* scalars per log window */

/* xr_adam_step_multi's update (torch.optim.Adam with L2 weight decay, the optional EMA copy, grad_scale on the gradients as they are read)
 * for n_tensors >= 1 tensors that share `step` and the constants: ceil(n_tensors / XR_ADAM_LIST_CAPACITY) launches.  The arrays are HOST
 * arrays of device pointers / element counts (ema_host may be NULL, or hold NULL entries); they are copied into the kernel arguments, so
 * nothing is uploaded and the caller may reuse them at once.  The work is cut into segments of XR_ADAM_LIST_SEGMENT floats of ONE tensor;
 * a workgroup takes XR_ADAM_LIST_SEGMENTS_PER_GROUP consecutive segments, so small tensors share a workgroup and a large one spreads over
 * many.  Per element the arithmetic is xr_adam_step_multi's (one definition: csrc/xr_adam.h), so a tensor comes out bit for bit as that
 * call leaves it.  A tensor whose p, g, m, v (or ema) is not 16-byte aligned is updated by 4-byte accesses instead of being refused; 4-byte
 * alignment is required.  Refused (XR_EINVAL): n_tensors < 1, a null array or entry (ema excepted), a length of 0 or beyond 2^32 - 1,
 * step < 1, a pointer that is not 4-byte aligned. */
int xr_adam_step_list(int n_tensors, float* const* p_host, const float* const* g_host, float* const* m_host, float* const* v_host,
                      float* const* ema_host, const size_t* n_host, int step, float lr, float beta1, float beta2, float eps,
                      float weight_decay, float ema_momentum, float grad_scale, void* stream);
/* XR_ADAM_LIST_CAPACITY, for a caller that cannot read this header */
int xr_adam_list_capacity(void);

/* One iteration's log scalars into a window on the device, one workgroup: for i < n_values,
 *   window[i] += (double)*values_host[i] * (double)num_samples,   window[XR_LOG_WINDOW_SLOTS + i] += (double)num_samples
 * values_host: a HOST array of n_values <= XR_LOG_WINDOW_SLOTS device pointers to one fp32 each (copied into the kernel arguments);
 * window: 2 * XR_LOG_WINDOW_SLOTS doubles on the device, zeroed by the caller when a window starts (window + s addresses the slots from s
 * on: then s + n_values <= XR_LOG_WINDOW_SLOTS is the caller's to keep).  Slot i is touched by one thread
 * and the calls of a stream run in order, so a slot's sums are taken in call order; num_samples < 2^29 keeps every product exact.
 * mmcv's LogBuffer.average over the window is window[i] / window[XR_LOG_WINDOW_SLOTS + i].
 * Refused (XR_EINVAL): n_values outside 1 .. XR_LOG_WINDOW_SLOTS, a null pointer, num_samples of 0 or >= 2^29. */
int xr_log_window_add(int n_values, const float* const* values_host, uint32_t num_samples, double* window, void* stream);

#ifdef __cplusplus
}
#endif
#endif
