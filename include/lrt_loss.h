/*
 * lrt_loss.h -- C ABI of the fused range-image training loss (liblrt_loss.so, a library of its own next to liblrt_hip.so).
 *
 * Two launches forward and one backward replace the per-pixel part of the reference's train.py:160-214 (and of
 * lidar_rt_amd.training.training_step) between the tracer's (H, W, 9) image and loss.backward(): four channel slices, a sigmoid or a
 * two-way softmax, three masked means, clamp + binary cross-entropy and the DSSIM term (lib/utils/loss_utils.py ssim: 11 x 11 Gaussian
 * window, sigma 1.5, zero padding, C1 = 0.01^2, C2 = 0.03^2).  Per pixel, with r = rendered[y, x, :], m = mask (1 = a return),
 * n = max(sum m, 1), N = H W:
 *
 *   depth     = w[0] * sum m |r[3] - gt_depth| / n
 *   intensity = w[1] * sum m |r[0] - gt_int| / n + w[2] * sum m (r[0] - gt_int)^2 / n + w[3] * (1 - mean_N SSIM(m r[0], m gt_int))
 *   ray drop  = w[4] * mean_N BCE(clamp(p, 1e-7, 1 - 1e-7), 1 - m),  p = sigmoid(r[2]), or softmax(r[1], r[2])[1] with use_rayhit
 *               (probability, clamp and logarithms in float32, the clamp passes gradient where torch.clamp does)
 *   total     = depth + intensity + ray drop
 *
 * A weight of 0 skips that term's work and yields an exact 0.  No float atomics: every sum is taken in a fixed order, so a call returns the
 * same bits every time and on every device of the same kind.
 *
 * Conventions: as in lrt.h -- device pointers to contiguous float32 (mask: uint8, 0 / non-zero), stream-ordered on `device`, no allocation
 * and no host wait inside a call, 0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_loss_last_error().  `weights` is a HOST
 * array of 5 doubles.  `work` is a caller-owned device buffer of at least lrt_loss_work_bytes(H, W) bytes, 16-byte aligned: the forward
 * leaves n, the SSIM derivative maps and its partial sums there, and the backward of the SAME inputs reads them.
 */
#ifndef LRT_LOSS_H_INCLUDED
#define LRT_LOSS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_LOSS_ABI_VERSION 1

int lrt_loss_abi_version(void);

/* Message of the calling thread's last failed lrt_loss_* call. */
const char* lrt_loss_last_error(void);

/* Bytes of the workspace for an H x W image (0 for an invalid size). */
size_t lrt_loss_work_bytes(int H, int W);

/* out (device, 5 floats) = [total, depth term, intensity term, ray-drop term, n]. */
int lrt_loss_forward(int device, int H, int W, const float* rendered, const float* gt_depth, const float* gt_intensity,
                     const uint8_t* mask, const double* weights, int use_rayhit, float* out, void* work, size_t work_bytes, void* stream);

/* d_rendered (H, W, 9) = *d_total (one float on the device) times the gradient of `total`.  Every 36-byte row is written once and whole:
 * channels 4-8, and channel 1 without use_rayhit, are exactly 0, and the buffer needs no clearing.  `work` must hold what
 * lrt_loss_forward left there for the same inputs, weights and use_rayhit. */
int lrt_loss_backward(int device, int H, int W, const float* rendered, const float* gt_depth, const float* gt_intensity,
                      const uint8_t* mask, const double* weights, int use_rayhit, const float* d_total, float* d_rendered, void* work,
                      size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_LOSS_H_INCLUDED */
