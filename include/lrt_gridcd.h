/*
 * lrt_gridcd.h -- C ABI of the Chamfer term on the range-image grid (liblrt_gridcd.so, a library of its own next to liblrt_hip.so and
 * liblrt_loss.so).
 *
 * Both clouds of the training loop's Chamfer term are o + d * range on the SAME (H, W) ray grid: cloud A the pixels with mask_a != 0 at
 * range_a, cloud B those with mask_b != 0 at range_b.  Pixel (h, w) of one cloud lies next to pixel (h, w) of the other, so the image is the
 * spatial index: no sort, no tree.  Per valid pixel of A
 *
 *   dist_a[h, w] = min over the valid pixels of B of the squared distance,   idx_a[h, w] = the lowest linear pixel index attaining it
 *
 * (invalid pixels: 0 and -1), dist_b / idx_b symmetrically, and
 *
 *   out = [loss, mean dist_a, mean dist_b, n_a],   loss = weight * 0.5 * (mean dist_a + mean dist_b)
 *
 * with the means over the valid pixels, summed in float64 in a fixed order and rounded once.  If either cloud is empty the loss, the means,
 * every distance and every gradient are exactly 0 (and every index -1): no error.
 *
 * Arithmetic (what makes the results bit-comparable with lrt_chamfer.h on torch-formed points): a point is fadd(o, fmul(d, r)), two
 * roundings, no contraction; a pair's squared distance is fma(dz, dz, fma(dy, dy, dx * dx)) with d = candidate - query; the minimum is taken
 * over (distance, pixel index) pairs, so it does not depend on the visiting order and ties go to the lower pixel index.
 *
 * Backward: with g_a = *d_loss * weight * 0.5 / n_a and g_b likewise over n_b,
 *
 *   grad_a(i) = 2 g_a (a_i - b_nn(i)) + sum over { j : nn_b(j) = i } of 2 g_b (a_i - b_j)            (grad_b symmetrically)
 *   d_range_a = grad_a . d,     d_rays_o = grad_a + grad_b,     d_rays_d = range_a * grad_a + range_b * grad_b
 *
 * The sum is a gather over an inverse neighbour list (integer atomics only), added up in float64 in ascending j: no float atomics, the same
 * bits on every call.  Every output element is written exactly once, zeros included: the buffers need no clearing.
 *
 * Conventions: as in lrt_loss.h -- device pointers to contiguous float32 (masks: uint8, 0 / non-zero; indices: int32), stream-ordered on
 * `device`, no allocation and no host wait inside a call, 0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_gridcd_last_error().
 * `work` is a caller-owned device buffer of at least lrt_gridcd_work_bytes(H, W) bytes, 16-byte aligned; it is scratch only: the backward
 * reads nothing the forward left there.
 */
#ifndef LRT_GRIDCD_H_INCLUDED
#define LRT_GRIDCD_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_GRIDCD_ABI_VERSION 1

int lrt_gridcd_abi_version(void);

/* Message of the calling thread's last failed lrt_gridcd_* call. */
const char* lrt_gridcd_last_error(void);

/* Bytes of the workspace for an H x W image (0 for an invalid size). */
size_t lrt_gridcd_work_bytes(int H, int W);

/* rays_o, rays_d (H, W, 3); range_*, dist_* (H, W) float32; mask_* (H, W) uint8; idx_* (H, W) int32; out: 4 floats on the device. */
int lrt_gridcd_forward(int device, int H, int W, const float* rays_o, const float* rays_d, const float* range_a, const uint8_t* mask_a,
                       const float* range_b, const uint8_t* mask_b, double weight, float* out, float* dist_a, float* dist_b,
                       int32_t* idx_a, int32_t* idx_b, void* work, size_t work_bytes, void* stream);

/* idx_a, idx_b: what the forward returned for the same inputs.  d_loss: one float on the device.  d_range_a (H, W); d_rays_o, d_rays_d
 * (H, W, 3) or both null (then cloud B's gradient is not formed). */
int lrt_gridcd_backward(int device, int H, int W, const float* rays_o, const float* rays_d, const float* range_a, const uint8_t* mask_a,
                        const float* range_b, const uint8_t* mask_b, double weight, const int32_t* idx_a, const int32_t* idx_b,
                        const float* d_loss, float* d_range_a, float* d_rays_o, float* d_rays_d, void* work, size_t work_bytes,
                        void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_GRIDCD_H_INCLUDED */
