/*
 * lrt_metrics.h -- C ABI of the fused evaluation metrics (liblrt_metrics.so, a library of its own next to liblrt_hip.so, liblrt_loss.so,
 * liblrt_gridcd.so and liblrt_init.so).
 *
 * One call turns one rendered frame and its ground truth into the row of figures that lidar_rt_amd.evaluation.evaluate reports for it (the
 * metric set of the reference's eval.py:282-365), restated line by line.  With pred_hit = pred_raydrop < (float)raydrop_ratio,
 * gt_hit = gt_mask != 0, mask = use_gt_mask ? gt_hit : pred_hit, n = H W:
 *
 *   depth       y = clamp(gt_depth, 1e-6, max_depth),                x = clamp(pred_depth * mask, 1e-6, max_depth),            peak = max_depth
 *   intensity   y = clamp(clamp(gt_intensity, 0, 1), 1e-6, 1),       x = clamp(clamp(pred_intensity, 0, 1) * mask, 1e-6, 1),   peak = 1
 *   (all of that in float32, as evaluate forms them), e = y - x: ONE float32 subtraction, and per image
 *
 *   rmse   = sqrt(sum e^2 / n)                                      (_image_metrics: mse.sqrt())
 *   mae    = sum |e| / n                                            (err.abs().mean())
 *   medae  = 0.5f * (v[(n - 1) / 2] + v[n / 2]), v = sorted |e|     (_median: numpy's median, float32; the SAME BITS as the sort gives)
 *   ssim   = mean over the (H - 6) x (W - 6) interior of skimage's structural_similarity window term: 7 x 7 uniform window, sample
 *            covariance (x 49 / 48), C1 = (0.01 R)^2, C2 = (0.03 R)^2, R = max y - min y   (ssim_uniform).  R = 0 (a constant ground
 *            truth) makes C1 = C2 = 0 and the term 0 / 0 or rounding noise over rounding noise: the row holds NaN.
 *   psnr   = 10 log10(peak^2 / max(sum e^2 / n, 1e-30))
 *
 *   ray drop, on the masks gt_drop = !gt_hit, pred_drop = !pred_hit (whatever use_gt_mask says), tp / fp / fn / eq counted exactly:
 *   rmse   = sqrt((n - eq) / n)          acc = eq / n
 *   f1     = 2 P R / max(P + R, 1e-30),  P = tp / max(tp + fp, 1),  R = tp / max(tp + fn, 1)            (raydrop_metrics)
 *
 *   points, from dist_a / dist_b = what lrt_gridcd_forward (lrt_gridcd.h) returns for cloud A = gt_depth under gt_mask and cloud B =
 *   pred_depth under `mask`, weight 1 (the caller runs it, with its own workspace, before this call on the same stream; the distances carry
 *   the same bits as chamfer_3DDist on the gathered points):
 *   chamfer_dist = sum dist_a / n_gt + sum dist_b / n_pred                                               (points_metrics)
 *   fscore       = 2 p1 p2 / (p1 + p2), p1 = count(dist_a < (float)fscore_threshold) / n_gt, p2 likewise over B, NaN -> 0   (fscore)
 *   n_pred, n_gt = the sizes of the two clouds (count of `mask`, count of gt_hit); extras
 *   An empty cloud: chamfer_dist = NaN, fscore = 0.  dist_a and dist_b both NULL: the points metrics are skipped, chamfer_dist = fscore = NaN.
 *
 * Sums: the squared and absolute error sums, the window sums of x, y, x^2, y^2, x y, the SSIM arithmetic, the counts, the final ratios, sqrt
 * and log10 are float64, added in a fixed order; each figure is rounded to float32 once.  medae comes from a three-level histogram selection
 * over the bit patterns of |e| (11 / 11 / 9 bits below the sign; both middle ranks are carried and may part at any level): integer atomics
 * only, so no figure depends on the order in which workgroups arrive, and two calls on the same inputs return the same bits.
 *
 * Conventions: as in lrt_loss.h -- device pointers to contiguous float32 (gt_mask: uint8, 0 / non-zero), stream-ordered on `device`, no
 * allocation, no host wait and no float atomics inside a call, 0 or a negative code (the LRT_ERR_* values of lrt.h) with
 * lrt_metrics_last_error().  `work` is a caller-owned device buffer of at least lrt_metrics_work_bytes(H, W) bytes, 16-byte aligned, scratch
 * only.  H < 7 or W < 7 (no SSIM window fits) is LRT_ERR_ARG.  Arguments are checked before the device is touched.
 *
 * `out`: LRT_METRICS_N floats on the device, typically one row of a caller-owned (frames, LRT_METRICS_N) table; EVERY element is written
 * on every call, so the table needs no clearing.
 */
#ifndef LRT_METRICS_H_INCLUDED
#define LRT_METRICS_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_METRICS_ABI_VERSION 1

/* the row */
#define LRT_METRICS_DEPTH_RMSE 0
#define LRT_METRICS_DEPTH_MAE 1
#define LRT_METRICS_DEPTH_MEDAE 2
#define LRT_METRICS_DEPTH_SSIM 3
#define LRT_METRICS_DEPTH_PSNR 4
#define LRT_METRICS_INTENSITY_RMSE 5
#define LRT_METRICS_INTENSITY_MAE 6
#define LRT_METRICS_INTENSITY_MEDAE 7
#define LRT_METRICS_INTENSITY_SSIM 8
#define LRT_METRICS_INTENSITY_PSNR 9
#define LRT_METRICS_RAYDROP_RMSE 10
#define LRT_METRICS_RAYDROP_ACC 11
#define LRT_METRICS_RAYDROP_F1 12
#define LRT_METRICS_POINTS_CHAMFER_DIST 13
#define LRT_METRICS_POINTS_FSCORE 14
#define LRT_METRICS_POINTS_N_PRED 15
#define LRT_METRICS_POINTS_N_GT 16
#define LRT_METRICS_N 17

int lrt_metrics_abi_version(void);

/* Message of the calling thread's last failed lrt_metrics_* call. */
const char* lrt_metrics_last_error(void);

/* Bytes of the workspace for an H x W image (0 for an invalid size). */
size_t lrt_metrics_work_bytes(int H, int W);

/* pred_*, gt_depth, gt_intensity, dist_a, dist_b: (H, W) float32; gt_mask: (H, W) uint8; out: LRT_METRICS_N floats on the device. */
int lrt_metrics_frame(int device, int H, int W, const float* pred_depth, const float* pred_intensity, const float* pred_raydrop,
                      const float* gt_depth, const float* gt_intensity, const uint8_t* gt_mask, const float* dist_a, const float* dist_b,
                      double raydrop_ratio, int use_gt_mask, double max_depth, double fscore_threshold, float* out, void* work,
                      size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_METRICS_H_INCLUDED */
