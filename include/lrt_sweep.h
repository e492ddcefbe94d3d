/*
 * lrt_sweep.h -- C ABI of the sweep rays (liblrt_sweep.so, a library of its own next to liblrt_hip.so, liblrt_loss.so, liblrt_gridcd.so,
 * liblrt_init.so, liblrt_metrics.so, liblrt_adam.so, liblrt_densify.so and liblrt_project.so).
 *
 * The ray grid of a spinning LiDAR that moves while it turns: column w of the range image is fired at its own instant, so it has its own
 * pose.  For frame f the pose at sweep fraction s is T_f(s) = P_f Exp(s xi_f): P_f (3, 4) the sensor-to-world pose at the reference instant,
 * xi_f = (rho, phi) the sensor's motion over one whole sweep in the sensor frame (the convention of poses.se3_exp and of
 * sensor2world @ Exp(xi)).  Column w has s = tau[w]; its local direction l(h, w) is RangeFrames.range_rays's (azimuth
 * (W - w - off) / W 2 pi - pi - yaw, inclination from two bounds or from the flipped per-beam table).  With R_w the rotation of T_f(tau[w]):
 *
 *     ray_d[f, h, w] = float32(R_w l / |R_w l|)        ray_o[f, h, w] = float32(translation of T_f(tau[w]))
 *
 * lidar_rt_amd/csrc/lrt_sweep_math.h holds the text; all of it float64, each component rounded once.
 *
 *   lrt_sweep_work_bytes   the size of the workspace for F frames of H x W.
 *   lrt_sweep_rays         two launches: the per-column table (Exp, the azimuth's sine and cosine, once per column) and the per-row table (the
 *                          inclination's sine and cosine, once per row) in float64; then one thread per output component, coalesced stores.
 *   lrt_sweep_backward     two launches: from g_o, g_d (F, H, W, 3) to d_pose (F, 3, 4) and d_twist (F, 6), the normalisation included.  One
 *                          thread per column sums its rows in row order and chains the sums through dExp/dxi; a workgroup sums its columns;
 *                          a finishing launch sums the workgroups of a frame in order.  All sums in float64 in a fixed order, no float atomics,
 *                          each result rounded to float32 once.
 *
 * Conventions: as in lrt_project.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`,
 * no allocation and no host wait inside a call, every output element is written, the inputs are not changed.  What a call reads from the
 * workspace it has written before, so a stale workspace does not leak.  0 or a negative code (the LRT_ERR_* values of lrt.h) with
 * lrt_sweep_last_error(); the arguments are checked before the device is touched and a refused call launches nothing.
 */
#ifndef LRT_SWEEP_H_INCLUDED
#define LRT_SWEEP_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_SWEEP_ABI_VERSION 1
#define LRT_SWEEP_BLOCK 256                /* output components per workgroup of the ray pass, table entries per workgroup of the table pass */
#define LRT_SWEEP_COLS 64                  /* columns per workgroup of the backward pass (one wave) */
#define LRT_SWEEP_MAX_RAYS 715827882LL     /* F * H * W: three components per ray, indexed below 2^31 */

int lrt_sweep_abi_version(void);

/* Message of the calling thread's last failed lrt_sweep_* call. */
const char* lrt_sweep_last_error(void);

/* Bytes of the workspace for F frames of H x W rays (a multiple of 256); negative for F, H, W < 1 or F * H * W > LRT_SWEEP_MAX_RAYS. */
long long lrt_sweep_work_bytes(long long F, int H, int W);

/* pose (F, 3, 4) float32; twist (F, 6) float32 or NULL (a static sensor: every column has the pose itself); inclination: n_inc float32,
 * n_inc == 2 (bounds) or n_inc == H (per-beam table; H == 2 reads as bounds); off: 0 (KITTI) or 0.5 (Waymo), in [0, 1); tau (W) float32 (not read
 * without a twist, may be NULL then).  ray_o, ray_d (F, H, W, 3) float32.
 * workspace: 256-byte aligned device memory of work_bytes >= lrt_sweep_work_bytes(F, H, W). */
int lrt_sweep_rays(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                   double off, double yaw, const float* tau, float* ray_o, float* ray_d, void* workspace, long long work_bytes, void* stream);

/* The same inputs, plus g_o, g_d (F, H, W, 3) float32.  d_pose (F, 3, 4) float32; d_twist (F, 6) float32, required with a twist; without one it
 * may be NULL, and is set to zero where it is given. */
int lrt_sweep_backward(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                       double off, double yaw, const float* tau, const float* g_o, const float* g_d, float* d_pose, float* d_twist,
                       void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_SWEEP_H_INCLUDED */
