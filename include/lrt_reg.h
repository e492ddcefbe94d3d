/*
 * lrt_reg.h -- C ABI of the scan registration (liblrt_reg.so, a library of its own next to liblrt_beams.so and the thirteen others):
 * projective point-to-plane ICP between two range images of the same sensor model.  The image is the spatial index: no tree, no sort.
 *
 * A PAIR is a source frame and a target frame, all float32 on the device:
 *     src_points (H, W, 3)  sensor-frame points (local direction * range),  src_mask (H, W) uint8
 *     tgt_points (H, W, 3), tgt_normals (H, W, 3), tgt_mask (H, W) uint8
 * X (3, 4) float64 row-major on the device is the source sensor's pose in the target sensor's frame, X = T_tgt^-1 T_src.  The sensor model is
 * that of lrt_project.h: H, W, n_inc inclinations (2 bounds, or a strictly monotonic table of H >= 3 beams) as float64 on the device, the
 * pixel offset `off`, `yaw`, and the depth interval (min_depth, max_depth] of lrt_project_math.h's PjRule; wrap = 1 always.
 *
 * THE RULE, per source pixel i with src_mask != 0 (lidar_rt_amd/csrc/lrt_reg_math.h is its text for the device and the host; float64 with
 * contraction off unless float32 is named):
 *   1. q = X p, rows summed left to right (pj_transform).  q32 = q rounded once to float32.
 *   2. (h0, w0) = the pixel of q by pj_classify, unchanged.  A point that is not PJ_KEEP has no partner.
 *   3. The partner: over rows h0 - rh .. h0 + rh (rows outside [0, H) are skipped) and columns w0 - rw .. w0 + rw (modulo W) the pixel with
 *      tgt_mask != 0 and the smallest d2 = fma(dz, dz, fma(dy, dy, dx * dx)), d = tgt_point - q32, all float32 (the arithmetic of lrt_gridcd.h);
 *      ties go to the lower linear pixel index h W + w; a pixel whose d2 is not a number is skipped.  No partner if there is no such pixel, if
 *      (double) d2 > max_dist * max_dist, or if the partner's normal is exactly (0, 0, 0).
 *      DECISION: the (0, 0, 1) fall-back normal of lrt_init_normals is NOT treated specially.  It cannot be told from the true normal of a
 *      level floor, which is the largest surface of most scans; a producer that knows a normal to be a fall-back stores (0, 0, 0) instead
 *      (registration.frame_geometry does for a pixel with fewer than three listed neighbours), and that is the one way to exclude a normal.
 *   4. e = n . (q - q_t), summed x, y, z; Huber weight w = 1 if |e| <= huber, else huber / |e|.
 *   5. Right perturbation X <- X Exp(delta), delta = (rho, phi), the convention of poses.se3_exp and of the twists (lrt_sweep_math.h, sw_exp).
 *      With m = R^T n the Jacobian of e is J = [m, p x m].
 *   6. The 30 sums of a pair, float64:  [0, 21) the upper triangle of A = sum w J J^T, row-major (00, 01, .., 05, 11, 12, .., 55), each term
 *      (w J_i) J_j;  [21, 27) b = sum (w J_i) e;  [27] sum (w e) e;  [28] sum w;  [29] the number of partners (an integer, exact in float64
 *      below 2^53).
 *      THE ORDER: a lane's one term; the 64 lanes of a wave by the butterfly x += shuffle_xor(x, m), m = 32, 16, .., 1; the four waves of a
 *      256-pixel workgroup in wave order; the workgroups of a pair (256 consecutive linear pixel indices each) in ascending order.  No atomics:
 *      equal inputs give equal bits, and a pair's sums do not depend on the other pairs of the call.
 *   Solve (one wave per pair): status 1 if the number of partners < min_pairs.  M = A + lambda diag(A) + LRT_REG_EPS I; Cholesky M = L L^T in
 *      float64, status 2 at the first pivot that is not > 0; M delta = -b.  Status 3 (converged) if |rho| < tol_t and |phi| < tol_r.  Status 0:
 *      X <- X Exp(delta).  From the first non-zero status on -- the iteration that sets it included -- X keeps its bits; later iterations of
 *      that pair write their log row and nothing else.
 *
 *   lrt_reg_work_bytes   the size of the workspace for F pairs of H x W (the workgroups' partial rows and the running status).
 *   lrt_reg_linearize    two launches: the 30 sums of every pair at X, and optionally assoc (F, H, W) int32: the partner's linear pixel index in
 *                        the target image, -1 for none (and for a source pixel that is masked out).
 *   lrt_reg_align        2 K launches for a schedule of K iterations -- linearize and solve, for all F pairs at once.  schedule (K, 3) float64 on
 *                        the HOST: rh, rw, max_dist per iteration (coarse to fine), K <= 32, rh <= 4, rw <= 16.  X_out (F, 3, 4) is the running
 *                        pose: iteration 0 reads X_init, every iteration writes X_out.  log (F, K, 8): partners, sum w e^2, sum w, |rho|, |phi|,
 *                        status after the iteration, 0, 0 (the two norms are 0 in a row whose status is 1 or 2, and in every row after the first
 *                        non-zero one).  hessian (F, 6, 6): the full symmetric A of the LAST iteration's sums.  status (F) int32.
 *
 * Conventions: as in lrt_init.h -- every data pointer but `schedule` is a device pointer to contiguous memory, all work is ordered on `stream`
 * of `device`, no allocation and no host wait inside a call, no float atomics, every output element is written, the inputs are not changed.
 * X_out of one call may be the X_init of a LATER call on the same stream: frames are chained without the host ever reading a pose.  What a
 * call reads from the workspace it has written before.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_reg_last_error(); the
 * arguments are checked before the device is touched and a refused call launches nothing.
 */
#ifndef LRT_REG_H_INCLUDED
#define LRT_REG_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_REG_ABI_VERSION 1
#define LRT_REG_BLOCK 256              /* source pixels per workgroup of the linearisation */
#define LRT_REG_NSUM 30                /* sums per pair */
#define LRT_REG_NLOG 8                 /* numbers per log row */
#define LRT_REG_MAX_ITER 32
#define LRT_REG_MAX_RH 4
#define LRT_REG_MAX_RW 16
#define LRT_REG_MAX_PAIRS 65535
#define LRT_REG_MAX_PIXELS 715827882LL /* F H W at most (2^31 - 1) / 3 */
#define LRT_REG_EPS 1e-12              /* the constant added to the diagonal before the Cholesky factorisation */

int lrt_reg_abi_version(void);

/* Message of the calling thread's last failed lrt_reg_* call. */
const char* lrt_reg_last_error(void);

/* Bytes of the workspace for F pairs of H x W pixels (a multiple of 256); negative for F, H, W < 1, F > LRT_REG_MAX_PAIRS or
 * F * H * W > LRT_REG_MAX_PIXELS. */
long long lrt_reg_work_bytes(long long F, int H, int W);

/* The 30 sums of F pairs at X (F, 3, 4) float64.  sums (F, 30) float64; assoc (F, H, W) int32 or NULL.  workspace: 256-byte aligned device
 * memory of work_bytes >= lrt_reg_work_bytes(F, H, W). */
int lrt_reg_linearize(int device, long long F, int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth,
                      double max_depth, const float* src_points, const unsigned char* src_mask, const float* tgt_points, const float* tgt_normals,
                      const unsigned char* tgt_mask, const double* X, int rh, int rw, double max_dist, double huber, double* sums, int* assoc,
                      void* workspace, long long work_bytes, void* stream);

/* K iterations from X_init (F, 3, 4) float64; see above.  X_out (F, 3, 4), log (F, K, 8), hessian (F, 6, 6) float64, status (F) int32. */
int lrt_reg_align(int device, long long F, int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth,
                  double max_depth, const float* src_points, const unsigned char* src_mask, const float* tgt_points, const float* tgt_normals,
                  const unsigned char* tgt_mask, const double* X_init, const double* schedule, int K, double huber, double lambda,
                  long long min_pairs, double tol_t, double tol_r, double* X_out, double* log, double* hessian, int* status, void* workspace,
                  long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_REG_H_INCLUDED */
