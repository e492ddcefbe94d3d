/*
 * lrt_mapreg.h -- C ABI of the scan-to-map registration (liblrt_mapreg.so, a twenty-first library next to liblrt_reg.so and liblrt_sweepfuse.so):
 * direct alignment of range images to the fused TSDF grid of lrt_mesh.h (Bylow et al., RSS 2013).  No correspondence search, no normals, no
 * rendered view: one trilinear sample per source pixel gives the residual and its gradient.
 *
 * The GRID is lrt_mesh.h's: tsdf float32 and weight int32, dense C-order (X, Y, Z), with voxel, trunc and min_weight >= 1.  A FRAME is
 * src_points (H, W, 3) float32 sensor-frame points and src_mask (H, W) uint8, as in lrt_reg.h.  pose (F, 3, 4) float64 row-major on the device is
 * the pose of source frame f in the GRID frame: the world minus the grid's origin.
 *
 * THE RULE, per source pixel with src_mask != 0 (lidar_rt_amd/csrc/lrt_mapreg_math.h is its text for the device and the host; float64 with
 * contraction off; it includes lrt_raycast_math.h, lrt_reg_math.h and lrt_project_math.h as they are):
 *   1. q = X p by pj_transform.  No term if a component is not finite, or if q on any axis lies outside [c_0, c_{N-1}], c_i = (double) rc_centre.
 *      A grid with an axis of fewer than 2 voxels has no domain.
 *   2. The cell is rc_cell and the fractions f = rc_clamp01((q - c_i) / (c_{i+1} - c_i)), exactly as in rc_ray.  The eight corners are v[n], n's
 *      bits being x, y, z.  No term if any corner's weight < min_weight, or if all eight corners are exactly 1.0f (free space: no gradient).
 *   3. D is the trilinear value in the lerp order of rc_tri.  With c00, c10, c01, c11 the four x-lerps, c0, c1 the two y-lerps and
 *      h_a = c_{i+1} - c_i per axis:
 *          gx = lerp(lerp(v1 - v0, v3 - v2, fy), lerp(v5 - v4, v7 - v6, fy), fz) / h_x
 *          gy = lerp(c10 - c00, c11 - c01, fz) / h_y
 *          gz = (c1 - c0) / h_z
 *      No term if g is exactly (0, 0, 0).
 *   4. e = trunc D and n = trunc g, not normalised.  The Huber weight, m = R^T n, J = [m, p x m] and the 30 sums are those of lrt_reg.h steps 4
 *      to 6, and so is THE ORDER: a lane's one term, the wave butterfly, the four waves in wave order, the workgroups (256 consecutive linear
 *      pixel indices each) ascending.  No atomics: equal inputs give equal bits, and a frame's sums do not depend on the other frames.
 *   5. The solve is rg_solve of lrt_reg_math.h, unchanged, one wave per frame, with the statuses and the freeze-after-first-status rule of
 *      lrt_reg_align.  It also writes G_out (F, 3, 4) = X_out^-1: R^T and -(R^T t), rows summed left to right -- the grid2sensor that
 *      lrt_mesh_integrate takes, so that fusing a tracked frame never needs the host to read a pose.
 *
 *   lrt_mapreg_work_bytes   the size of the workspace for F frames of H x W (the workgroups' partial rows and the running status).
 *   lrt_mapreg_linearize    two launches: the 30 sums of every frame at `pose`, and optionally cell (F, H, W) int32: the linear voxel index
 *                           (i Y + j) Z + k of the cell's base corner, -1 for a pixel without a term.
 *   lrt_mapreg_align        2 K launches for K <= 32 iterations from X_init.  X_out (F, 3, 4) is the running pose: iteration 0 reads X_init, every
 *                           iteration writes X_out and G_out.  log (F, K, 8): terms, sum w e^2, sum w, |rho|, |phi|, status after the iteration,
 *                           0, 0.  hessian (F, 6, 6): the full symmetric A of the LAST iteration's sums.  status (F) int32.
 *
 * Conventions: as in lrt_reg.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`, no
 * allocation and no host wait inside a call, no float atomics, every output element is written, the inputs are not changed.  X_out of one call
 * may be the X_init of a LATER call on the same stream.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_mapreg_last_error(); the
 * arguments are checked before the device is touched and a refused call launches nothing.
 */
#ifndef LRT_MAPREG_H_INCLUDED
#define LRT_MAPREG_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_MAPREG_ABI_VERSION 1
#define LRT_MAPREG_BLOCK 256              /* source pixels per workgroup of the linearisation: LRT_REG_BLOCK */
#define LRT_MAPREG_NSUM 30                /* sums per frame: LRT_REG_NSUM */
#define LRT_MAPREG_NLOG 8                 /* numbers per log row: LRT_REG_NLOG */
#define LRT_MAPREG_MAX_ITER 32
#define LRT_MAPREG_MAX_FRAMES 65535
#define LRT_MAPREG_MAX_PIXELS 715827882LL /* F H W at most (2^31 - 1) / 3 */
#define LRT_MAPREG_MAX_VOXELS 2147483647LL /* X Y Z: LRT_MESH_MAX_VOXELS */

int lrt_mapreg_abi_version(void);

/* Message of the calling thread's last failed lrt_mapreg_* call. */
const char* lrt_mapreg_last_error(void);

/* Bytes of the workspace for F frames of H x W pixels (a multiple of 256); negative for F, H, W < 1, F > LRT_MAPREG_MAX_FRAMES or
 * F * H * W > LRT_MAPREG_MAX_PIXELS. */
long long lrt_mapreg_work_bytes(long long F, int H, int W);

/* The 30 sums of F frames at pose (F, 3, 4) float64.  sums (F, 30) float64; cell (F, H, W) int32 or NULL.  workspace: 256-byte aligned device
 * memory of work_bytes >= lrt_mapreg_work_bytes(F, H, W). */
int lrt_mapreg_linearize(int device, int X, int Y, int Z, double voxel, double trunc, const float* tsdf, const int* weight, int min_weight, long long F,
                         int H, int W, const float* src_points, const unsigned char* src_mask, const double* pose, double huber, double* sums, int* cell,
                         void* workspace, long long work_bytes, void* stream);

/* K iterations from X_init (F, 3, 4) float64; see above.  X_out, G_out (F, 3, 4), log (F, K, 8), hessian (F, 6, 6) float64, status (F) int32. */
int lrt_mapreg_align(int device, int X, int Y, int Z, double voxel, double trunc, const float* tsdf, const int* weight, int min_weight, long long F,
                     int H, int W, const float* src_points, const unsigned char* src_mask, const double* X_init, int K, double huber, double lambda,
                     long long min_pairs, double tol_t, double tol_r, double* X_out, double* G_out, double* log, double* hessian, int* status,
                     void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_MAPREG_H_INCLUDED */
