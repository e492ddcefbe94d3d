/*
 * lrt_sweepproj.h -- C ABI of the range-image projection under the sweep model (liblrt_sweepproj.so, a library of its own next to
 * liblrt_project.so and liblrt_sweep.so): the inverse of lrt_sweep_rays, as lrt_project_points is the inverse of RangeFrames.range_rays.
 *
 * Column w of a moving sensor is fired from its own pose P Exp(tau[w] xi) (include/lrt_sweep.h).  A point given in the sensor frame of the
 * frame's reference instant (a motion-compensated scan, or world points under points2sensor) therefore belongs to the column that, AT ITS OWN
 * INSTANT, has the point inside its azimuth bin, and its range is measured from that column's origin.  The frame's pose never enters:
 * relative to the reference instant column w sits at E_w = Exp(tau[w] xi) = [R_w | t_w], and it sees the point p at q_w = R_w^T (p - t_w).
 *
 *   lrt_sweepproj_work_bytes   the size of the workspace: the key image (one 64-bit word per pixel of every frame) and the column table
 *                              (the inverse of E_w as 12 float64 per frame and column).
 *   lrt_sweepproj_points       F frames in one call, at most four launches: the column table; the key image set to all-ones and the counts to
 *                              zero; one thread per point runs the column search and does one 64-bit unsigned atomic min on its pixel's
 *                              word; one thread per pixel turns the word into depth, mask and index and gathers the winner's intensity.
 *
 * The rule per point (lidar_rt_amd/csrc/lrt_sweepproj_math.h holds the text; all of it float64, the one float32 value is r32):
 *   1. p = points2sensor[f] (x, y, z, 1) where a transform is given.  A non-finite coordinate: invalid.
 *   2. The search starts at the static column w_0 of p: lrt_project.h's u and rint, taken mod W with `wrap`, clamped into [0, W - 1] without.
 *   3. At most LRT_SWEEPPROJ_MAX_EVAL evaluations: q = q_{w_k}, c = rint(u(q)).  c (wrapped, with `wrap`) == w_k: converged.  Without `wrap`,
 *      c outside [0, W) whose clamp is w_k: the point is beyond the image's edge, the search ends out of view.  Otherwise w_{k+1} is the
 *      wrapped or clamped c.  No convergence within the evaluations: unseen.  A column whose E_w is exactly the identity (no twist, a zero
 *      twist, tau[w] == 0) leaves the point as it is, the sign of a zero included.
 *   4. q of the LAST evaluated column is classed in lrt_project.h's order: a non-finite q or r = |q| == 0 is invalid; r32 = (float) r outside
 *      (min_depth, max_depth] is out_of_range; a column out of view is out_of_view; a search that did not converge is unseen; the row comes
 *      from el = atan2(z, hypot(x, y)) of q by lrt_project.h's row rules, a failing row is out_of_view; otherwise the point is kept at pixel
 *      (row, w_k) with r32.
 *   5. The winner of a pixel is the kept point with the smallest r32, ties to the lower in-frame index: the key of lrt_project.h.
 * A point becomes at most one pixel: the fixed point that the iteration reaches from the static column.  With twist == NULL or all zeros
 * every output equals lrt_project_points on the same arguments bit for bit, and unseen is 0.
 *
 * Outputs, every element written: depth, intensity (F, H, W) float32, 0 where there is no return; mask (F, H, W) uint8; index (F, H, W) int32,
 * the winner's row WITHIN ITS FRAME, -1 where there is none; counts (F, 7) int64 = points, invalid, out_of_range, out_of_view, unseen, hidden,
 * pixels: points == the sum of the other six.
 *
 * Conventions: those of lrt_project.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of
 * `device`, no allocation and no host wait inside the call.  The only atomics are a 64-bit unsigned min and 64-bit integer adds, which commute:
 * two calls on equal inputs give equal bits, whatever the arrival order; the key image and the column table are set inside the call, so a
 * stale workspace does not leak.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_sweepproj_last_error(); the arguments are
 * checked before the device is touched and a refused call launches nothing.  Memory safety does not depend on the values in `offsets`,
 * `inclination`, `tau`, `twist` or the points: a column that arithmetic produced is range-checked before it indexes the table (a NaN
 * included), and a row or a pixel outside its array is never touched.
 */
#ifndef LRT_SWEEPPROJ_H_INCLUDED
#define LRT_SWEEPPROJ_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_SWEEPPROJ_ABI_VERSION 1
#define LRT_SWEEPPROJ_N_COUNTS 7
#define LRT_SWEEPPROJ_MAX_EVAL 8              /* evaluations of the column search per point */
#define LRT_SWEEPPROJ_TABLE 12                /* float64 per frame and column: the inverse of E_w, row-major 3 x 4 */
#define LRT_SWEEPPROJ_BLOCK 256               /* points, pixels or columns per workgroup */
#define LRT_SWEEPPROJ_MAX_POINTS 2147483647LL /* in-frame indices are int32 */
#define LRT_SWEEPPROJ_MAX_PIXELS 2147483647LL /* F * H * W */

int lrt_sweepproj_abi_version(void);

/* Message of the calling thread's last failed lrt_sweepproj_* call. */
const char* lrt_sweepproj_last_error(void);

/* Bytes of the workspace for F frames of H x W pixels: F H W 8 for the key image plus F W 96 for the column table, rounded up to a multiple of
 * 256; negative for F, H, W < 1 or F * H * W > LRT_SWEEPPROJ_MAX_PIXELS. */
long long lrt_sweepproj_work_bytes(long long F, int H, int W);

/* points, offsets, points2sensor, inclination, off, yaw, the depths, wrap and the outputs: as in lrt_project_points.
 * twist (F, 6) float64 xi = (rho, phi), the sensor's motion over one sweep in the sensor frame (lrt_sweep.h), or NULL (a static sensor);
 * tau (W) float64, the instant of every column in sweeps, shared by the frames: required with a twist, not read without one.
 * workspace: 256-byte aligned device memory of work_bytes >= lrt_sweepproj_work_bytes(F, H, W). */
int lrt_sweepproj_points(int device, long long N, const float* points, long long F, const long long* offsets, const double* points2sensor,
                         const double* twist, const double* tau, int H, int W, const double* inclination, int n_inc, double off, double yaw,
                         double min_depth, double max_depth, int wrap,
                         float* depth, float* intensity, unsigned char* mask, int* index, long long* counts,
                         void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_SWEEPPROJ_H_INCLUDED */
