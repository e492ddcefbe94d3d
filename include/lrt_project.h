/*
 * lrt_project.h -- C ABI of the range-image projection of point clouds (liblrt_project.so, a library of its own next to liblrt_hip.so,
 * liblrt_loss.so, liblrt_gridcd.so, liblrt_init.so, liblrt_metrics.so, liblrt_adam.so and liblrt_densify.so).
 *
 * The step in front of everything else: a LiDAR scan (points in the sensor frame) becomes the range image the loops read -- the spherical
 * projection that keeps the NEAREST return of every pixel.  It is the inverse of RangeFrames.range_rays (lidar_rt_amd/training.py); the
 * reference does it in a Python loop over the points of a frame (lib/dataloader/kitti_loader/__init__.py:206-242).
 *
 *   lrt_project_work_bytes   the size of the workspace (the key image: one 64-bit word per pixel of every frame) for F frames of H x W.
 *   lrt_project_points       F frames in one call, at most three launches: the key image is set to all-ones and the counts to zero; one thread
 *                            per point does one 64-bit unsigned atomic min on its pixel's word; one thread per pixel turns the word into
 *                            depth, mask and index and gathers the winner's intensity.
 *
 * The rule per point (lidar_rt_amd/csrc/lrt_project_math.h holds the text; all of it float64): p = points2sensor[f] (x, y, z, 1) where a
 * transform is given; r = sqrt(x^2 + y^2 + z^2), r32 = (float) r, az = atan2(y, x), el = atan2(z, hypot(x, y)).  A point is dropped at the
 * first test it fails:
 *   invalid        a non-finite coordinate, or r == 0
 *   out_of_range   kept only if min_depth < r32 <= max_depth
 *   out_of_view    column: u = (pi - (az + yaw)) W / 2 pi - off, w = rint(u) (half to even); with `wrap` w is taken mod W, without it a w
 *                  outside [0, W) is out of view (what the reference's loader does: it loses the column that straddles azimuth +-pi).
 *                  row from two bounds [inc0, inc1]: v = H - off - (el - inc0) / (inc1 - inc0) H, h = rint(v), outside [0, H) is out of
 *                  view (rows never wrap).  Row from a table of H beams (row h has inclination inc[H - 1 - h]; the table is strictly
 *                  monotonic -- the CALLER guarantees it, the values live on the device): the beam with the nearest inclination, ties to
 *                  the lower row; further from an outermost beam than half the gap to its one neighbour is out of view.
 * The winner of a pixel is the kept point with the smallest r32; ties go to the lower index within the frame (the order in which the
 * reference's loop keeps the first of equals).  The key is (bits(r32) << 32) | index: positive floats order as their bit patterns.
 *
 * Outputs, every element written: depth (F, H, W) float32 and intensity (F, H, W) float32, 0 where there is no return; mask (F, H, W) uint8;
 * index (F, H, W) int32, the winner's row WITHIN ITS FRAME, -1 where there is none; counts (F, 6) int64 = points, invalid, out_of_range,
 * out_of_view, hidden (kept points that lost their pixel), pixels (winners): points == invalid + out_of_range + out_of_view + hidden + pixels.
 *
 * Conventions: as in lrt_densify.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`,
 * no allocation and no host wait inside the call.  The only atomics are a 64-bit unsigned min and 64-bit integer adds, which commute: two calls
 * on equal inputs give equal bits, whatever the arrival order, and the key image is set inside the call, so a stale workspace does not
 * leak.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_project_last_error(); the arguments are checked before the device is
 * touched and a refused call launches nothing.  Memory safety does not depend on the values in `offsets` or `inclination`: a row or a pixel
 * outside its array is never touched.
 */
#ifndef LRT_PROJECT_H_INCLUDED
#define LRT_PROJECT_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_PROJECT_ABI_VERSION 1
#define LRT_PROJECT_N_COUNTS 6
#define LRT_PROJECT_BLOCK 256               /* points per workgroup of the scatter, pixels per workgroup of the fill and the resolve */
#define LRT_PROJECT_MAX_POINTS 2147483647LL /* in-frame indices are int32 */
#define LRT_PROJECT_MAX_PIXELS 2147483647LL /* F * H * W */

int lrt_project_abi_version(void);

/* Message of the calling thread's last failed lrt_project_* call. */
const char* lrt_project_last_error(void);

/* Bytes of the workspace for F frames of H x W pixels (a multiple of 256); negative for F, H, W < 1 or F * H * W > LRT_PROJECT_MAX_PIXELS. */
long long lrt_project_work_bytes(long long F, int H, int W);

/* points (N, 4) float32 [x, y, z, intensity], all frames back to back; offsets (F + 1) int64, frame f owns rows offsets[f] .. offsets[f + 1]
 * (0 = offsets[0] <= ... <= offsets[F] = N; an empty frame is legal); points2sensor (F, 3, 4) float64 or NULL (the points are in the sensor
 * frame); inclination: n_inc float64, n_inc == 2 (bounds) or n_inc == H (per-beam table; H == 2 reads as bounds); off: 0 (KITTI) or 0.5
 * (Waymo), in [0, 1); 0 <= min_depth < max_depth <= FLT_MAX; wrap: 0 or 1.
 * workspace: 256-byte aligned device memory of work_bytes >= lrt_project_work_bytes(F, H, W). */
int lrt_project_points(int device, long long N, const float* points, long long F, const long long* offsets, const double* points2sensor,
                       int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth, double max_depth, int wrap,
                       float* depth, float* intensity, unsigned char* mask, int* index, long long* counts,
                       void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_PROJECT_H_INCLUDED */
