/*
 * lrt_segment.h -- C ABI of the range-image segmentation (liblrt_segment.so, a sixteenth library next to liblrt_reg.so and the fourteen others):
 * ground, connected segments, free-space evidence between frames, one integer row per segment and the extent of a track -- what
 * lidar_rt_amd/actors.py turns into the tracking boxes of moving actors.  The image is the spatial index: no tree, no sort.
 *
 * All operators take F frames of ONE H x W sensor model in one call (the frame is grid.y); a frame's result does not depend on the frames
 * beside it.  The inputs, on the device:
 *     points (F, H, W, 3) float32  sensor-frame points (local direction * range),  mask (F, H, W) uint8
 * lidar_rt_amd/csrc/lrt_segment_math.h is the text of every rule for the device and the host (float64 with contraction off unless float32 is
 * named).  EVERY RESULT IS AN INTEGER that does not depend on the order in which lanes arrive: the numpy twins are exact.
 *
 *   lrt_seg_ground   one launch, one lane per (frame, column).  Rows are visited in the order of ASCENDING inclination (row h carries
 *       inc0 + (H - h - off) / H (inc1 - inc0), or the table's entry H - 1 - h: from row H - 1 down when the last inclination is the larger one,
 *       from row 0 up otherwise).  h = up . p summed x, y, z; g = p - h up.  A valid pixel is ground
 *         - while the column has no ground pixel: if z_lo <= h <= z_hi;
 *         - from then on: if |h - h_g| <= slope |g - g_g| against the LAST ground pixel below it (pixels that are not ground in between are
 *           skipped, so the road resumes behind a car; the band is not asked again, so the road may climb).
 *       ground (F, H, W) uint8: 1 or 0, 0 for a pixel that is not valid.
 *   lrt_seg_label    three launches.  Kept pixels: mask != 0 && (exclude == NULL || exclude == 0).  Two kept 4-neighbours -- (h, w +- 1 mod W)
 *       or (h +- 1, w): the column seam is closed -- are joined if and only if, in float32, d2 = fma(dz, dz, fma(dy, dy, dx * dx)) <=
 *       max(d_abs * d_abs, (c_dir * c_dir) * min(r2_a, r2_b)), r2 the same form of the point itself, c_dir = c_h for a horizontal and c_v for a
 *       vertical pair, every product rounded once; a pair with a NaN on either side is not joined.  label (F, H, W) int32: the SMALLEST linear
 *       pixel index h W + w of the pixel's component, -1 for a pixel that is not kept.  (Union-find in `label` itself: runs along a wave are
 *       joined by a ballot, every other pair by atomicMin on roots, then one flatten pass.  Parents only ever decrease, so the root is the
 *       component's smallest index whatever the arrival order.)
 *   lrt_seg_freespace  one launch.  Per valid source pixel q = X p (pj_transform), its pixel by pj_classify with wrap = 1, rq = sqrt(qx qx + qy qy +
 *       qz qz); over the valid target pixels of rows h0 - rh .. h0 + rh (rows outside the image are skipped) and columns w0 - rw .. w0 + rw
 *       (modulo W): ev (F, H, W) int8 = -1 for an invalid source pixel, one that is not PJ_KEEP, or a window without a valid target pixel; 1 if
 *       EVERY valid target pixel of the window has (double) range_t > rq + m_abs + m_rel * rq; 0 otherwise.
 *   lrt_seg_stats    five launches (fill, ballot count, one-workgroup scan per frame, number, accumulate).  Roots (label == own index) are
 *       numbered in ascending index per frame.  seg (F, H, W) int32: the dense id of the pixel's segment or -1; n_seg (F) int32 = min(roots,
 *       S_max); overflow (F) int32 = roots beyond S_max (their pixels get seg = -1); table (F, S_max, 16) int64, a row: the root index, the
 *       pixel count, per evidence image (either may be NULL: zeros) the count of ev == 1 and of ev >= 0, sum qx, qy, qz, min qx, qy, qz,
 *       max qx, qy, qz, 0, with q = llrint(p * 1024) of the float32 coordinate (a coordinate that is not finite, or beyond 9e15 / 1024, counts as
 *       0: points lie within max_depth).  Rows from n_seg on are zeros.  64-bit integer atomics: sums, minima and maxima of integers.
 *   lrt_seg_track_bounds  two launches (fill, accumulate).  track_of (F, S_max) int32, -1 for none; pose (NT, F, 3, 4) float64, the actor in
 *       the SENSOR frame of that frame.  Per pixel of a tracked segment a = R^T (p - t), llrint(a * 1024); bounds (NT, 6) int64 = min x, y, z,
 *       max x, y, z and count (NT) int64.  A track without pixels: count 0, and its bounds are the fill's (INT64_MAX, INT64_MIN).
 *
 * Conventions: as in lrt_reg.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`, no
 * allocation and no host wait inside a call, no float atomics, every output element is written, the inputs are not changed.  0 or a negative
 * code (the LRT_ERR_* values of lrt.h) with lrt_segment_last_error(); the arguments are checked before the device is touched and a refused
 * call launches nothing.
 */
#ifndef LRT_SEGMENT_H_INCLUDED
#define LRT_SEGMENT_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_SEGMENT_ABI_VERSION 1
#define LRT_SEGMENT_BLOCK 256              /* pixels per workgroup */
#define LRT_SEGMENT_NCOL 16                /* int64 entries per table row */
#define LRT_SEGMENT_MAX_RH 4
#define LRT_SEGMENT_MAX_RW 16
#define LRT_SEGMENT_MAX_FRAMES 65535
#define LRT_SEGMENT_MAX_PIXELS 715827882LL /* F H W at most (2^31 - 1) / 3 */
#define LRT_SEGMENT_MAX_SEGMENTS 1048576   /* S_max at most */
#define LRT_SEGMENT_MAX_TRACKS 65535

int lrt_segment_abi_version(void);

/* Message of the calling thread's last failed lrt_seg_* call. */
const char* lrt_segment_last_error(void);

/* Bytes of the workspace of lrt_seg_stats for F frames of H x W pixels (a multiple of 256); negative for F, H, W < 1, F > LRT_SEGMENT_MAX_FRAMES
 * or F * H * W > LRT_SEGMENT_MAX_PIXELS.  The other operators need none. */
long long lrt_seg_work_bytes(long long F, int H, int W);

int lrt_seg_ground(int device, long long F, int H, int W, const double* inclination, int n_inc, const float* points, const unsigned char* mask,
                   double up_x, double up_y, double up_z, double z_lo, double z_hi, double slope, unsigned char* ground, void* stream);

int lrt_seg_label(int device, long long F, int H, int W, const float* points, const unsigned char* mask, const unsigned char* exclude,
                  double d_abs, double c_h, double c_v, int* label, void* stream);

/* X (F, 3, 4) float64, X = T_tgt^-1 T_src; tgt_range (F, H, W) float32; the sensor model arguments of lrt_reg_linearize. */
int lrt_seg_freespace(int device, long long F, int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth,
                      double max_depth, const float* src_points, const unsigned char* src_mask, const float* tgt_range, const unsigned char* tgt_mask,
                      const double* X, int rh, int rw, double m_abs, double m_rel, signed char* ev, void* stream);

/* ev0, ev1 (F, H, W) int8 or NULL.  workspace: 256-byte aligned device memory of work_bytes >= lrt_seg_work_bytes(F, H, W). */
int lrt_seg_stats(int device, long long F, int H, int W, const float* points, const int* label, const signed char* ev0, const signed char* ev1,
                  int S_max, int* seg, int* n_seg, int* overflow, long long* table, void* workspace, long long work_bytes, void* stream);

int lrt_seg_track_bounds(int device, long long F, int H, int W, const float* points, const int* seg, int S_max, const int* track_of, int NT,
                         const double* pose, long long* bounds, long long* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_SEGMENT_H_INCLUDED */
