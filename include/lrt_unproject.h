/*
 * lrt_unproject.h -- C ABI of the point clouds of range images (liblrt_unproject.so, a library of its own next to liblrt_hip.so and the ten
 * other operator libraries).
 *
 * The step behind everything else: a rendered range image (a depth per ray) becomes the scan a downstream stack reads -- the kept pixels'
 * points, compacted in frame-then-row-major order, the order boolean indexing gives.  It is the inverse of lrt_project_points /
 * lrt_sweepproj_points; the reference does it per frame with a boolean mask (lib/scene/lidar_sensor.py:170-191).
 *
 *   lrt_unproject_work_bytes   the size of the workspace (the per-workgroup counts and bases, the per-frame running totals).
 *   lrt_unproject_points       F frames in one call, three launches: count (one workgroup per 256 consecutive pixels of ONE frame), scan (one
 *                              workgroup over the per-workgroup counts, the running total in int64), write.
 *
 * The rule per pixel (lidar_rt_amd/csrc/lrt_unproject_math.h holds the text).  A pixel gets exactly one class, the first that applies:
 *   invalid        a non-finite depth, origin or direction
 *   masked         keep == 0, or not raydrop < (float) raydrop_ratio (a NaN ray-drop is masked)
 *   out_of_range   not min_depth < depth <= max_depth (a depth of 0, "no return", falls here)
 *   kept           otherwise
 * The point of a kept pixel: without a transform p = o + d * r in float32, the product rounded, then the sum rounded (no contraction) --
 * bit for bit what the boolean-mask expression gives.  With a transform T (3 x 4, row-major, float64): (x, y, z) = o + d * r in float64,
 * q_k = T_k0 x + T_k1 y + T_k2 z + T_k3 summed left to right without contraction, rounded to float32 ONCE.  T is given per frame or per
 * COLUMN (the frame of a moving sensor: every point in the pose of the column that fired it).
 *
 * Outputs: points (cap, 4) float32 [x, y, z, intensity] and pixel (cap) int32 = h W + w, cap = F H W, rows offsets[f] .. offsets[f + 1] belong
 * to frame f and are ordered by pixel; rows from offsets[F] on are not written.  offsets (F + 1) int64.  counts (F, 5) int64 = pixels,
 * invalid, masked, out_of_range, points: pixels == invalid + masked + out_of_range + points.
 *
 * Conventions: as in lrt_project.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`,
 * no allocation and no host wait inside the call.  There is no atomic of any kind: the class is a pure function of the inputs, the count and
 * the write pass evaluate it alike, and every row has one writer -- two calls on equal inputs give equal bits.  Every word of the workspace
 * that is read was written inside the call before, so a stale workspace does not leak.  0 or a negative code (the LRT_ERR_* values of lrt.h)
 * with lrt_unproject_last_error(); the arguments are checked before the device is touched and a refused call launches nothing.
 */
#ifndef LRT_UNPROJECT_H_INCLUDED
#define LRT_UNPROJECT_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_UNPROJECT_ABI_VERSION 1
#define LRT_UNPROJECT_N_COUNTS 5
#define LRT_UNPROJECT_BLOCK 256               /* pixels per workgroup of the count and the write, workgroups per chunk of the scan */
#define LRT_UNPROJECT_MAX_PIXELS 2147483647LL /* F * H * W */
#define LRT_UNPROJECT_MAX_WORKGROUPS 16777215LL /* F * ceil(H W / 256): a launch is a grid of that many workgroups of 256 threads, below 2^32 threads */

int lrt_unproject_abi_version(void);

/* Message of the calling thread's last failed lrt_unproject_* call. */
const char* lrt_unproject_last_error(void);

/* Bytes of the workspace for F frames of H x W pixels (a multiple of 256); negative for F, H, W < 1, F * H * W > LRT_UNPROJECT_MAX_PIXELS or
 * F * ceil(H W / 256) > LRT_UNPROJECT_MAX_WORKGROUPS (many frames of few pixels: a workgroup serves ONE frame).  lrt_unproject_points refuses
 * the same sizes in its argument check. */
long long lrt_unproject_work_bytes(long long F, int H, int W);

/* depth (F, H, W) float32; rays_o, rays_d (F, H, W, 3) float32; intensity (F, H, W) float32 or NULL (0); keep (F, H, W) uint8 or NULL;
 * raydrop (F, H, W) float32 or NULL (raydrop_ratio is not read then); world2out: NULL, or float64 (F, 3, 4) with per_column == 0, or
 * (F, W, 3, 4) with per_column == 1; 0 <= min_depth < max_depth <= FLT_MAX.
 * workspace: 256-byte aligned device memory of work_bytes >= lrt_unproject_work_bytes(F, H, W). */
int lrt_unproject_points(int device, long long F, int H, int W, const float* depth, const float* rays_o, const float* rays_d, const float* intensity,
                         const unsigned char* keep, const float* raydrop, double raydrop_ratio, const double* world2out, int per_column,
                         double min_depth, double max_depth, float* points, int* pixel, long long* offsets, long long* counts,
                         void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_UNPROJECT_H_INCLUDED */
