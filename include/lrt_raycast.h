/*
 * lrt_raycast.h -- C ABI of the ray casting of a fused TSDF grid (liblrt_raycast.so, a nineteenth library next to liblrt_mesh.so and the
 * seventeen others): the range a sensor would see, per ray, from the dense grid that lrt_mesh_integrate fills.
 *
 * lidar_rt_amd/csrc/lrt_raycast_math.h is the text of the rule for the device and the host: float64 with contraction off, only + - * /, sqrt,
 * floor, min and max.  The grid is the one of lrt_mesh.h: dense, C-order (X, Y, Z), voxel centre c_i = (float) (voxel (i + 0.5)) per axis in the
 * grid frame, which sits at `origin` (float64) in the world.
 *
 *   ray        o = (double) ray_o - origin, u = (double) ray_d / |(double) ray_d|; a non-finite component or a zero direction: a miss, 0 samples.
 *   domain     the box of voxel centres [c_0, c_{N-1}] per axis; t_in = max(min_depth, slab entry), t_out = min(max_depth, slab exit); on an axis
 *              with u_a == 0 the ray is inside iff c_0 <= o_a <= c_{N-1}.  A grid with an axis of fewer than 2 voxels has no domain.
 *   sample k   t_0 = t_in, t_{k+1} = t_k + s_k, p = o + t_k u (formed afresh), while t_k <= t_out.  Cell i = clamp(floor(p_a / voxel - 0.5), 0,
 *              N_a - 2), fraction f = clamp((p_a - c_i) / (c_{i+1} - c_i), 0, 1); D_k the trilinear tsdf (lerp a + f (b - a): x, then y, then z).
 *              Known iff all eight corners have weight >= min_weight.
 *   step       s_k = far_step when the sample is known and all eight corners hold exactly 1.0f, else step.  0 < step <= far_step < trunc: a known
 *              sample whose corners are all 1.0f lies at least trunc in front of a Euclidean surface, so a step shorter than trunc skips no crossing.
 *   hit        the first k with samples k-1 and k known, D_{k-1} > 0 and D_k <= 0: w = D_{k-1} / (D_{k-1} - D_k), t* = t_{k-1} + (t_k - t_{k-1}) w,
 *              depth = (float) t*; intensity = I_{k-1} + (I_k - I_{k-1}) w from each sample's own cell.  A miss writes depth 0, hit 0, intensity 0.
 *   samples    the number of samples evaluated (at a hit: up to and including sample k).
 *
 * lrt_raycast: one launch, one lane per ray (rays in memory order), no LDS, no atomics; N == 0 launches nothing.  The grid is not changed and every
 * output element is written.  The arguments are checked before the device is touched: 0 < step <= far_step < trunc (finite), 0 <= min_depth <
 * max_depth (finite), max_depth + step > max_depth in float64 (every step advances t), and the grid's diagonal voxel |(X, Y, Z)| at most
 * LRT_RAYCAST_MAX_SAMPLES steps (a bound on the samples of a ray).
 *
 * Conventions: as in lrt_mesh.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`, no
 * allocation and no host wait inside a call.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_raycast_last_error(); a refused call
 * launches nothing.
 */
#ifndef LRT_RAYCAST_H_INCLUDED
#define LRT_RAYCAST_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_RAYCAST_ABI_VERSION 1
#define LRT_RAYCAST_BLOCK 256                 /* rays per workgroup */
#define LRT_RAYCAST_MAX_VOXELS 2147483647LL   /* X Y Z, as LRT_MESH_MAX_VOXELS */
#define LRT_RAYCAST_MAX_RAYS 2147483647LL     /* N */
#define LRT_RAYCAST_MAX_SAMPLES 16777216      /* the grid's diagonal / step */

int lrt_raycast_abi_version(void);

/* Message of the calling thread's last failed lrt_raycast call. */
const char* lrt_raycast_last_error(void);

/* tsdf, weight (X, Y, Z) float32 / int32, intensity (X, Y, Z) float32 or NULL; min_weight >= 1; ray_o, ray_d (N, 3) float32 in the world;
 * depth (N) float32, hit (N) uint8, out_intensity (N) float32 given iff intensity is (for N == 0 it may be NULL), samples (N) int32 or NULL. */
int lrt_raycast(int device, int X, int Y, int Z, double voxel, double trunc, double origin_x, double origin_y, double origin_z, const float* tsdf,
                const int* weight, const float* intensity, int min_weight, long long N, const float* ray_o, const float* ray_d, double step,
                double far_step, double min_depth, double max_depth, float* depth, unsigned char* hit, float* out_intensity, int* samples,
                void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_RAYCAST_H_INCLUDED */
