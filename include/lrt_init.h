/*
 * lrt_init.h -- C ABI of the scene initialisation from range images (liblrt_init.so, a library of its own next to liblrt_hip.so,
 * liblrt_loss.so and liblrt_gridcd.so): per-return normals from an exact k-nearest-neighbour search on the ray grid, the split of a frame's
 * returns by tracking box, and the voxel mean of a cloud.  What the reference does with Open3D on the CPU before its training loop starts.
 *
 * 1. lrt_init_normals.  A frame's cloud is o + d * range over the pixels with mask != 0 of an (H, W) ray grid, so the image is the spatial
 *    index (as in lrt_gridcd.h): no sort, no tree.  Per valid pixel
 *
 *      nbr[h, w, 0..k-1] = the k smallest (squared distance, linear pixel index) pairs over ALL valid pixels of the frame, ascending
 *
 *    the pixel itself included (distance 0), duplicated points at distance 0, ties to the lower pixel index; -1 beyond k or beyond the number
 *    of valid pixels, and all -1 for an invalid pixel.  The list does not depend on the visiting order: it equals a brute-force scan exactly.
 *    Arithmetic: a point is fadd(o, fmul(d, r)), two roundings, no contraction; a pair's squared distance is
 *    fma(dz, dz, fma(dy, dy, dx * dx)) with d = candidate - query in float32 (lrt_gridcd.h).
 *
 *      normal[h, w] = the unit eigenvector of the smallest eigenvalue of the covariance of the listed points about their mean
 *
 *    formed in float64 (csrc/lrt_init_math.h: closed form), rounded once to float32, then turned to face the sensor:
 *    dot(n, rays_o - p) >= 0, and where that is exactly 0 the first non-zero component is positive.  Fewer than 3 listed points or a
 *    covariance of rank < 2: (0, 0, 1).  Invalid pixels: zeros.
 *
 * 2. lrt_init_assign.  A pixel's point belongs to the FIRST actor a with present[a] != 0 for which |R_a^T (p - t_a)| < size_a / 2 holds on
 *    every axis (strict, float32; R_a from pose[a] = [t, q_wxyz] with the quaternion normalised first).  label = -1 (invalid pixel),
 *    0 (background) or a + 1; local_point / local_normal hold the actor-frame values where label > 0 and the inputs unchanged elsewhere.
 *    A = 0 is allowed (pose / size / present may then be null).
 *
 * 3. lrt_init_voxel_keys, lrt_init_voxel_mean.  Voxel origin = the cloud's componentwise minimum - voxel_size / 2; voxel index =
 *    floor((p - origin) / voxel_size) per axis in float64; key = ix << 42 | iy << 21 | iz (int64).  An index outside [0, 2^21) sets
 *    info[1] = LRT_INIT_KEY_RANGE instead of wrapping.  The caller sorts the keys STABLY (key, input index) and passes the sorted keys and
 *    the permutation to lrt_init_voxel_mean, which writes one row per occupied voxel in ascending key order -- the mean point, intensity and
 *    normal (not renormalised), each summed in float64 in ascending input index and rounded once, and the count -- zeros in the rows from
 *    M to N - 1, and info[0] = M.  info: two int32 on the device; the caller reads it once, after the last call.
 *
 * Conventions: as in lrt_gridcd.h -- device pointers to contiguous float32 (masks: uint8, 0 / non-zero; indices: int32; keys: int64),
 * stream-ordered on `device`, no allocation and no host wait inside a call, 0 or a negative code (the LRT_ERR_* values of lrt.h) with
 * lrt_init_last_error().  `work` is a caller-owned device buffer of at least lrt_init_*_work_bytes bytes, 16-byte aligned, scratch only
 * (except that lrt_init_voxel_mean needs no state from lrt_init_voxel_keys).  No float atomics: two calls return the same bits.  Every output
 * element is written exactly once, zeros included: the buffers need no clearing.
 */
#ifndef LRT_INIT_H_INCLUDED
#define LRT_INIT_H_INCLUDED

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_INIT_ABI_VERSION 1
#define LRT_INIT_KMAX 8
#define LRT_INIT_KEY_RANGE 1 /* info[1]: a voxel index does not fit into 21 bits */

int lrt_init_abi_version(void);

/* Message of the calling thread's last failed lrt_init_* call. */
const char* lrt_init_last_error(void);

/* Bytes of the workspace of lrt_init_normals for an H x W image (0 for an invalid size). */
size_t lrt_init_normals_work_bytes(int H, int W);

/* Bytes of the workspace of the two voxel calls for N points (0 for an invalid N). */
size_t lrt_init_voxel_work_bytes(long long N);

/* rays_o, rays_d (H, W, 3); range (H, W); mask (H, W) uint8; 3 <= k <= 8; nbr (H, W, 8) int32; normal (H, W, 3). */
int lrt_init_normals(int device, int H, int W, const float* rays_o, const float* rays_d, const float* range, const uint8_t* mask, int k,
                     int32_t* nbr, float* normal, void* work, size_t work_bytes, void* stream);

/* n pixels: point, normal (n, 3); mask (n) uint8; pose (A, 7); size (A, 3); present (A) uint8; label (n) int32; local_* (n, 3). */
int lrt_init_assign(int device, long long n, const float* point, const float* normal, const uint8_t* mask, int A, const float* pose,
                    const float* size, const uint8_t* present, int32_t* label, float* local_point, float* local_normal, void* stream);

/* points (N, 3); keys (N) int64; info: 2 x int32 (info[1] is written here: 0 or LRT_INIT_KEY_RANGE). */
int lrt_init_voxel_keys(int device, long long N, const float* points, double voxel_size, int64_t* keys, int32_t* info, void* work,
                        size_t work_bytes, void* stream);

/* sorted_keys (N) int64 ascending, perm (N) int32: the stable sort's permutation; points, normals (N, 3), intensity (N): the UNSORTED cloud;
 * out_points, out_normals (N, 3), out_intensity (N), count (N) int32: M rows and N - M rows of zeros; info[0] = M. */
int lrt_init_voxel_mean(int device, long long N, const int64_t* sorted_keys, const int32_t* perm, const float* points, const float* intensity,
                        const float* normals, float* out_points, float* out_intensity, float* out_normals, int32_t* count, int32_t* info,
                        void* work, size_t work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_INIT_H_INCLUDED */
