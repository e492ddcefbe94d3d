/*
 * lrt_place.h -- C ABI of the place matcher (liblrt_place.so, a seventeenth library next to liblrt_segment.so and the fifteen others): one small
 * descriptor per scan and every scan against every earlier scan at every yaw -- what lidar_rt_amd/pose_graph.py turns into the loop edges of a
 * pose graph over the odometry of lidar_rt_amd/registration.py.  The image is the index: a sector is a band of columns, there is no atan2.
 *
 * lidar_rt_amd/csrc/lrt_place_math.h is the text of every rule for the device and the host (float64 with contraction off).  EVERY RESULT IS AN
 * INTEGER that does not depend on the order in which lanes arrive: the numpy twins are exact.
 *
 *   lrt_place_describe   one launch, one workgroup per frame.  points (F, H, W, 3) float32 sensor-frame points, mask (F, H, W) uint8.  For a
 *       valid pixel h = up . p summed x, y, z; g = p - h up; rho = sqrt(gx gx + gy gy + gz gz).  The pixel is kept iff r_min <= rho < r_max and
 *       h >= z_lo (a NaN keeps nothing).  ring = min(NR - 1, floor((rho - r_min) * NR / (r_max - r_min))); sector = (w * NS) / W in integers;
 *       value = min(255, 1 + floor((h - z_lo) / z_step)).  A cell keeps the maximum over its pixels, 0 for an empty cell (integer atomicMax on
 *       32-bit words in LDS, packed to bytes once per frame).
 *       desc (F, NS, NRP) uint8, sector-major, NRP = NR rounded up to a multiple of 4 (the padding is 0): a sector is NRP / 4 dwords and a yaw
 *       is a contiguous offset.  sum (F) int32: the sum of a descriptor's bytes.
 *   lrt_place_match      one launch.  For every query i and candidate j with j + gap <= i
 *           D(i, j, s) = sum over cells |a_i[r, (c + s) mod NS] - a_j[r, c]|,   s in [0, NS)
 *       best_d (F, F) int32 = min over s, best_s (F, F) int32 = the lowest s that attains it; -1 in both for a pair outside the triangle.
 *       D <= 255 * 32 * 128 < 2^20, so the key D << 7 | s fits a word and the minimum with its tie rule is one butterfly of integer min.
 *
 * Conventions: as in lrt_segment.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`,
 * no allocation and no host wait inside a call, no float atomics, every output element is written, the inputs are not changed.  0 or a negative
 * code (the LRT_ERR_* values of lrt.h) with lrt_place_last_error(); the arguments are checked before the device is touched and a refused call
 * launches nothing.
 */
#ifndef LRT_PLACE_H_INCLUDED
#define LRT_PLACE_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_PLACE_ABI_VERSION 1
#define LRT_PLACE_BLOCK 256               /* lanes per workgroup of lrt_place_match: four waves */
#define LRT_PLACE_DESCRIBE_BLOCK 512      /* lanes per workgroup of lrt_place_describe */
#define LRT_PLACE_TILE 16                 /* candidates per workgroup of lrt_place_match: four per wave, side by side */
#define LRT_PLACE_MAX_RINGS 32
#define LRT_PLACE_MAX_SECTORS 128
#define LRT_PLACE_MAX_FRAMES 32768        /* F F fits an int32 index with room to spare */
#define LRT_PLACE_MAX_PIXELS 715827882LL  /* F H W at most (2^31 - 1) / 3 */

int lrt_place_abi_version(void);

/* Message of the calling thread's last failed lrt_place_* call. */
const char* lrt_place_last_error(void);

int lrt_place_describe(int device, long long F, int H, int W, const float* points, const unsigned char* mask, int NR, int NS, double up_x,
                       double up_y, double up_z, double r_min, double r_max, double z_lo, double z_step, unsigned char* desc, int* sum,
                       void* stream);

/* desc (F, NS, NRP) uint8 as lrt_place_describe writes it (4-byte aligned); 0 <= gap. */
int lrt_place_match(int device, long long F, int NR, int NS, const unsigned char* desc, long long gap, int* best_d, int* best_s, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_PLACE_H_INCLUDED */
