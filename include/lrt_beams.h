/*
 * lrt_beams.h -- C ABI of the beam rays (liblrt_beams.so, a library of its own next to liblrt_sweep.so and the twelve others).
 *
 * The sweep rays (lrt_sweep.h) of a sensor whose lasers are not where the nominal grid puts them: image row h has an elevation offset eps_h and
 * an azimuth offset delta_h, in radians, beams[h] = (eps_h, delta_h).  The table is indexed by the image row; it is NOT flipped the way the
 * per-beam inclination table is.  For frame f, row h, column w, with R_w, t_w the pose T_f(tau[w]) = P_f Exp(tau[w] xi_f) of the column:
 *
 *     e = inclination(h) + eps_h,  a = azimuth(w) + delta_h,  l = (cos e cos a, cos e sin a, sin e)
 *     ray_d[f, h, w] = float32(R_w l / |R_w l|)        ray_o[f, h, w] = float32(t_w)
 *
 * The origins are the sweep rays': a column still fires at tau[w]; the offsets say how a laser is mounted, not when it fires.  A row whose two
 * offsets are exactly zero carries the bits of lrt_sweep_rays.  lidar_rt_amd/csrc/lrt_beams_math.h holds the text; all of it float64, each
 * component rounded once.  A table value indexes nothing: a non-finite offset gives non-finite rays and gradients and nothing else.
 *
 *   lrt_beams_work_bytes   the size of the workspace for F frames of H x W.
 *   lrt_beams_rays         two launches: the per-column table (Exp, the azimuth's sine and cosine and the three axes they give, once per column)
 *                          and the per-row table (sine and cosine of the offset elevation and of the azimuth offset, once per row) in float64;
 *                          then one thread per output component, coalesced stores.
 *   lrt_beams_backward     two launches: from g_o, g_d (F, H, W, 3) to d_pose (F, 3, 4), d_twist (F, 6) and d_beams (H, 2), the normalisation
 *                          included.  One wave per LRT_SWEEP_COLS columns of a frame, one thread per column.  A thread sums its column's rows in
 *                          row order and chains the sums through dExp/dxi; the wave sums its columns.  Each row's two beam terms are summed over
 *                          the wave's columns by a butterfly and written as float64 partials per (frame, column block, row).  The finishing
 *                          launch adds a frame's workgroups in order for d_pose and d_twist, and a row's partials in ascending (frame, block)
 *                          order for d_beams.  All sums in float64 in a fixed order, no float atomics, each result rounded to float32 once.
 *                          An output that is not asked for costs no reduction, and the others keep their bits.
 *
 * Conventions: as in lrt_sweep.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`,
 * no allocation and no host wait inside a call, every output element is written, the inputs are not changed.  What a call reads from the
 * workspace it has written before, so a stale workspace does not leak.  0 or a negative code (the LRT_ERR_* values of lrt.h) with
 * lrt_beams_last_error(); the arguments are checked before the device is touched and a refused call launches nothing.
 */
#ifndef LRT_BEAMS_H_INCLUDED
#define LRT_BEAMS_H_INCLUDED

#include "lrt_sweep.h"                     /* LRT_SWEEP_BLOCK, LRT_SWEEP_COLS, LRT_SWEEP_MAX_RAYS hold here too */

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_BEAMS_ABI_VERSION 1

int lrt_beams_abi_version(void);

/* Message of the calling thread's last failed lrt_beams_* call. */
const char* lrt_beams_last_error(void);

/* Bytes of the workspace for F frames of H x W rays (a multiple of 256); negative for F, H, W < 1 or F * H * W > LRT_SWEEP_MAX_RAYS. */
long long lrt_beams_work_bytes(long long F, int H, int W);

/* pose, twist, inclination, n_inc, off, yaw, tau: as in lrt_sweep_rays.  beams (H, 2) float32: (eps_h, delta_h) of image row h, required.
 * ray_o, ray_d (F, H, W, 3) float32.  workspace: 256-byte aligned device memory of work_bytes >= lrt_beams_work_bytes(F, H, W). */
int lrt_beams_rays(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                   double off, double yaw, const float* tau, const float* beams, float* ray_o, float* ray_d, void* workspace, long long work_bytes,
                   void* stream);

/* The same inputs, plus g_o, g_d (F, H, W, 3) float32.  d_pose (F, 3, 4) float32 or NULL; d_beams (H, 2) float32 or NULL; at least one of the
 * two.  d_twist (F, 6) float32 goes with d_pose: required with a twist; without one it may be NULL, and is set to zero where it is given; it
 * must be NULL when d_pose is. */
int lrt_beams_backward(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                       double off, double yaw, const float* tau, const float* beams, const float* g_o, const float* g_d, float* d_pose,
                       float* d_twist, float* d_beams, void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_BEAMS_H_INCLUDED */
