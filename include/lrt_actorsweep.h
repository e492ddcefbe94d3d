/*
 * lrt_actorsweep.h -- C ABI of actors that move within a sweep (liblrt_actorsweep.so, a library of its own next to liblrt_sweep.so and
 * liblrt_sweepproj.so): a stage IN FRONT of lrt_preprocess_forward that advances the actor-local parameters of every Gaussian of a moving actor
 * to the instant at which the sweep passes over its centre.
 *
 * Over one sweep an actor moves as A(s) = A Exp(s eta): A the tracking-box pose at the frame's reference instant (the `poses` row of
 * lrt_preprocess.h, its quaternion normalised as build_rotation does), eta = (rho, phi) the actor's twist over one whole sweep in its OWN frame
 * (the convention of lrt_sweep.h), s in sweeps.  Column w of the sensor is fired at tau[w] from P Exp(tau[w] xi).  A Gaussian with the local
 * centre x is placed at s* = tau[w*], where w* is the column that, at its own instant, has the centre inside its azimuth bin:
 *
 *   y(w) = A Exp(tau[w] eta) x,   q(w) = (P Exp(tau[w] xi))^-1 y(w),   w* : rint(u(q(w*))) mod W == w*     (u: lrt_sweepproj.h's column rule, wrapped)
 *
 * The search is lrt_sweepproj.h's fixed-point iteration: it starts at the static column of A x as the sensor sees it at s = 0 and makes at most
 * LRT_ACTORSWEEP_MAX_EVAL evaluations.  A search that does not converge keeps the LAST evaluated column (any instant of the sweep is a valid
 * placement) and is counted as `unconverged`.  A q that is not finite or lies on the z axis (x == y == 0) in any evaluation ends the search: the
 * Gaussian passes through with column -1 and is counted as `invalid`.
 *
 *   xyz_s = float32(R_E x + t_E)                          E = Exp(s* eta) = [R_E | t_E]
 *   rot_s = float32(q_E (x) raw / max(|raw|, 1e-12))      q_E the unit quaternion of R_E (half-angle form, the series near zero)
 *   column = w*                                           int32, -1 for a Gaussian that was not searched or is invalid
 *
 * Pass-through is bit for bit (xyz_s = xyz, rot_s = rot_raw NOT normalised): every Gaussian of an unposed asset (poses[a][7] == 0) and of an
 * asset whose twist row is all zeros (neither is searched: column -1), and every Gaussian whose s* eta is zero in all six entries (E is exactly
 * the identity; tau[w*] == 0), which still records its column.  The instants are piecewise constant in every input, so the backward treats
 * them as constants: it reads the saved columns and does not search again.
 *
 *   lrt_actorsweep_work_bytes   the workspace: the column table (W x 12 float64) and the backward's partial sums (6 float64 per workgroup + asset).
 *   lrt_actorsweep_forward      two launches: the column table (which also clears the counts), then one thread per Gaussian.
 *   lrt_actorsweep_backward     two launches: one thread per Gaussian writes d_xyz and d_rot_raw and reduces its term of d_actor_twist over the
 *                               workgroup per asset (float64, fixed order); one workgroup per asset adds the partials in a fixed order and
 *                               rounds once.  No float atomics: equal inputs give equal bits.
 *
 * counts (4) int64 = moved, passed, unconverged, invalid; moved + passed == P; unconverged and invalid are subsets of the two.  They are formed
 * by ballots and 64-bit integer adds, which commute.
 *
 * Conventions: every data pointer is a device pointer to contiguous memory; rot_raw, rot_s, g_rot_s and d_rot_raw are 16-byte aligned (their rows
 * are read and written as float4; a misaligned one is refused), all work is ordered on `stream` of `device`, no allocation and no
 * host wait inside a call.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_actorsweep_last_error(); the arguments are checked
 * before the device is touched and a refused call launches nothing.  Memory safety does not depend on the values in seg_start, tau, the twists,
 * the saved columns or the points: a column that arithmetic produced or that was read back is range-checked before it indexes anything (a NaN
 * included), and an asset or a partial-sum row outside its array is never touched.
 */
#ifndef LRT_ACTORSWEEP_H_INCLUDED
#define LRT_ACTORSWEEP_H_INCLUDED

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_ACTORSWEEP_ABI_VERSION 1
#define LRT_ACTORSWEEP_N_COUNTS 4
#define LRT_ACTORSWEEP_MAX_EVAL 8              /* evaluations of the column search per Gaussian */
#define LRT_ACTORSWEEP_TABLE 12                /* float64 per column: world -> the column's sensor frame, row-major 3 x 4 */
#define LRT_ACTORSWEEP_BLOCK 256               /* Gaussians or columns per workgroup */
#define LRT_ACTORSWEEP_MAX_POINTS 1073741824LL /* Gaussians per call (seg_start is int32) */
#define LRT_ACTORSWEEP_MAX_ASSETS 1048576
#define LRT_ACTORSWEEP_MAX_COLUMNS 1048576

int lrt_actorsweep_abi_version(void);

/* Message of the calling thread's last failed lrt_actorsweep_* call. */
const char* lrt_actorsweep_last_error(void);

/* Bytes of the workspace: W 96 for the column table, rounded up to a multiple of 256, plus 48 ((P + 255) / 256 + A) for the partial sums,
 * rounded up likewise; negative for P < 0, A < 1, W < 1 or one of them above its maximum. */
long long lrt_actorsweep_work_bytes(long long P, int A, int W);

/* xyz (P, 3), rot_raw (P, 4) float32; seg_start (A + 1) int32; poses (A, 8) float32 (lrt_preprocess.h); actor_twist (A, 6) float32;
 * world2sensor (3, 4) float64 = P^-1; sensor_twist (6) float64 or NULL (a static sensor); tau (W) float64; off, yaw: the column rule's
 * (lrt_project.h).  Outputs, every element written: xyz_s (P, 3), rot_s (P, 4) float32, column (P) int32, counts (4) int64.
 * workspace: 256-byte aligned device memory of work_bytes >= lrt_actorsweep_work_bytes(P, A, W). */
int lrt_actorsweep_forward(int device, long long P, int A, const float* xyz, const float* rot_raw, const int32_t* seg_start, const float* poses,
                           const float* actor_twist, const double* world2sensor, const double* sensor_twist, const double* tau, int W, double off,
                           double yaw, float* xyz_s, float* rot_s, int32_t* column, long long* counts, void* workspace, long long work_bytes,
                           void* stream);

/* column (P): what the forward wrote.  g_xyz_s (P, 3), g_rot_s (P, 4) float32.  Outputs, overwritten: d_xyz (P, 3), d_rot_raw (P, 4) (the rows
 * of passing Gaussians are copies), d_actor_twist (A, 6) float32 (the rows of unposed, empty and zero-twist assets are zero). */
int lrt_actorsweep_backward(int device, long long P, int A, const float* xyz, const float* rot_raw, const int32_t* seg_start, const float* poses,
                            const float* actor_twist, const double* tau, int W, const int32_t* column, const float* g_xyz_s, const float* g_rot_s,
                            float* d_xyz, float* d_rot_raw, float* d_actor_twist, void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_ACTORSWEEP_H_INCLUDED */
