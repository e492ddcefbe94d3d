/*
 * lrt_sweepfuse.h -- C ABI of the TSDF fusion of range images of a MOVING sensor (liblrt_sweepfuse.so, a twentieth library next to
 * liblrt_raycast.so and the eighteen others): lrt_mesh_integrate with every voxel centre projected under the sweep model, so that the grid a
 * driving sequence is fused into is not sheared by the sensor's motion within a sweep.
 *
 * lidar_rt_amd/csrc/lrt_sweepfuse_math.h is the text of the rule for the device and the host (float64 with contraction off).  It adds nothing
 * of its own to the arithmetic: the voxel centre and the update are lrt_mesh_math.h's (mh_centre, mh_fuse's operations), the column search and
 * the drop class are lrt_sweepproj_math.h's (sp_search, sp_classify), so a voxel takes the pixel that project_points_sweep gives its centre as
 * a point.  The grid is the one of lrt_mesh.h: dense, C-order (X, Y, Z), voxel v = (i Y + j) Z + k, tsdf float32, weight int32, intensity
 * float32 (optional), owned by the caller and updated in place.
 *
 * Per voxel, per frame f in ascending order:
 *   1. c = mh_centre per axis; p = pj_transform(grid2sensor[f], c), the centre in the sensor frame of the frame's REFERENCE instant.  A p that is
 *      not finite: the frame does not take part.
 *   2. sp_search(p, table_f, R, q, &w, &evals) with R.wrap = 1: the fixed-point search from the static column, at most LRT_SWEEPFUSE_MAX_EVAL
 *      evaluations.  table_f[w] = sp_column_entry(twist[f], tau[w]), the inverse of Exp(tau[w] twist[f]) as a row-major 3 x 4.
 *   3. sp_classify(q, state, R, inclination, &h, &r32): the voxel takes part iff the class is PJ_KEEP, mask[h, w] is set and depth[h, w] > 0.  An
 *      unseen (the search did not converge), out-of-view, out-of-range or invalid centre is skipped for this frame.
 *   4. sdf = (double) depth - (double) r32, skipped below -trunc; d = min(1, sdf / trunc); D = (Wt D + d) / (Wt + 1), I likewise, Wt += 1.  D, I
 *      and Wt are float64 across the frames of a call and rounded once at its end; a voxel that no frame sees keeps its bits.  r32 is measured
 *      from the origin of the column that sees the voxel, at that column's own instant: that is the compensation.
 *   5. twist == NULL, or a frame whose twist is all zeros: every table entry is exactly the identity, sp_to_column returns p itself, and the
 *      frame's contribution equals lrt_mesh_integrate's bit for bit.
 *
 * lrt_sweepfuse_integrate: two launches (the column table into the workspace, then one lane per voxel), none for F == 0.  No allocation, no host
 * wait, no atomics.  Memory safety does not depend on the values in twist, tau, inclination, the images or the workspace: a column that
 * arithmetic produced is range-checked before it indexes the table (a NaN included), a pixel outside its image is never read, and the table is
 * written inside the call, so a stale workspace does not leak.
 *
 * Conventions: as in lrt_mesh.h and lrt_sweepproj.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on
 * `stream` of `device`.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_sweepfuse_last_error(); the arguments are checked before
 * the device is touched and a refused call launches nothing.
 */
#ifndef LRT_SWEEPFUSE_H_INCLUDED
#define LRT_SWEEPFUSE_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_SWEEPFUSE_ABI_VERSION 1
#define LRT_SWEEPFUSE_BLOCK 256                 /* voxels per workgroup: LRT_MESH_BLOCK */
#define LRT_SWEEPFUSE_MAX_EVAL 8                /* evaluations of a search: LRT_SWEEPPROJ_MAX_EVAL */
#define LRT_SWEEPFUSE_TABLE 12                  /* doubles per column of the table: LRT_SWEEPPROJ_TABLE */
#define LRT_SWEEPFUSE_MAX_VOXELS 2147483647LL   /* X Y Z, and F H W: LRT_MESH_MAX_VOXELS */
#define LRT_SWEEPFUSE_MAX_FRAMES 65536          /* frames per call: LRT_MESH_MAX_FRAMES */

int lrt_sweepfuse_abi_version(void);

/* Message of the calling thread's last failed lrt_sweepfuse_* call. */
const char* lrt_sweepfuse_last_error(void);

/* Bytes of the workspace of a call with F frames of W columns: the column table, F W 96 bytes rounded up to 256; negative for F < 0,
 * F > LRT_SWEEPFUSE_MAX_FRAMES or W < 1. */
long long lrt_sweepfuse_work_bytes(long long F, int W);

/* The arguments of lrt_mesh_integrate, then: twist (F, 6) float64 (rho, phi), the sensor's motion over one sweep in the sensor frame, or NULL (a
 * static sensor); tau (W) float64, the instant of every column in sweeps, required with a twist; workspace: 256-byte aligned, at least
 * lrt_sweepfuse_work_bytes(F, W). */
int lrt_sweepfuse_integrate(int device, int X, int Y, int Z, double voxel, double trunc, float* tsdf, int* weight, float* intensity, long long F,
                            const double* grid2sensor, int H, int W, const float* depth, const unsigned char* mask, const float* frame_intensity,
                            const double* inclination, int n_inc, double off, double yaw, double min_depth, double max_depth, const double* twist,
                            const double* tau, void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_SWEEPFUSE_H_INCLUDED */
