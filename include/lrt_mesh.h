/*
 * lrt_mesh.h -- C ABI of the surface meshes from range images (liblrt_mesh.so, an eighteenth library next to liblrt_place.so and the sixteen
 * others): projective TSDF fusion of posed range images into a dense grid, and marching cubes over that grid.  The image is the index: every voxel
 * centre is projected into every range image, with no tree and no sort.
 *
 * lidar_rt_amd/csrc/lrt_mesh_math.h is the text of every rule for the device and the host (float64 with contraction off); the projection of a
 * voxel centre is lrt_project_math.h itself, so a voxel takes the pixel that project_points gives its centre as a point.
 *
 * The grid is dense, axis-aligned, C-order (X, Y, Z): voxel v = (i Y + j) Z + k, X Y Z <= 2^31 - 1.  Voxel centre c = (float) (voxel (i + 0.5))
 * per axis, in the grid frame.  The caller owns the state: tsdf float32, weight int32 (0 = unobserved), intensity float32 (optional).  A fresh grid
 * is all zeros.
 *
 *   lrt_mesh_integrate   one launch, one lane per voxel, the frames in ascending order inside the lane.  Per frame f: q = grid2sensor[f] c,
 *       pj_classify(q): a voxel takes part iff the point is kept, mask[h, w] is set and depth[h, w] > 0; sdf = depth - r32, skipped if sdf < -trunc;
 *       d = min(1, sdf / trunc); D = (Wt D + d) / (Wt + 1), I = (Wt I + i) / (Wt + 1), Wt += 1, held in float64 across the frames of the call and
 *       rounded to float32 once at its end.  A voxel that no frame sees keeps its bits.  The state arrays are updated in place (the one exception
 *       to "the inputs are not changed").  F == 0 launches nothing.
 *   lrt_mesh_count       two launches: each voxel's owned-edge mask and counts, then a scan of the workgroups' counts; totals (2) int64 = V, T.
 *   lrt_mesh_write       two launches: the vertices (and each voxel's vertex and triangle offsets, in the workspace), then the faces.
 *       An observed corner has weight >= min_weight; an active cell (i < X-1, j < Y-1, k < Z-1) has 8 observed corners; a crossed edge (v, axis) has
 *       two observed ends of which exactly one has tsdf < 0; an emitted edge is crossed and touches an active cell.  vertices (V, 3) float32, one per
 *       emitted edge ascending by (v, axis): t = d_a / (d_a - d_b), p = c_a + t (c_b - c_a) in float64, rounded once; vertex_intensity (V) the same
 *       interpolation of the corner intensities (NULL: none).  faces (T, 3) int32 ascending by cell, then in the order of csrc/lrt_mesh_tables.h;
 *       (v1 - v0) x (v2 - v0) points from negative to positive tsdf.
 *
 * Conventions: as in lrt_place.h -- every data pointer is a device pointer to contiguous memory, all work is ordered on `stream` of `device`, no
 * allocation and no host wait inside a call, no float atomics, every output element is written.  The caller reads the two totals once, between
 * lrt_mesh_count and lrt_mesh_write, to size the outputs.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_mesh_last_error(); the
 * arguments are checked before the device is touched and a refused call launches nothing.
 */
#ifndef LRT_MESH_H_INCLUDED
#define LRT_MESH_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_MESH_ABI_VERSION 1
#define LRT_MESH_BLOCK 256                 /* voxels per workgroup of every launch */
#define LRT_MESH_SCAN_PASS 256             /* workgroup counts per pass of the scan (one workgroup walks them in passes) */
#define LRT_MESH_MAX_VOXELS 2147483647LL   /* X Y Z */
#define LRT_MESH_MAX_FRAMES 65536          /* frames per integrate call */
#define LRT_MESH_MAX_OUTPUT 2147483647LL   /* V and T: a vertex id and a face row are int32 */

int lrt_mesh_abi_version(void);

/* Message of the calling thread's last failed lrt_mesh_* call. */
const char* lrt_mesh_last_error(void);

/* grid2sensor (F, 3, 4) float64; depth (F, H, W) float32; mask (F, H, W) uint8; frame_intensity (F, H, W) float32 or NULL, given iff intensity is;
 * inclination n_inc float64 (2 bounds or H >= 3 beams, as lrt_project_points); off, yaw as range_image.convention; 0 <= min_depth < max_depth;
 * voxel > 0, trunc > 0. */
int lrt_mesh_integrate(int device, int X, int Y, int Z, double voxel, double trunc, float* tsdf, int* weight, float* intensity, long long F,
                       const double* grid2sensor, int H, int W, const float* depth, const unsigned char* mask, const float* frame_intensity,
                       const double* inclination, int n_inc, double off, double yaw, double min_depth, double max_depth, void* stream);

/* Bytes of the extraction's workspace for an X x Y x Z grid (a multiple of 256); negative for a dimension < 1 or X Y Z > LRT_MESH_MAX_VOXELS. */
long long lrt_mesh_work_bytes(int X, int Y, int Z);

/* workspace: 256-byte aligned, at least lrt_mesh_work_bytes; totals (2) int64 device memory. */
int lrt_mesh_count(int device, int X, int Y, int Z, const float* tsdf, const int* weight, int min_weight, void* workspace, long long work_bytes,
                   long long* totals, void* stream);

/* The workspace lrt_mesh_count filled and the totals V, T it wrote (each at most LRT_MESH_MAX_OUTPUT); intensity and vertex_intensity both or
 * neither. */
int lrt_mesh_write(int device, int X, int Y, int Z, double voxel, const float* tsdf, const float* intensity, void* workspace, long long work_bytes,
                   long long V, long long T, float* vertices, float* vertex_intensity, int* faces, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_MESH_H_INCLUDED */
