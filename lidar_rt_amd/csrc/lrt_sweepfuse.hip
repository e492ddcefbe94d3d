// lrt_sweepfuse.hip -- TSDF fusion of range images of a moving sensor (include/lrt_sweepfuse.h), gfx950.  Compiled into liblrt_sweepfuse.so, a
// library of its own.  No allocation, no host wait, no atomics; the rule per voxel and frame is lrt_sweepfuse_math.h, which is lrt_mesh_math.h's
// update behind lrt_sweepproj_math.h's column search.
//
//   k_sf_table   one thread per frame and column: sp_column_entry(twist[f], tau[w]), the inverse of Exp(tau[w] twist[f]) as 12 doubles in the
//                workspace -- formed exactly as liblrt_sweepproj.so forms its table, so the device's entries are the ones project_points_sweep
//                uses.  Without a twist every entry is the identity.  The whole table is written in every call: a stale workspace is never read.
//   k_sf_fuse    one lane per voxel, LRT_SWEEPFUSE_BLOCK lanes per workgroup.  The lane holds D, I, Wt in float64 registers and walks the frames in
//                ascending order; a frame's transform is wave-uniform (scalar loads), its table entries and its pixel are per-lane gathers.  The
//                voxel order is the grid's C order (X, Y, Z): consecutive lanes differ in k only, so they share x and y, hence the azimuth and
//                nearly always the column -- the 96-byte table gather is close to wave-uniform and its lines are shared by the wave.  Keep that
//                order.  One store per state array, only for a voxel some frame saw.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_sweepfuse_math.h"
#include "../../include/lrt_sweepfuse.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_SWEEPFUSE_BLOCK;
static_assert(SP_MAX_EVAL == LRT_SWEEPFUSE_MAX_EVAL && SP_TABLE == LRT_SWEEPFUSE_TABLE, "the rule's header and the C ABI disagree");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

// ---- table ------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_sf_table(long long n_cols, int W, const double* __restrict__ twist, const double* __restrict__ tau, double* __restrict__ table)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n_cols) return;
    double E[SP_TABLE];
    if (twist) {
        const long long f = i / W;
        const int w = (int)(i - f * W);
        double xi[6];
        for (int k = 0; k < 6; k++) xi[k] = twist[6 * f + k];
        sp_column_entry(xi, tau[w], E);
    } else {
        sf_identity(E);
    }
    for (int k = 0; k < SP_TABLE; k++) table[SP_TABLE * i + k] = E[k];
}

// ---- fuse -------------------------------------------------------------------------------------------------------------------------------------------------
struct FuseArgs {
    int X, Y, Z, F;
    long long N, HW;
    double voxel, trunc;
    PjRule rule;
    float* tsdf;
    int* weight;
    float* intensity;
    const float* depth;
    const unsigned char* mask;
    const float* fint;
    const double* inc;
};

// T is a parameter of its own, const and restrict: frame f's twelve entries are wave-uniform loads the compiler may issue as scalar ones.  The table
// was written by the launch before this one on the same stream.
__global__ __launch_bounds__(NT) void k_sf_fuse(FuseArgs a, const double* __restrict__ T, const double* __restrict__ table)
{
    const long long g = (long long)blockIdx.x * NT + threadIdx.x;
    if (g >= a.N) return;
    const int v = (int)g;
    const int YZ = a.Y * a.Z;
    const int i = v / YZ, r = v - i * YZ, j = r / a.Z, k = r - j * a.Z;
    const float cx = mh_centre(a.voxel, i), cy = mh_centre(a.voxel, j), cz = mh_centre(a.voxel, k);
    double D = (double)a.tsdf[v], Wt = (double)a.weight[v], I = a.intensity ? (double)a.intensity[v] : 0.0;
    int seen = 0;
    for (int f = 0; f < a.F; f++) {
        const long long o = (long long)f * a.HW;
        MhFrame fr;
        fr.depth = a.depth + o; fr.mask = a.mask + o; fr.intensity = a.fint ? a.fint + o : nullptr;
        int cls, evals;
        seen |= sf_fuse(T + 12LL * f, cx, cy, cz, table + (long long)f * a.rule.W * SP_TABLE, a.rule, a.inc, fr, a.trunc, &D, &I, &Wt, &cls, &evals);
    }
    if (!seen) return;                                                   // no frame saw the voxel: it keeps its bits
    a.tsdf[v] = (float)D;
    a.weight[v] = (int)Wt;
    if (a.intensity) a.intensity[v] = (float)I;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define SF_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)
#define SF_LAUNCHED(what) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) SF_FAIL(LRT_ERR_HIP, "%s: launch of %s failed: %s", fn, what, hipGetErrorString(e_)); } while (0)

static bool finite_d(double x) { return x - x == 0.0; }

static long long work_bytes_of(long long F, int W)
{
    if (F < 0 || F > LRT_SWEEPFUSE_MAX_FRAMES || W < 1) return -1;
    return round256(F * W * (long long)(SP_TABLE * sizeof(double)));
}

extern "C" {

int lrt_sweepfuse_abi_version(void) { return LRT_SWEEPFUSE_ABI_VERSION; }

const char* lrt_sweepfuse_last_error(void) { return g_err; }

long long lrt_sweepfuse_work_bytes(long long F, int W) { return work_bytes_of(F, W); }

int lrt_sweepfuse_integrate(int device, int X, int Y, int Z, double voxel, double trunc, float* tsdf, int* weight, float* intensity, long long F,
                            const double* grid2sensor, int H, int W, const float* depth, const unsigned char* mask, const float* frame_intensity,
                            const double* inclination, int n_inc, double off, double yaw, double min_depth, double max_depth, const double* twist,
                            const double* tau, void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_sweepfuse_integrate";
    if (X < 1 || Y < 1 || Z < 1 || (long long)X * Y * Z > LRT_SWEEPFUSE_MAX_VOXELS)
        SF_FAIL(LRT_ERR_ARG, "%s: a grid of %d x %d x %d voxels (each at least 1, X Y Z at most %lld)", fn, X, Y, Z, LRT_SWEEPFUSE_MAX_VOXELS);
    if (!(voxel > 0.0 && finite_d(voxel)) || !(trunc > 0.0 && finite_d(trunc))) SF_FAIL(LRT_ERR_ARG, "%s: voxel %g, trunc %g (both positive)", fn, voxel, trunc);
    if (F < 0 || F > LRT_SWEEPFUSE_MAX_FRAMES) SF_FAIL(LRT_ERR_ARG, "%s: %lld frames (0 to %d)", fn, F, LRT_SWEEPFUSE_MAX_FRAMES);
    if (H < 1 || W < 1 || F * H * (long long)W > LRT_SWEEPFUSE_MAX_VOXELS)
        SF_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d pixels (each at least 1, F H W at most %lld)", fn, F, H, W, LRT_SWEEPFUSE_MAX_VOXELS);
    if (!(n_inc == 2 || (n_inc == H && H >= 3))) SF_FAIL(LRT_ERR_ARG, "%s: %d inclinations for %d rows (2 bounds or one per row of at least 3)", fn, n_inc, H);
    if (!(off >= 0.0 && off < 1.0) || !finite_d(yaw)) SF_FAIL(LRT_ERR_ARG, "%s: off %g (in [0, 1)), yaw %g", fn, off, yaw);
    if (!(min_depth >= 0.0 && min_depth < max_depth && finite_d(max_depth))) SF_FAIL(LRT_ERR_ARG, "%s: depths (%g, %g]", fn, min_depth, max_depth);
    if (!tsdf || !weight) SF_FAIL(LRT_ERR_ARG, "%s: null tsdf / weight pointer", fn);
    if (!intensity != !frame_intensity) SF_FAIL(LRT_ERR_ARG, "%s: the grid's intensity and the frames' intensity go together", fn);
    if (F > 0 && (!grid2sensor || !depth || !mask || !inclination)) SF_FAIL(LRT_ERR_ARG, "%s: null grid2sensor / depth / mask / inclination pointer", fn);
    if (twist && !tau) SF_FAIL(LRT_ERR_ARG, "%s: null tau pointer with a twist (the column times are required then)", fn);
    if (F == 0) return LRT_OK;
    if (!workspace || ((uintptr_t)workspace & 255)) SF_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    const long long need = work_bytes_of(F, W);
    if (work_bytes < need) SF_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld frames of %d columns need %lld", fn, work_bytes, F, W, need);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) SF_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) SF_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    double* table = (double*)workspace;
    const long long n_cols = F * W;
    hipLaunchKernelGGL(k_sf_table, dim3((unsigned)((n_cols + NT - 1) / NT)), dim3(NT), 0, stream, n_cols, W, twist, tau, table);
    SF_LAUNCHED("the table");
    FuseArgs a;
    a.X = X; a.Y = Y; a.Z = Z; a.F = (int)F; a.N = (long long)X * Y * Z; a.HW = (long long)H * W;
    a.voxel = voxel; a.trunc = trunc;
    a.rule.H = H; a.rule.W = W; a.rule.n_inc = n_inc; a.rule.wrap = 1; a.rule.off = off; a.rule.yaw = yaw; a.rule.min_depth = min_depth; a.rule.max_depth = max_depth;
    a.tsdf = tsdf; a.weight = weight; a.intensity = intensity; a.depth = depth; a.mask = mask; a.fint = frame_intensity; a.inc = inclination;
    hipLaunchKernelGGL(k_sf_fuse, dim3((unsigned)((a.N + NT - 1) / NT)), dim3(NT), 0, stream, a, grid2sensor, table);
    SF_LAUNCHED("the fusion");
    return LRT_OK;
}

}  // extern "C"
