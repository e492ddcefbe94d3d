// lrt_mapreg.hip -- the scan-to-map registration (include/lrt_mapreg.h), gfx950.  Compiled into liblrt_mapreg.so, a library of its own.  No
// allocation, no host wait; the rule is lrt_mapreg_math.h on top of lrt_raycast_math.h, lrt_reg_math.h and lrt_project_math.h.
//
//   k_mapreg_linearize   one lane per source pixel, 256-lane workgroups, grid (ceil(H W / 256), F).  A lane transforms its point, gathers the
//                        eight tsdf and eight weight corners of its cell (neighbouring pixels hit neighbouring cells: the z pairs share a cache
//                        line) and holds its 30 terms in registers (zero without a term); the wave sums them by a butterfly of shuffles
//                        (m = 32 .. 1, the same order on every run), the four waves are added through LDS in wave order, and the workgroup
//                        writes one partial row of 30 float64.  The reduction is k_reg_linearize's, line for line.
//   k_mapreg_solve       one wave per frame.  Lane k < 30 adds column k of the frame's partial rows in ascending workgroup order.  For
//                        lrt_mapreg_linearize that is the result.  For lrt_mapreg_align lane 0 then takes the step (rg_solve), writes the running
//                        pose and its inverse, the log row and the running status, and on the last iteration the hessian and the status.
//
// There is no atomic: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_mapreg_math.h"
#include "../../include/lrt_mapreg.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_MAPREG_BLOCK;
constexpr int NS = LRT_MAPREG_NSUM;
constexpr int NL = LRT_MAPREG_NLOG;

static_assert(NT == 256, "k_mapreg_linearize is written for four waves");
static_assert(NS == RG_NSUM, "the header and the rule disagree");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

struct LinArgs {
    int HW, n_wg;
    RcGrid grid;
    double trunc, huber;
    const float* sp;
    const unsigned char* sm;
    const double* X;                                                 // (F, 3, 4)
    double* part;                                                    // (F, n_wg, 30) in the workspace
    int* cell;                                                       // (F, H W) or null
};

__global__ __launch_bounds__(NT) void k_mapreg_linearize(LinArgs a)
{
    __shared__ double s_part[(NT / 64) * NS];
    const int tid = threadIdx.x;
    const long long f = blockIdx.y;
    const int i = blockIdx.x * NT + tid;
    double t[NS];
#pragma unroll
    for (int k = 0; k < NS; k++) t[k] = 0.0;
    if (i < a.HW) {
        const long long base = f * a.HW;
        long long b = -1;
        if (a.sm[base + i]) b = mr_pixel(a.grid, a.trunc, a.X + 12 * f, a.sp + 3 * (base + i), a.huber, t, nullptr);
        if (a.cell) a.cell[base + i] = (int)b;
    }
#pragma unroll
    for (int k = 0; k < NS; k++) {
        double v = t[k];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);    // the same order on every run, the sum in every lane
        t[k] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int k = 0; k < NS; k++) s_part[(tid >> 6) * NS + k] = t[k];
    }
    __syncthreads();
    if (tid < NS) {
        const double v = ((s_part[tid] + s_part[NS + tid]) + s_part[2 * NS + tid]) + s_part[3 * NS + tid];
        a.part[(f * a.n_wg + blockIdx.x) * NS + tid] = v;
    }
}

struct SolveArgs {
    int n_wg, it, K;
    const double* part;
    double* sums;                                                    // (F, 30): lrt_mapreg_linearize; null for lrt_mapreg_align
    const double* X_in;
    double *X_out, *G_out;
    double lambda, min_pairs, tol_t, tol_r;
    int* running;                                                    // (F) in the workspace
    double *log, *hessian;
    int* status;
};

__global__ __launch_bounds__(64) void k_mapreg_solve(SolveArgs a)
{
    __shared__ double s[NS];
    const int lane = threadIdx.x;
    const long long f = blockIdx.x;
    if (lane < NS) {
        const double* __restrict__ col = a.part + f * a.n_wg * NS + lane;
        double v = 0.0;
        int g = 0;
        for (; g + 8 <= a.n_wg; g += 8) {                              // eight loads in flight, added in ascending order all the same
            double x[8];
#pragma unroll
            for (int j = 0; j < 8; j++) x[j] = col[(long long)(g + j) * NS];
#pragma unroll
            for (int j = 0; j < 8; j++) v += x[j];
        }
        for (; g < a.n_wg; g++) v += col[(long long)g * NS];
        s[lane] = v;
        if (a.sums) a.sums[f * NS + lane] = v;
    }
    __syncthreads();
    if (a.sums || lane != 0) return;
    double X[12], G[12], norms[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 12; k++) X[k] = a.X_in[12 * f + k];
    int st = a.it == 0 ? RG_OK : a.running[f];
    if (st == RG_OK) st = rg_solve(s, a.lambda, a.min_pairs, a.tol_t, a.tol_r, X, norms);
    a.running[f] = st;
    mr_inverse(X, G);
#pragma unroll
    for (int k = 0; k < 12; k++) { a.X_out[12 * f + k] = X[k]; a.G_out[12 * f + k] = G[k]; }
    double* row = a.log + (f * a.K + a.it) * NL;
    row[0] = s[29]; row[1] = s[27]; row[2] = s[28]; row[3] = norms[0]; row[4] = norms[1]; row[5] = (double)st; row[6] = 0.0; row[7] = 0.0;
    if (a.it == a.K - 1) {
        double* h = a.hessian + 36 * f;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int j = i; j < 6; j++) { h[6 * i + j] = s[k]; h[6 * j + i] = s[k]; k++; }
        }
        a.status[f] = st;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define MR_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline long long n_wg_of(long long hw) { return (hw + NT - 1) / NT; }

static long long work_bytes_of(long long F, int H, int W)
{
    if (F < 1 || H < 1 || W < 1 || F > LRT_MAPREG_MAX_FRAMES) return -1;
    const long long hw = (long long)H * W;
    if (hw > LRT_MAPREG_MAX_PIXELS || F > LRT_MAPREG_MAX_PIXELS / hw) return -1;
    return round256(8 * (NS * F * n_wg_of(hw) + F));
}

static bool finite_d(double x) { return x - x == 0.0; }

// The checks both calls share; fills `a` but for X and cell.
static int check_common(const char* fn, int X, int Y, int Z, double voxel, double trunc, const float* tsdf, const int* weight, int min_weight, long long F,
                        int H, int W, const float* sp, const unsigned char* sm, double huber, void* workspace, long long work_bytes, LinArgs* a)
{
    if (X < 1 || Y < 1 || Z < 1 || (long long)X * Y > LRT_MAPREG_MAX_VOXELS / Z)
        MR_FAIL(LRT_ERR_ARG, "%s: a grid of %d x %d x %d voxels (each at least 1, X Y Z at most %lld)", fn, X, Y, Z, LRT_MAPREG_MAX_VOXELS);
    if (!(voxel > 0.0 && finite_d(voxel))) MR_FAIL(LRT_ERR_ARG, "%s: voxel %g (positive)", fn, voxel);
    if (!(trunc > 0.0 && finite_d(trunc))) MR_FAIL(LRT_ERR_ARG, "%s: trunc %g (positive)", fn, trunc);
    if (min_weight < 1) MR_FAIL(LRT_ERR_ARG, "%s: min_weight %d (at least 1: weight 0 is unobserved)", fn, min_weight);
    if (!tsdf || !weight) MR_FAIL(LRT_ERR_ARG, "%s: null tsdf / weight pointer", fn);
    const long long need = work_bytes_of(F, H, W);
    if (need < 0)
        MR_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d pixels (each at least 1, at most %d frames, F H W at most %lld)", fn, F, H, W, LRT_MAPREG_MAX_FRAMES,
                LRT_MAPREG_MAX_PIXELS);
    if (!sp || !sm) MR_FAIL(LRT_ERR_ARG, "%s: null src_points / src_mask pointer", fn);
    if (!(huber > 0.0 && finite_d(huber))) MR_FAIL(LRT_ERR_ARG, "%s: huber %g (positive)", fn, huber);
    if (!workspace || ((uintptr_t)workspace & 255)) MR_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) MR_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld frames of %d x %d need %lld", fn, work_bytes, F, H, W, need);
    a->HW = H * W; a->n_wg = (int)n_wg_of((long long)H * W);
    a->grid.X = X; a->grid.Y = Y; a->grid.Z = Z; a->grid.min_weight = min_weight; a->grid.voxel = voxel;
    a->grid.ox = 0.0; a->grid.oy = 0.0; a->grid.oz = 0.0;
    a->grid.tsdf = tsdf; a->grid.weight = weight; a->grid.intensity = nullptr;
    a->trunc = trunc; a->huber = huber; a->sp = sp; a->sm = sm;
    a->part = (double*)workspace;
    a->cell = nullptr;
    return LRT_OK;
}

static int select_device(const char* fn, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) MR_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    return LRT_OK;
}

extern "C" {

int lrt_mapreg_abi_version(void) { return LRT_MAPREG_ABI_VERSION; }

const char* lrt_mapreg_last_error(void) { return g_err; }

long long lrt_mapreg_work_bytes(long long F, int H, int W) { return work_bytes_of(F, H, W); }

int lrt_mapreg_linearize(int device, int X, int Y, int Z, double voxel, double trunc, const float* tsdf, const int* weight, int min_weight, long long F,
                         int H, int W, const float* src_points, const unsigned char* src_mask, const double* pose, double huber, double* sums, int* cell,
                         void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_mapreg_linearize";
    LinArgs a;
    int rc = check_common(fn, X, Y, Z, voxel, trunc, tsdf, weight, min_weight, F, H, W, src_points, src_mask, huber, workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if (!pose || !sums) MR_FAIL(LRT_ERR_ARG, "%s: null pose / sums pointer", fn);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) MR_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    a.X = pose; a.cell = cell;
    hipLaunchKernelGGL(k_mapreg_linearize, dim3((unsigned)a.n_wg, (unsigned)F), dim3(NT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) MR_FAIL(LRT_ERR_HIP, "%s: launch of the linearisation failed: %s", fn, hipGetErrorString(e));
    SolveArgs s = {};
    s.n_wg = a.n_wg; s.part = a.part; s.sums = sums;
    hipLaunchKernelGGL(k_mapreg_solve, dim3((unsigned)F), dim3(64), 0, stream, s);
    e = hipGetLastError();
    if (e != hipSuccess) MR_FAIL(LRT_ERR_HIP, "%s: launch of the sum failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_mapreg_align(int device, int X, int Y, int Z, double voxel, double trunc, const float* tsdf, const int* weight, int min_weight, long long F,
                     int H, int W, const float* src_points, const unsigned char* src_mask, const double* X_init, int K, double huber, double lambda,
                     long long min_pairs, double tol_t, double tol_r, double* X_out, double* G_out, double* log, double* hessian, int* status,
                     void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_mapreg_align";
    LinArgs a;
    int rc = check_common(fn, X, Y, Z, voxel, trunc, tsdf, weight, min_weight, F, H, W, src_points, src_mask, huber, workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if (K < 1 || K > LRT_MAPREG_MAX_ITER) MR_FAIL(LRT_ERR_ARG, "%s: %d iterations (1 to %d)", fn, K, LRT_MAPREG_MAX_ITER);
    if (!(lambda >= 0.0 && finite_d(lambda))) MR_FAIL(LRT_ERR_ARG, "%s: lambda %g (not negative)", fn, lambda);
    if (min_pairs < 1) MR_FAIL(LRT_ERR_ARG, "%s: min_pairs %lld (at least 1)", fn, min_pairs);
    if (!(tol_t >= 0.0 && tol_r >= 0.0)) MR_FAIL(LRT_ERR_ARG, "%s: tolerances %g, %g (not negative)", fn, tol_t, tol_r);
    if (!X_init || !X_out || !G_out || !log || !hessian || !status)
        MR_FAIL(LRT_ERR_ARG, "%s: null X_init / X_out / G_out / log / hessian / status pointer", fn);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) MR_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    SolveArgs s = {};
    s.n_wg = a.n_wg; s.K = K; s.part = a.part; s.sums = nullptr; s.X_out = X_out; s.G_out = G_out;
    s.lambda = lambda; s.min_pairs = (double)min_pairs; s.tol_t = tol_t; s.tol_r = tol_r;
    s.running = (int*)(a.part + (long long)NS * F * a.n_wg);
    s.log = log; s.hessian = hessian; s.status = status;
    for (int it = 0; it < K; it++) {
        a.X = it == 0 ? X_init : X_out;
        hipLaunchKernelGGL(k_mapreg_linearize, dim3((unsigned)a.n_wg, (unsigned)F), dim3(NT), 0, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) MR_FAIL(LRT_ERR_HIP, "%s: launch of linearisation %d failed: %s", fn, it, hipGetErrorString(e));
        s.it = it; s.X_in = a.X;
        hipLaunchKernelGGL(k_mapreg_solve, dim3((unsigned)F), dim3(64), 0, stream, s);
        e = hipGetLastError();
        if (e != hipSuccess) MR_FAIL(LRT_ERR_HIP, "%s: launch of solve %d failed: %s", fn, it, hipGetErrorString(e));
    }
    return LRT_OK;
}

}  // extern "C"
