// lrt_sweep.hip -- the sweep rays (include/lrt_sweep.h), gfx950.  Compiled into liblrt_sweep.so, a library of its own.  No allocation, no host
// wait; the rule is lrt_sweep_math.h, all of it float64.
//
//   k_sweep_tables       one thread per column (f, w): T_f(tau[w]) = P_f Exp(tau[w] xi_f), the azimuth's sine and cosine, and from them the nine
//                        numbers a ray of the column needs (a = R (cos az, sin az, 0), c = R (0, 0, 1), t); H more threads: one row's cos and sin
//                        of the inclination.
//   k_sweep_rays         one thread per output COMPONENT (f, h, w, i): v = cos(inc) a + sin(inc) c, d = v / |v|; consecutive threads store
//                        consecutive floats of ray_d and of ray_o.  The tables are read through the cache: nine numbers serve 3 H threads.
//   k_sweep_bwd_cols     one wave per 64 columns of a frame, one thread per column.  The rows are walked in chunks of 64: each thread first puts
//                        one row's cos and sin into LDS (so a row's pair is computed once per workgroup, never per ray), then every thread sums
//                        its column's rows in row order: Ga = sum cos(inc) gv, Gc = sum sin(inc) gv, Gt = sum g_o.  The sums are chained through
//                        dExp/dxi (sw_column_bwd) into the column's 18 numbers, those are summed over the wave by a butterfly of shuffles, and
//                        lane 0 writes the workgroup's 18 numbers.
//   k_sweep_bwd_finish   one thread per result (f, k): the frame's workgroups summed in order, rounded to float32 once.
//
// Every sum is float64 in a fixed order and there is no atomic: equal inputs give equal bits.  This is the scheme of k_pp_bwd<1> / k_pp_bwd<2>.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_sweep_math.h"
#include "../../include/lrt_sweep.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_SWEEP_BLOCK;
constexpr int NCOL = LRT_SWEEP_COLS;
constexpr int SW_COL = 9;                                            // a (3), c (3), t (3) of a column
constexpr int SW_OUT = 18;                                           // d_pose (12) and d_twist (6) of a frame

static_assert(NCOL == 64, "k_sweep_bwd_cols is written for one wave");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

struct SweepArgs {
    long long F;
    int H, W, n_inc;
    double off, yaw;
    const float *pose, *twist, *inc, *tau;
    double *col, *row, *part;                                        // (F W, 9), (H, 2), (F, n_wg, 18) in the workspace
    int n_wg;
};

// ---- forward ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_sweep_tables(SweepArgs a)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const long long n_col = a.F * a.W;
    if (i < n_col) {
        const long long f = i / a.W;
        const int w = (int)(i - f * a.W);
        double R[9], t[3], ax[3], cx[3], sa, ca;
        sw_column_pose(a.pose + 12 * f, a.twist ? a.twist + 6 * f : nullptr, a.twist ? (double)a.tau[w] : 0.0, R, t);
        sincos(sw_azimuth(w, a.W, a.off, a.yaw), &sa, &ca);
        sw_column_axes(R, ca, sa, ax, cx);
        double* o = a.col + SW_COL * i;
        o[0] = ax[0]; o[1] = ax[1]; o[2] = ax[2]; o[3] = cx[0]; o[4] = cx[1]; o[5] = cx[2]; o[6] = t[0]; o[7] = t[1]; o[8] = t[2];
    } else if (i < n_col + a.H) {
        const int h = (int)(i - n_col);
        double si, ci;
        sincos(sw_inclination(h, a.H, a.inc, a.n_inc, a.off), &si, &ci);
        a.row[2 * h] = ci; a.row[2 * h + 1] = si;
    }
}

__global__ __launch_bounds__(NT) void k_sweep_rays(long long n_out, int H, int W, const double* __restrict__ col, const double* __restrict__ row,
                                                   float* __restrict__ ray_o, float* __restrict__ ray_d)
{
    const long long e = (long long)blockIdx.x * NT + threadIdx.x;
    if (e >= n_out) return;
    const long long ray = e / 3;
    const int comp = (int)(e - 3 * ray);
    const long long fh = ray / W;
    const int w = (int)(ray - fh * W);
    const long long f = fh / H;
    const int h = (int)(fh - f * H);
    const double* c = col + SW_COL * (f * W + w);
    const double ax[3] = {c[0], c[1], c[2]}, cx[3] = {c[3], c[4], c[5]};
    double d[3], n;
    sw_ray(ax, cx, row[2 * h], row[2 * h + 1], d, &n);
    ray_d[e] = (float)(comp == 0 ? d[0] : comp == 1 ? d[1] : d[2]);
    ray_o[e] = (float)c[6 + comp];
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NCOL) void k_sweep_bwd_cols(SweepArgs a, const float* __restrict__ g_o, const float* __restrict__ g_d)
{
    __shared__ double s_row[2 * NCOL];
    const int tid = threadIdx.x;
    const long long f = blockIdx.y;
    const int w = blockIdx.x * NCOL + tid;
    const bool active = w < a.W;
    const float* P = a.pose + 12 * f;
    const float* xi = a.twist ? a.twist + 6 * f : nullptr;
    double s = 0.0, sa = 0.0, ca = 1.0, ax[3] = {1.0, 0.0, 0.0}, cx[3] = {0.0, 0.0, 1.0};
    if (active) {
        double R[9], t[3];
        s = xi ? (double)a.tau[w] : 0.0;
        sw_column_pose(P, xi, s, R, t);
        sincos(sw_azimuth(w, a.W, a.off, a.yaw), &sa, &ca);
        sw_column_axes(R, ca, sa, ax, cx);
    }
    double Ga[3] = {0.0, 0.0, 0.0}, Gc[3] = {0.0, 0.0, 0.0}, Gt[3] = {0.0, 0.0, 0.0};
    for (int h0 = 0; h0 < a.H; h0 += NCOL) {                        // uniform over the workgroup
        __syncthreads();
        if (h0 + tid < a.H) {
            double si, ci;
            sincos(sw_inclination(h0 + tid, a.H, a.inc, a.n_inc, a.off), &si, &ci);
            s_row[2 * tid] = ci; s_row[2 * tid + 1] = si;
        }
        __syncthreads();
        const int n = a.H - h0 < NCOL ? a.H - h0 : NCOL;
        if (active) {
            for (int k = 0; k < n; k++) {
                const long long r = 3 * (((long long)f * a.H + (h0 + k)) * a.W + w);
                const double ci = s_row[2 * k], si = s_row[2 * k + 1];
                const double g[3] = {(double)g_d[r], (double)g_d[r + 1], (double)g_d[r + 2]};
                double d[3], nrm, gv[3];
                sw_ray(ax, cx, ci, si, d, &nrm);
                sw_ray_bwd(d, nrm, g, gv);
                for (int i = 0; i < 3; i++) {
                    Ga[i] += ci * gv[i];
                    Gc[i] += si * gv[i];
                    Gt[i] += (double)g_o[r + i];
                }
            }
        }
    }
    double out[SW_OUT];
    for (int k = 0; k < SW_OUT; k++) out[k] = 0.0;
    if (active) sw_column_bwd(P, xi, s, ca, sa, Ga, Gc, Gt, out, out + 12);
    for (int k = 0; k < SW_OUT; k++) {
        double v = out[k];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);    // a butterfly: the same order on every run
        out[k] = v;
    }
    if (tid == 0) {
        double* o = a.part + SW_OUT * ((long long)f * a.n_wg + blockIdx.x);
        for (int k = 0; k < SW_OUT; k++) o[k] = out[k];
    }
}

__global__ __launch_bounds__(NT) void k_sweep_bwd_finish(long long F, int n_wg, const double* __restrict__ part, float* __restrict__ d_pose,
                                                         float* __restrict__ d_twist)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= F * SW_OUT) return;
    const long long f = i / SW_OUT;
    const int k = (int)(i - f * SW_OUT);
    double v = 0.0;
    for (int g = 0; g < n_wg; g++) v += part[SW_OUT * (f * n_wg + g) + k];
    if (k < 12) d_pose[12 * f + k] = (float)v;
    else if (d_twist) d_twist[6 * f + (k - 12)] = (float)v;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define SW_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline int n_wg_of(int W) { return (W + NCOL - 1) / NCOL; }

static long long work_bytes_of(long long F, int H, int W)
{
    if (F < 1 || H < 1 || W < 1) return -1;
    const long long hw = (long long)H * W;
    if (hw > LRT_SWEEP_MAX_RAYS || F > LRT_SWEEP_MAX_RAYS / hw) return -1;
    return round256(8 * (SW_COL * F * W + 2 * (long long)H + SW_OUT * F * n_wg_of(W)));
}

// The checks both calls share; fills `a` on success.
static int check_common(const char* fn, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                        double off, double yaw, const float* tau, void* workspace, long long work_bytes, SweepArgs* a)
{
    const long long need = work_bytes_of(F, H, W);
    if (need < 0) SW_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d rays (each at least 1, F H W at most %lld)", fn, F, H, W, LRT_SWEEP_MAX_RAYS);
    if (n_inc != 2 && n_inc != H) SW_FAIL(LRT_ERR_ARG, "%s: %d inclinations (2 bounds, or one per row: %d)", fn, n_inc, H);
    if (!(off >= 0.0 && off < 1.0)) SW_FAIL(LRT_ERR_ARG, "%s: pixel offset %g (0 for KITTI, 0.5 for Waymo)", fn, off);
    if (!(yaw - yaw == 0.0)) SW_FAIL(LRT_ERR_ARG, "%s: yaw %g", fn, yaw);
    if (!pose || !inclination) SW_FAIL(LRT_ERR_ARG, "%s: null pose / inclination pointer", fn);
    if (twist && !tau) SW_FAIL(LRT_ERR_ARG, "%s: a twist without column times (null tau pointer)", fn);
    if (!workspace || ((uintptr_t)workspace & 255)) SW_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) SW_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld frames of %d x %d need %lld", fn, work_bytes, F, H, W, need);
    a->F = F; a->H = H; a->W = W; a->n_inc = n_inc; a->off = off; a->yaw = yaw;
    a->pose = pose; a->twist = twist; a->inc = inclination; a->tau = tau;
    a->n_wg = n_wg_of(W);
    a->col = (double*)workspace;
    a->row = a->col + SW_COL * F * W;
    a->part = a->row + 2 * (long long)H;
    return LRT_OK;
}

extern "C" {

int lrt_sweep_abi_version(void) { return LRT_SWEEP_ABI_VERSION; }

const char* lrt_sweep_last_error(void) { return g_err; }

long long lrt_sweep_work_bytes(long long F, int H, int W) { return work_bytes_of(F, H, W); }

int lrt_sweep_rays(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                   double off, double yaw, const float* tau, float* ray_o, float* ray_d, void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_sweep_rays";
    SweepArgs a;
    const int rc = check_common(fn, F, H, W, pose, twist, inclination, n_inc, off, yaw, tau, workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if (!ray_o || !ray_d) SW_FAIL(LRT_ERR_ARG, "%s: null ray_o / ray_d pointer", fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) SW_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) SW_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const long long n_tab = F * W + H, n_out = 3 * F * H * W;
    hipLaunchKernelGGL(k_sweep_tables, dim3((unsigned)((n_tab + NT - 1) / NT)), dim3(NT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) SW_FAIL(LRT_ERR_HIP, "%s: launch of the tables failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_sweep_rays, dim3((unsigned)((n_out + NT - 1) / NT)), dim3(NT), 0, stream, n_out, H, W, (const double*)a.col, (const double*)a.row,
                       ray_o, ray_d);
    e = hipGetLastError();
    if (e != hipSuccess) SW_FAIL(LRT_ERR_HIP, "%s: launch of the ray pass failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_sweep_backward(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                       double off, double yaw, const float* tau, const float* g_o, const float* g_d, float* d_pose, float* d_twist,
                       void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_sweep_backward";
    SweepArgs a;
    const int rc = check_common(fn, F, H, W, pose, twist, inclination, n_inc, off, yaw, tau, workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if (!g_o || !g_d) SW_FAIL(LRT_ERR_ARG, "%s: null g_o / g_d pointer", fn);
    if (!d_pose) SW_FAIL(LRT_ERR_ARG, "%s: null d_pose pointer", fn);
    if (twist && !d_twist) SW_FAIL(LRT_ERR_ARG, "%s: a twist without a d_twist pointer", fn);
    if (F > 65535) SW_FAIL(LRT_ERR_ARG, "%s: %lld frames in one call (at most 65535)", fn, F);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) SW_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) SW_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_sweep_bwd_cols, dim3((unsigned)a.n_wg, (unsigned)F), dim3(NCOL), 0, stream, a, g_o, g_d);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) SW_FAIL(LRT_ERR_HIP, "%s: launch of the column pass failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_sweep_bwd_finish, dim3((unsigned)((F * SW_OUT + NT - 1) / NT)), dim3(NT), 0, stream, F, a.n_wg, (const double*)a.part, d_pose, d_twist);
    e = hipGetLastError();
    if (e != hipSuccess) SW_FAIL(LRT_ERR_HIP, "%s: launch of the finish failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
