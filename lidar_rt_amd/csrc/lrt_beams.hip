// lrt_beams.hip -- the beam rays (include/lrt_beams.h), gfx950.  Compiled into liblrt_beams.so, a library of its own.  No allocation, no host
// wait; the rule is lrt_beams_math.h on top of lrt_sweep_math.h, all of it float64.  The scheme is lrt_sweep.hip's with a second reduction axis.
//
//   k_beams_tables       one thread per column (f, w): T_f(tau[w]), the azimuth's sine and cosine, and from them the twelve numbers a ray of the
//                        column needs (A = R (ca, sa, 0), B = R (-sa, ca, 0), c = R (0, 0, 1), t); H more threads: one row's four numbers
//                        (cos and sin of the offset elevation, cos and sin of the azimuth offset).
//   k_beams_rays         one thread per output COMPONENT (f, h, w, i): a_h = cd A + sd B, v = ci a_h + si c, d = v / |v|; consecutive threads
//                        store consecutive floats of ray_d and of ray_o.
//   k_beams_bwd_cols     one wave per 64 columns of a frame, one thread per column.  The rows are walked in chunks of 64: each thread first puts
//                        one row's four numbers into LDS, then every thread walks the chunk's rows in row order.  Per ray: gv.  For the pose:
//                        Gp += ci cd gv, Gq += ci sd gv, Gc += si gv, Gt += g_o in the thread's registers.  For the beams: the ray's two terms
//                        are summed over the wave by a butterfly of shuffles (every lane ends with the sum; lanes past W give zero) and lane k
//                        keeps row k's pair, so that after the chunk the wave writes 64 rows' partials with one coalesced store.  After the
//                        rows the three sums go through dExp/dxi (bm_column_bwd) into the column's 18 numbers, a butterfly sums those, and
//                        lane 0 writes the workgroup's 18.
//   k_beams_bwd_finish   one thread per result: (f, k) sums the frame's workgroups in order; (h, j) sums the row's partials over the frames and
//                        the workgroups in ascending order.  Each rounded to float32 once.
//
// Which outputs are wanted is a kernel argument, not a template: the arithmetic of an output is the same instructions whatever else is asked
// for, so its bits do not depend on it.  Every sum is float64 in a fixed order and there is no atomic: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_beams_math.h"
#include "../../include/lrt_beams.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_SWEEP_BLOCK;
constexpr int NCOL = LRT_SWEEP_COLS;
constexpr int BM_COL = 12;                                           // A (3), B (3), c (3), t (3) of a column
constexpr int BM_ROW = 4;                                            // cos e, sin e, cos delta, sin delta of a row
constexpr int BM_OUT = 18;                                           // d_pose (12) and d_twist (6) of a frame

static_assert(NCOL == 64, "k_beams_bwd_cols is written for one wave");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

struct BeamArgs {
    long long F;
    int H, W, n_inc;
    double off, yaw;
    const float *pose, *twist, *inc, *tau, *beams;
    double *col, *row, *part, *bpart;                                // (F W, 12), (H, 4), (F, n_wg, 18), (F, n_wg, H, 2) in the workspace
    int n_wg;
};

// ---- forward ------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_beams_tables(BeamArgs a)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    const long long n_col = a.F * a.W;
    if (i < n_col) {
        const long long f = i / a.W;
        const int w = (int)(i - f * a.W);
        double R[9], t[3], A[3], B[3], cx[3], sa, ca;
        sw_column_pose(a.pose + 12 * f, a.twist ? a.twist + 6 * f : nullptr, a.twist ? (double)a.tau[w] : 0.0, R, t);
        sincos(sw_azimuth(w, a.W, a.off, a.yaw), &sa, &ca);
        sw_column_axes(R, ca, sa, A, cx);
        bm_column_axis(R, ca, sa, B);
        double* o = a.col + BM_COL * i;
        for (int k = 0; k < 3; k++) { o[k] = A[k]; o[3 + k] = B[k]; o[6 + k] = cx[k]; o[9 + k] = t[k]; }
    } else if (i < n_col + a.H) {
        const int h = (int)(i - n_col);
        double r[BM_ROW];
        bm_row(h, a.H, a.inc, a.n_inc, a.off, a.beams, r);
        for (int k = 0; k < BM_ROW; k++) a.row[BM_ROW * h + k] = r[k];
    }
}

__global__ __launch_bounds__(NT) void k_beams_rays(long long n_out, int H, int W, const double* __restrict__ col, const double* __restrict__ row,
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
    const double* c = col + BM_COL * (f * W + w);
    const double* r = row + BM_ROW * h;
    const double A[3] = {c[0], c[1], c[2]}, B[3] = {c[3], c[4], c[5]}, cx[3] = {c[6], c[7], c[8]};
    double ah[3], d[3], n;
    bm_row_axis(A, B, r[2], r[3], ah);
    sw_ray(ah, cx, r[0], r[1], d, &n);
    ray_d[e] = (float)(comp == 0 ? d[0] : comp == 1 ? d[1] : d[2]);
    ray_o[e] = (float)c[9 + comp];
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NCOL) void k_beams_bwd_cols(BeamArgs a, const float* __restrict__ g_o, const float* __restrict__ g_d, int want_pose,
                                                         int want_beams)
{
    __shared__ double s_row[BM_ROW * NCOL];
    const int tid = threadIdx.x;
    const long long f = blockIdx.y;
    const int w = blockIdx.x * NCOL + tid;
    const bool active = w < a.W;
    const float* P = a.pose + 12 * f;
    const float* xi = a.twist ? a.twist + 6 * f : nullptr;
    double s = 0.0, sa = 0.0, ca = 1.0, A[3] = {1.0, 0.0, 0.0}, B[3] = {0.0, 1.0, 0.0}, cx[3] = {0.0, 0.0, 1.0};
    if (active) {
        double R[9], t[3];
        s = xi ? (double)a.tau[w] : 0.0;
        sw_column_pose(P, xi, s, R, t);
        sincos(sw_azimuth(w, a.W, a.off, a.yaw), &sa, &ca);
        sw_column_axes(R, ca, sa, A, cx);
        bm_column_axis(R, ca, sa, B);
    }
    double Gp[3] = {0.0, 0.0, 0.0}, Gq[3] = {0.0, 0.0, 0.0}, Gc[3] = {0.0, 0.0, 0.0}, Gt[3] = {0.0, 0.0, 0.0};
    for (int h0 = 0; h0 < a.H; h0 += NCOL) {                        // uniform over the workgroup
        __syncthreads();
        if (h0 + tid < a.H) {
            double r[BM_ROW];
            bm_row(h0 + tid, a.H, a.inc, a.n_inc, a.off, a.beams, r);
            for (int k = 0; k < BM_ROW; k++) s_row[BM_ROW * tid + k] = r[k];
        }
        __syncthreads();
        const int n = a.H - h0 < NCOL ? a.H - h0 : NCOL;
        double keep_e = 0.0, keep_d = 0.0;
        for (int k = 0; k < n; k++) {                               // uniform too: the shuffles below are the whole wave's
            double ge = 0.0, gd = 0.0;
            if (active) {
                const long long r = 3 * (((long long)f * a.H + (h0 + k)) * a.W + w);
                const double rw[BM_ROW] = {s_row[BM_ROW * k], s_row[BM_ROW * k + 1], s_row[BM_ROW * k + 2], s_row[BM_ROW * k + 3]};
                const double g[3] = {(double)g_d[r], (double)g_d[r + 1], (double)g_d[r + 2]};
                double ah[3], d[3], nrm, gv[3];
                bm_row_axis(A, B, rw[2], rw[3], ah);
                sw_ray(ah, cx, rw[0], rw[1], d, &nrm);
                sw_ray_bwd(d, nrm, g, gv);
                if (want_pose) {
                    const double wp = rw[0] * rw[2], wq = rw[0] * rw[3];
                    for (int i = 0; i < 3; i++) {
                        Gp[i] += wp * gv[i];
                        Gq[i] += wq * gv[i];
                        Gc[i] += rw[1] * gv[i];
                        Gt[i] += (double)g_o[r + i];
                    }
                }
                if (want_beams) bm_ray_beam_bwd(A, B, cx, ah, rw, gv, &ge, &gd);
            }
            if (want_beams) {
                for (int m = 32; m >= 1; m >>= 1) {                 // a butterfly: the same order on every run, the sum in every lane
                    ge += __shfl_xor(ge, m);
                    gd += __shfl_xor(gd, m);
                }
                if (tid == k) { keep_e = ge; keep_d = gd; }
            }
        }
        if (want_beams && tid < n) {
            double* o = a.bpart + 2 * (((long long)f * a.n_wg + blockIdx.x) * a.H + (h0 + tid));
            o[0] = keep_e; o[1] = keep_d;
        }
    }
    if (!want_pose) return;                                         // uniform
    double out[BM_OUT];
    for (int k = 0; k < BM_OUT; k++) out[k] = 0.0;
    if (active) bm_column_bwd(P, xi, s, ca, sa, Gp, Gq, Gc, Gt, out, out + 12);
    for (int k = 0; k < BM_OUT; k++) {
        double v = out[k];
        for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        out[k] = v;
    }
    if (tid == 0) {
        double* o = a.part + BM_OUT * ((long long)f * a.n_wg + blockIdx.x);
        for (int k = 0; k < BM_OUT; k++) o[k] = out[k];
    }
}

// n_pose = F * 18 with d_pose, 0 without; the 2 H beam results follow
__global__ __launch_bounds__(NT) void k_beams_bwd_finish(long long F, int H, int n_wg, long long n_pose, const double* __restrict__ part,
                                                         const double* __restrict__ bpart, float* __restrict__ d_pose, float* __restrict__ d_twist,
                                                         float* __restrict__ d_beams)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n_pose) {
        const long long f = i / BM_OUT;
        const int k = (int)(i - f * BM_OUT);
        double v = 0.0;
        for (int g = 0; g < n_wg; g++) v += part[BM_OUT * (f * n_wg + g) + k];
        if (k < 12) d_pose[12 * f + k] = (float)v;
        else if (d_twist) d_twist[6 * f + (k - 12)] = (float)v;
    } else if (d_beams && i < n_pose + 2 * (long long)H) {
        const long long j = i - n_pose;                              // = 2 h + (0: eps, 1: delta)
        double v = 0.0;
        for (long long fg = 0; fg < F * n_wg; fg++) v += bpart[2 * fg * H + j];
        d_beams[j] = (float)v;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define BM_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline int n_wg_of(int W) { return (W + NCOL - 1) / NCOL; }

static long long work_bytes_of(long long F, int H, int W)
{
    if (F < 1 || H < 1 || W < 1) return -1;
    const long long hw = (long long)H * W;
    if (hw > LRT_SWEEP_MAX_RAYS || F > LRT_SWEEP_MAX_RAYS / hw) return -1;
    const long long n_wg = n_wg_of(W);
    return round256(8 * (BM_COL * F * W + BM_ROW * (long long)H + BM_OUT * F * n_wg + 2 * F * n_wg * H));
}

// The checks both calls share; fills `a` on success.
static int check_common(const char* fn, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                        double off, double yaw, const float* tau, const float* beams, void* workspace, long long work_bytes, BeamArgs* a)
{
    const long long need = work_bytes_of(F, H, W);
    if (need < 0) BM_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d rays (each at least 1, F H W at most %lld)", fn, F, H, W, LRT_SWEEP_MAX_RAYS);
    if (n_inc != 2 && n_inc != H) BM_FAIL(LRT_ERR_ARG, "%s: %d inclinations (2 bounds, or one per row: %d)", fn, n_inc, H);
    if (!(off >= 0.0 && off < 1.0)) BM_FAIL(LRT_ERR_ARG, "%s: pixel offset %g (0 for KITTI, 0.5 for Waymo)", fn, off);
    if (!(yaw - yaw == 0.0)) BM_FAIL(LRT_ERR_ARG, "%s: yaw %g", fn, yaw);
    if (!pose || !inclination) BM_FAIL(LRT_ERR_ARG, "%s: null pose / inclination pointer", fn);
    if (!beams) BM_FAIL(LRT_ERR_ARG, "%s: null beams pointer (the sweep rays have no table: lrt_sweep_rays)", fn);
    if (twist && !tau) BM_FAIL(LRT_ERR_ARG, "%s: a twist without column times (null tau pointer)", fn);
    if (!workspace || ((uintptr_t)workspace & 255)) BM_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) BM_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld frames of %d x %d need %lld", fn, work_bytes, F, H, W, need);
    a->F = F; a->H = H; a->W = W; a->n_inc = n_inc; a->off = off; a->yaw = yaw;
    a->pose = pose; a->twist = twist; a->inc = inclination; a->tau = tau; a->beams = beams;
    a->n_wg = n_wg_of(W);
    a->col = (double*)workspace;
    a->row = a->col + BM_COL * F * W;
    a->part = a->row + BM_ROW * (long long)H;
    a->bpart = a->part + BM_OUT * F * a->n_wg;
    return LRT_OK;
}

extern "C" {

int lrt_beams_abi_version(void) { return LRT_BEAMS_ABI_VERSION; }

const char* lrt_beams_last_error(void) { return g_err; }

long long lrt_beams_work_bytes(long long F, int H, int W) { return work_bytes_of(F, H, W); }

int lrt_beams_rays(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                   double off, double yaw, const float* tau, const float* beams, float* ray_o, float* ray_d, void* workspace, long long work_bytes,
                   void* stream_)
{
    const char* fn = "lrt_beams_rays";
    BeamArgs a;
    const int rc = check_common(fn, F, H, W, pose, twist, inclination, n_inc, off, yaw, tau, beams, workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if (!ray_o || !ray_d) BM_FAIL(LRT_ERR_ARG, "%s: null ray_o / ray_d pointer", fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) BM_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) BM_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const long long n_tab = F * W + H, n_out = 3 * F * H * W;
    hipLaunchKernelGGL(k_beams_tables, dim3((unsigned)((n_tab + NT - 1) / NT)), dim3(NT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) BM_FAIL(LRT_ERR_HIP, "%s: launch of the tables failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_beams_rays, dim3((unsigned)((n_out + NT - 1) / NT)), dim3(NT), 0, stream, n_out, H, W, (const double*)a.col, (const double*)a.row,
                       ray_o, ray_d);
    e = hipGetLastError();
    if (e != hipSuccess) BM_FAIL(LRT_ERR_HIP, "%s: launch of the ray pass failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_beams_backward(int device, long long F, int H, int W, const float* pose, const float* twist, const float* inclination, int n_inc,
                       double off, double yaw, const float* tau, const float* beams, const float* g_o, const float* g_d, float* d_pose,
                       float* d_twist, float* d_beams, void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_beams_backward";
    BeamArgs a;
    const int rc = check_common(fn, F, H, W, pose, twist, inclination, n_inc, off, yaw, tau, beams, workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if (!g_o || !g_d) BM_FAIL(LRT_ERR_ARG, "%s: null g_o / g_d pointer", fn);
    if (!d_pose && !d_beams) BM_FAIL(LRT_ERR_ARG, "%s: neither d_pose nor d_beams is asked for", fn);
    if (d_pose && twist && !d_twist) BM_FAIL(LRT_ERR_ARG, "%s: a twist without a d_twist pointer", fn);
    if (!d_pose && d_twist) BM_FAIL(LRT_ERR_ARG, "%s: d_twist goes with d_pose (null d_pose pointer)", fn);
    if (F > 65535) BM_FAIL(LRT_ERR_ARG, "%s: %lld frames in one call (at most 65535)", fn, F);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) BM_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) BM_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_beams_bwd_cols, dim3((unsigned)a.n_wg, (unsigned)F), dim3(NCOL), 0, stream, a, g_o, g_d, d_pose ? 1 : 0, d_beams ? 1 : 0);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) BM_FAIL(LRT_ERR_HIP, "%s: launch of the column pass failed: %s", fn, hipGetErrorString(e));
    const long long n_pose = d_pose ? F * BM_OUT : 0, n_fin = n_pose + (d_beams ? 2 * (long long)H : 0);
    hipLaunchKernelGGL(k_beams_bwd_finish, dim3((unsigned)((n_fin + NT - 1) / NT)), dim3(NT), 0, stream, F, H, a.n_wg, n_pose, (const double*)a.part,
                       (const double*)a.bpart, d_pose, d_twist, d_beams);
    e = hipGetLastError();
    if (e != hipSuccess) BM_FAIL(LRT_ERR_HIP, "%s: launch of the finish failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
