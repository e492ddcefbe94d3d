// lrt_reg.hip -- the scan registration (include/lrt_reg.h), gfx950.  Compiled into liblrt_reg.so, a library of its own.  No allocation, no host
// wait; the rule is lrt_reg_math.h on top of lrt_project_math.h and lrt_sweep_math.h.
//
//   k_reg_linearize   one lane per source pixel, consecutive lanes on consecutive columns, so that the windows of neighbouring lanes overlap and
//                     the target loads of a wave fall into few cache lines.  256-lane workgroups, grid (ceil(H W / 256), F).  A lane holds its 30
//                     terms in registers (zero without a partner); the wave sums them by a butterfly of shuffles (m = 32 .. 1, the same order on
//                     every run), the four waves are added through LDS in wave order, and the workgroup writes one partial row of 30 float64.
//   k_reg_solve       one wave per pair.  Lane k < 30 adds column k of the pair's partial rows in ascending workgroup order.  For
//                     lrt_reg_linearize that is the result.  For lrt_reg_align lane 0 then takes the step (rg_solve), writes the running pose,
//                     the log row and the running status, and on the last iteration the hessian and the status.
//
// The target window of a workgroup is NOT staged in LDS: see profiles/registration.md.  There is no atomic: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_reg_math.h"
#include "../../include/lrt_reg.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_REG_BLOCK;
constexpr int NS = LRT_REG_NSUM;
constexpr int NL = LRT_REG_NLOG;

static_assert(NT == 256, "k_reg_linearize is written for four waves");
static_assert(NS == RG_NSUM, "the header and the rule disagree");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

struct LinArgs {
    int HW, n_wg;
    PjRule rule;
    const double* inc;
    const float *sp, *tp, *tn;
    const unsigned char *sm, *tm;
    const double* X;                                                 // (F, 3, 4)
    int rh, rw;
    double max_d2, huber;
    double* part;                                                    // (F, n_wg, 30) in the workspace
    int* assoc;                                                      // (F, H W) or null
};

__global__ __launch_bounds__(NT) void k_reg_linearize(LinArgs a)
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
        int partner = -1;
        if (a.sm[base + i])
            partner = rg_pixel(a.X + 12 * f, a.sp + 3 * (base + i), a.rule, a.inc, a.tp + 3 * base, a.tn + 3 * base, a.tm + base, a.rh, a.rw, a.max_d2,
                               a.huber, t);
        if (a.assoc) a.assoc[base + i] = partner;
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
    double* sums;                                                    // (F, 30): lrt_reg_linearize; null for lrt_reg_align
    const double* X_in;
    double* X_out;
    double lambda, min_pairs, tol_t, tol_r;
    int* running;                                                    // (F) in the workspace
    double *log, *hessian;
    int* status;
};

__global__ __launch_bounds__(64) void k_reg_solve(SolveArgs a)
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
    double X[12], norms[2] = {0.0, 0.0};
#pragma unroll
    for (int k = 0; k < 12; k++) X[k] = a.X_in[12 * f + k];
    int st = a.it == 0 ? RG_OK : a.running[f];
    if (st == RG_OK) st = rg_solve(s, a.lambda, a.min_pairs, a.tol_t, a.tol_r, X, norms);
    a.running[f] = st;
#pragma unroll
    for (int k = 0; k < 12; k++) a.X_out[12 * f + k] = X[k];
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

#define RG_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline long long n_wg_of(long long hw) { return (hw + NT - 1) / NT; }

static long long work_bytes_of(long long F, int H, int W)
{
    if (F < 1 || H < 1 || W < 1 || F > LRT_REG_MAX_PAIRS) return -1;
    const long long hw = (long long)H * W;
    if (hw > LRT_REG_MAX_PIXELS || F > LRT_REG_MAX_PIXELS / hw) return -1;
    return round256(8 * (NS * F * n_wg_of(hw) + F));
}

static bool finite_d(double x) { return x - x == 0.0; }

// The checks both calls share; fills `a` but for X, the window and the distance.
static int check_common(const char* fn, long long F, int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth,
                        double max_depth, const float* sp, const unsigned char* sm, const float* tp, const float* tn, const unsigned char* tm,
                        double huber, void* workspace, long long work_bytes, LinArgs* a)
{
    const long long need = work_bytes_of(F, H, W);
    if (need < 0)
        RG_FAIL(LRT_ERR_ARG, "%s: %lld pairs of %d x %d pixels (each at least 1, at most %d pairs, F H W at most %lld)", fn, F, H, W, LRT_REG_MAX_PAIRS,
                LRT_REG_MAX_PIXELS);
    if (n_inc != 2 && (n_inc != H || H < 3)) RG_FAIL(LRT_ERR_ARG, "%s: %d inclinations (2 bounds, or one per row of at least 3: %d)", fn, n_inc, H);
    if (!(off >= 0.0 && off < 1.0)) RG_FAIL(LRT_ERR_ARG, "%s: pixel offset %g (0 for KITTI, 0.5 for Waymo)", fn, off);
    if (!finite_d(yaw)) RG_FAIL(LRT_ERR_ARG, "%s: yaw %g", fn, yaw);
    if (!(min_depth >= 0.0 && min_depth < max_depth && finite_d(max_depth))) RG_FAIL(LRT_ERR_ARG, "%s: depths (%g, %g] (0 <= min < max)", fn, min_depth, max_depth);
    if (!inclination) RG_FAIL(LRT_ERR_ARG, "%s: null inclination pointer", fn);
    if (!sp || !sm) RG_FAIL(LRT_ERR_ARG, "%s: null src_points / src_mask pointer", fn);
    if (!tp || !tn || !tm) RG_FAIL(LRT_ERR_ARG, "%s: null tgt_points / tgt_normals / tgt_mask pointer", fn);
    if (!(huber > 0.0 && finite_d(huber))) RG_FAIL(LRT_ERR_ARG, "%s: huber %g (positive)", fn, huber);
    if (!workspace || ((uintptr_t)workspace & 255)) RG_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) RG_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld pairs of %d x %d need %lld", fn, work_bytes, F, H, W, need);
    a->HW = H * W; a->n_wg = (int)n_wg_of((long long)H * W);
    a->rule.H = H; a->rule.W = W; a->rule.n_inc = n_inc; a->rule.wrap = 1;
    a->rule.off = off; a->rule.yaw = yaw; a->rule.min_depth = min_depth; a->rule.max_depth = max_depth;
    a->inc = inclination; a->sp = sp; a->sm = sm; a->tp = tp; a->tn = tn; a->tm = tm; a->huber = huber;
    a->part = (double*)workspace;
    a->assoc = nullptr;
    return LRT_OK;
}

static int check_window(const char* fn, double rh, double rw, double max_dist)
{
    if (!(rh >= 0.0 && rh <= LRT_REG_MAX_RH && rh == (double)(int)rh) || !(rw >= 0.0 && rw <= LRT_REG_MAX_RW && rw == (double)(int)rw))
        RG_FAIL(LRT_ERR_ARG, "%s: a window of %g rows and %g columns either side (whole numbers, at most %d and %d)", fn, rh, rw, LRT_REG_MAX_RH, LRT_REG_MAX_RW);
    if (!(max_dist > 0.0 && finite_d(max_dist))) RG_FAIL(LRT_ERR_ARG, "%s: max_dist %g (positive)", fn, max_dist);
    return LRT_OK;
}

static int select_device(const char* fn, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) RG_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    return LRT_OK;
}

extern "C" {

int lrt_reg_abi_version(void) { return LRT_REG_ABI_VERSION; }

const char* lrt_reg_last_error(void) { return g_err; }

long long lrt_reg_work_bytes(long long F, int H, int W) { return work_bytes_of(F, H, W); }

int lrt_reg_linearize(int device, long long F, int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth,
                      double max_depth, const float* src_points, const unsigned char* src_mask, const float* tgt_points, const float* tgt_normals,
                      const unsigned char* tgt_mask, const double* X, int rh, int rw, double max_dist, double huber, double* sums, int* assoc,
                      void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_reg_linearize";
    LinArgs a;
    int rc = check_common(fn, F, H, W, inclination, n_inc, off, yaw, min_depth, max_depth, src_points, src_mask, tgt_points, tgt_normals, tgt_mask, huber,
                          workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if ((rc = check_window(fn, (double)rh, (double)rw, max_dist)) != LRT_OK) return rc;
    if (!X || !sums) RG_FAIL(LRT_ERR_ARG, "%s: null X / sums pointer", fn);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) RG_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    a.X = X; a.rh = rh; a.rw = rw; a.max_d2 = max_dist * max_dist; a.assoc = assoc;
    hipLaunchKernelGGL(k_reg_linearize, dim3((unsigned)a.n_wg, (unsigned)F), dim3(NT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) RG_FAIL(LRT_ERR_HIP, "%s: launch of the linearisation failed: %s", fn, hipGetErrorString(e));
    SolveArgs s = {};
    s.n_wg = a.n_wg; s.part = a.part; s.sums = sums;
    hipLaunchKernelGGL(k_reg_solve, dim3((unsigned)F), dim3(64), 0, stream, s);
    e = hipGetLastError();
    if (e != hipSuccess) RG_FAIL(LRT_ERR_HIP, "%s: launch of the sum failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_reg_align(int device, long long F, int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth,
                  double max_depth, const float* src_points, const unsigned char* src_mask, const float* tgt_points, const float* tgt_normals,
                  const unsigned char* tgt_mask, const double* X_init, const double* schedule, int K, double huber, double lambda,
                  long long min_pairs, double tol_t, double tol_r, double* X_out, double* log, double* hessian, int* status, void* workspace,
                  long long work_bytes, void* stream_)
{
    const char* fn = "lrt_reg_align";
    LinArgs a;
    int rc = check_common(fn, F, H, W, inclination, n_inc, off, yaw, min_depth, max_depth, src_points, src_mask, tgt_points, tgt_normals, tgt_mask, huber,
                          workspace, work_bytes, &a);
    if (rc != LRT_OK) return rc;
    if (!schedule) RG_FAIL(LRT_ERR_ARG, "%s: null schedule pointer", fn);
    if (K < 1 || K > LRT_REG_MAX_ITER) RG_FAIL(LRT_ERR_ARG, "%s: a schedule of %d iterations (1 to %d)", fn, K, LRT_REG_MAX_ITER);
    for (int it = 0; it < K; it++)
        if ((rc = check_window(fn, schedule[3 * it], schedule[3 * it + 1], schedule[3 * it + 2])) != LRT_OK) return rc;
    if (!(lambda >= 0.0 && finite_d(lambda))) RG_FAIL(LRT_ERR_ARG, "%s: lambda %g (not negative)", fn, lambda);
    if (min_pairs < 1) RG_FAIL(LRT_ERR_ARG, "%s: min_pairs %lld (at least 1)", fn, min_pairs);
    if (!(tol_t >= 0.0 && tol_r >= 0.0)) RG_FAIL(LRT_ERR_ARG, "%s: tolerances %g, %g (not negative)", fn, tol_t, tol_r);
    if (!X_init || !X_out || !log || !hessian || !status) RG_FAIL(LRT_ERR_ARG, "%s: null X_init / X_out / log / hessian / status pointer", fn);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) RG_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    SolveArgs s = {};
    s.n_wg = a.n_wg; s.K = K; s.part = a.part; s.sums = nullptr; s.X_out = X_out;
    s.lambda = lambda; s.min_pairs = (double)min_pairs; s.tol_t = tol_t; s.tol_r = tol_r;
    s.running = (int*)(a.part + (long long)NS * F * a.n_wg);
    s.log = log; s.hessian = hessian; s.status = status;
    for (int it = 0; it < K; it++) {
        a.X = it == 0 ? X_init : X_out;
        a.rh = (int)schedule[3 * it]; a.rw = (int)schedule[3 * it + 1]; a.max_d2 = schedule[3 * it + 2] * schedule[3 * it + 2];
        hipLaunchKernelGGL(k_reg_linearize, dim3((unsigned)a.n_wg, (unsigned)F), dim3(NT), 0, stream, a);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) RG_FAIL(LRT_ERR_HIP, "%s: launch of linearisation %d failed: %s", fn, it, hipGetErrorString(e));
        s.it = it; s.X_in = a.X;
        hipLaunchKernelGGL(k_reg_solve, dim3((unsigned)F), dim3(64), 0, stream, s);
        e = hipGetLastError();
        if (e != hipSuccess) RG_FAIL(LRT_ERR_HIP, "%s: launch of solve %d failed: %s", fn, it, hipGetErrorString(e));
    }
    return LRT_OK;
}

}  // extern "C"
