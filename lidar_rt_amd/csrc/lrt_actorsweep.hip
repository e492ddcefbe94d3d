// lrt_actorsweep.hip -- actors that move within a sweep (include/lrt_actorsweep.h), gfx950.  Compiled into liblrt_actorsweep.so, a library of its
// own.  No allocation, no host wait; the rule per Gaussian is lrt_actorsweep_math.h.
//
//   k_as_table    one thread per column: world -> the column's sensor frame, (P Exp(tau[w] xi))^-1, as 12 doubles in the workspace (24 KB at
//                 W = 256, 196 KB at W = 2048: it stays in L2).  Its first four threads clear the counts.
//   k_as_fwd      one thread per Gaussian: its asset (the binary search of k_pp_fwd), the column search, the placement, three stores.
//                 Exp(tau[w] eta_a) is evaluated per search step -- the series of sw_coef, no table of A x W entries to fill and to miss in.
//                 The four counts of a workgroup come from ballots, are added over the four waves in LDS and leave as one 64-bit integer add each.
//   k_as_bwd      one thread per Gaussian: d_xyz, d_rot_raw, and its six float64 terms of d_actor_twist, reduced per asset the workgroup touches
//                 (wave shuffles, then the four waves in LDS, fixed order) into row (workgroup + asset) of the partial sums: the layout of
//                 k_pp_bwd<1>, unique because a later workgroup starts at or after the last asset of an earlier one.
//   k_as_finish   one workgroup per asset: the rows of the workgroups that cover its segment in a fixed order, rounded to float32 once.
//
// The only atomics are 64-bit integer adds, which commute: equal inputs give equal bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_actorsweep_math.h"
#include "../../include/lrt_actorsweep.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_ACTORSWEEP_BLOCK;
constexpr int NC = LRT_ACTORSWEEP_N_COUNTS;
enum { C_MOVED = 0, C_PASSED = 1, C_UNCONVERGED = 2, C_INVALID = 3 };

static_assert(NT == 256, "the kernels below are written for four waves");
static_assert(AS_MAX_EVAL == LRT_ACTORSWEEP_MAX_EVAL && AS_TABLE == LRT_ACTORSWEEP_TABLE, "the rule's header and the C ABI disagree");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

// The asset of Gaussian g: seg[lo] <= g < seg[hi] for ascending segments; within [0, A) whatever `seg` holds.
__device__ __forceinline__ int as_asset(int g, int A, const int32_t* __restrict__ seg)
{
    int lo = 0, hi = A;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg[mid] <= g) lo = mid; else hi = mid; }
    return lo;
}

// eta of asset a; returns whether the asset is searched at all: posed, and a twist row that is not all zeros
__device__ __forceinline__ bool as_live(int a, const float* __restrict__ poses, const float* __restrict__ twist, double* eta)
{
    bool any = false;
    for (int k = 0; k < 6; k++) {
        eta[k] = (double)twist[6 * (size_t)a + k];
        any = any || eta[k] != 0.0;
    }
    return any && poses[8 * (size_t)a + 7] != 0.f;
}

// ---- table --------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_as_table(int W, const double* __restrict__ w2s, const double* __restrict__ xi, const double* __restrict__ tau,
                                                 double* __restrict__ table, long long* __restrict__ counts)
{
    const int w = blockIdx.x * NT + threadIdx.x;
    if (w < NC) counts[w] = 0;
    if (w >= W) return;
    double m[AS_TABLE], x[6], T[AS_TABLE];
    for (int k = 0; k < AS_TABLE; k++) m[k] = w2s[k];
    if (xi) {
        for (int k = 0; k < 6; k++) x[k] = xi[k];
        as_table_entry(m, x, tau[w], T);
    } else {
        as_table_entry(m, nullptr, tau[w], T);
    }
    for (int k = 0; k < AS_TABLE; k++) table[AS_TABLE * (size_t)w + k] = T[k];
}

// ---- forward ------------------------------------------------------------------------------------------------------------------------------------------
struct FwdArgs {
    int P, A, W;
    const float *xyz, *rot, *poses, *twist;
    const int32_t* seg;
    const double *w2s, *table, *tau;
    double off, yaw;
    float *xyz_s, *rot_s;
    int32_t* column;
    long long* counts;
};

__global__ __launch_bounds__(NT) void k_as_fwd(FwdArgs a)
{
    __shared__ unsigned s_n[NT / 64][NC];
    const int tid = threadIdx.x;
    const int g = blockIdx.x * NT + tid;
    const bool exists = g < a.P;
    bool moved = false, unconverged = false, invalid = false;
    if (exists) {
        const int as = as_asset(g, a.A, a.seg);
        const float xf[3] = {a.xyz[3 * (size_t)g], a.xyz[3 * (size_t)g + 1], a.xyz[3 * (size_t)g + 2]};
        const float4 rq = reinterpret_cast<const float4*>(a.rot)[g];
        const float rf[4] = {rq.x, rq.y, rq.z, rq.w};
        float xo[3] = {xf[0], xf[1], xf[2]}, ro[4] = {rf[0], rf[1], rf[2], rf[3]};
        int col = -1;
        double eta[6];
        if (as_live(as, a.poses, a.twist, eta)) {
            double Ra[9], ta[3], w2s[AS_TABLE];
            as_pose(a.poses + 8 * (size_t)as, Ra, ta);
            for (int k = 0; k < AS_TABLE; k++) w2s[k] = a.w2s[k];
            PjRule R;
            R.H = 1; R.W = a.W; R.n_inc = 2; R.wrap = 1; R.off = a.off; R.yaw = a.yaw; R.min_depth = 0.0; R.max_depth = 0.0;
            const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]};
            int evals;
            const int state = as_search(x, Ra, ta, eta, w2s, a.table, a.tau, R, &col, &evals);
            invalid = state == AS_INVALID;
            unconverged = state == AS_UNCONVERGED;
            if (!invalid && col >= 0 && col < a.W) moved = as_place(eta, a.tau[col], xf, rf, xo, ro);
            else col = -1;
        }
        a.xyz_s[3 * (size_t)g] = xo[0]; a.xyz_s[3 * (size_t)g + 1] = xo[1]; a.xyz_s[3 * (size_t)g + 2] = xo[2];
        reinterpret_cast<float4*>(a.rot_s)[g] = make_float4(ro[0], ro[1], ro[2], ro[3]);
        a.column[g] = col;
    }
    const unsigned long long b_moved = __ballot(exists && moved), b_passed = __ballot(exists && !moved);
    const unsigned long long b_unc = __ballot(exists && unconverged), b_inv = __ballot(exists && invalid);
    if ((tid & 63) == 0) {
        s_n[tid >> 6][C_MOVED] = (unsigned)__popcll(b_moved); s_n[tid >> 6][C_PASSED] = (unsigned)__popcll(b_passed);
        s_n[tid >> 6][C_UNCONVERGED] = (unsigned)__popcll(b_unc); s_n[tid >> 6][C_INVALID] = (unsigned)__popcll(b_inv);
    }
    __syncthreads();
    if (tid < NC) {
        long long n = 0;
        for (int k = 0; k < NT / 64; k++) n += s_n[k][tid];
        if (n) __hip_atomic_fetch_add(a.counts + tid, n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
    int P, A, W;
    const float *xyz, *rot, *poses, *twist;
    const int32_t* seg;
    const double* tau;
    const int32_t* column;
    const float *g_xyz, *g_rot;
    float *d_xyz, *d_rot, *d_twist;
    double* part;
};

__device__ __forceinline__ double as_wave_sum(double v)
{
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// the 6 partials of the workgroup -> red[wave][k]: wave sums, then the caller adds the 4 waves in order
__device__ __forceinline__ void as_block_sum6(double (&v)[6], double (*red)[6])
{
    for (int k = 0; k < 6; k++) v[k] = as_wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0)
        for (int k = 0; k < 6; k++) red[threadIdx.x >> 6][k] = v[k];
    __syncthreads();
}

__global__ __launch_bounds__(NT) void k_as_bwd(BwdArgs a)
{
    __shared__ double red[NT / 64][6];
    const int tid = threadIdx.x;
    const int g = blockIdx.x * NT + tid;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int ga = -1;                                                   // this thread's asset; -1 past the end
    if (g < a.P) {
        ga = as_asset(g, a.A, a.seg);
        const float xf[3] = {a.xyz[3 * (size_t)g], a.xyz[3 * (size_t)g + 1], a.xyz[3 * (size_t)g + 2]};
        const float4 rq = reinterpret_cast<const float4*>(a.rot)[g];
        const float rf[4] = {rq.x, rq.y, rq.z, rq.w};
        const float gx = a.g_xyz[3 * (size_t)g], gy = a.g_xyz[3 * (size_t)g + 1], gz = a.g_xyz[3 * (size_t)g + 2];
        const float4 gr = reinterpret_cast<const float4*>(a.g_rot)[g];
        float dxo[3] = {gx, gy, gz}, dro[4] = {gr.x, gr.y, gr.z, gr.w};
        const int col = a.column[g];
        double eta[6];
        if (as_live(ga, a.poses, a.twist, eta) && col >= 0 && col < a.W) {
            const double gg[3] = {(double)gx, (double)gy, (double)gz}, hh[4] = {(double)gr.x, (double)gr.y, (double)gr.z, (double)gr.w};
            double dx[3], dr[4];
            if (as_place_bwd(eta, a.tau[col], xf, rf, gg, hh, dx, dr, acc)) {
                for (int k = 0; k < 3; k++) dxo[k] = (float)dx[k];
                for (int k = 0; k < 4; k++) dro[k] = (float)dr[k];
            }
        }
        a.d_xyz[3 * (size_t)g] = dxo[0]; a.d_xyz[3 * (size_t)g + 1] = dxo[1]; a.d_xyz[3 * (size_t)g + 2] = dxo[2];
        reinterpret_cast<float4*>(a.d_rot)[g] = make_float4(dro[0], dro[1], dro[2], dro[3]);
    }
    // one row of `part` per searched, non-empty asset the workgroup touches (the assets of its first and last Gaussian)
    const int b0 = blockIdx.x * NT;
    const int last = b0 + NT - 1 < a.P - 1 ? b0 + NT - 1 : a.P - 1;
    const int a0 = as_asset(b0, a.A, a.seg), a1 = as_asset(last, a.A, a.seg);
    for (int as = a0; as <= a1; as++) {                              // uniform trip count and branches: every thread reaches every barrier
        double eta[6];
        if (!as_live(as, a.poses, a.twist, eta) || a.seg[as] >= a.seg[as + 1]) continue;
        double v[6];
        for (int k = 0; k < 6; k++) v[k] = ga == as ? acc[k] : 0.0;
        as_block_sum6(v, red);
        if (tid < 6) a.part[6 * ((size_t)blockIdx.x + as) + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
        __syncthreads();
    }
}

__global__ __launch_bounds__(NT) void k_as_finish(int P, int A, const int32_t* __restrict__ seg, const float* __restrict__ poses,
                                                  const float* __restrict__ twist, const double* __restrict__ part, float* __restrict__ d_twist)
{
    __shared__ double red[NT / 64][6];
    const int as = blockIdx.x;
    if (as >= A) return;
    int s0 = seg[as], s1 = seg[as + 1];
    s0 = s0 < 0 ? 0 : (s0 > P ? P : s0);                            // a row of `part` outside the array is never read
    s1 = s1 < 0 ? 0 : (s1 > P ? P : s1);
    double eta[6];
    const bool live = as_live(as, poses, twist, eta) && s1 > s0;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (live)
        for (int b = (s0 >> 8) + (int)threadIdx.x; b <= (s1 - 1) >> 8; b += NT)
            for (int k = 0; k < 6; k++) v[k] += part[6 * ((size_t)b + as) + k];
    as_block_sum6(v, red);
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        d_twist[6 * (size_t)as + k] = live ? (float)(((red[0][k] + red[1][k]) + red[2][k]) + red[3][k]) : 0.f;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define AS_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static long long table_bytes_of(int W) { return round256((long long)W * AS_TABLE * (long long)sizeof(double)); }

static long long work_bytes_of(long long P, int A, int W)
{
    if (P < 0 || P > LRT_ACTORSWEEP_MAX_POINTS || A < 1 || A > LRT_ACTORSWEEP_MAX_ASSETS || W < 1 || W > LRT_ACTORSWEEP_MAX_COLUMNS) return -1;
    return table_bytes_of(W) + round256(6 * (long long)sizeof(double) * ((P + NT - 1) / NT + A));
}

// The checks both calls share; 0 or a negative code.
static int check_common(const char* fn, long long P, int A, int W, const void* xyz, const void* rot, const void* seg, const void* poses, const void* twist,
                        const void* tau, const void* workspace, long long work_bytes)
{
    if (P < 0 || P > LRT_ACTORSWEEP_MAX_POINTS) AS_FAIL(LRT_ERR_ARG, "%s: %lld Gaussians (0 .. %lld)", fn, P, LRT_ACTORSWEEP_MAX_POINTS);
    if (A < 1 || A > LRT_ACTORSWEEP_MAX_ASSETS) AS_FAIL(LRT_ERR_ARG, "%s: %d assets (1 .. %d)", fn, A, LRT_ACTORSWEEP_MAX_ASSETS);
    if (W < 1 || W > LRT_ACTORSWEEP_MAX_COLUMNS) AS_FAIL(LRT_ERR_ARG, "%s: %d columns (1 .. %d)", fn, W, LRT_ACTORSWEEP_MAX_COLUMNS);
    if (P > 0 && (!xyz || !rot)) AS_FAIL(LRT_ERR_ARG, "%s: null xyz / rot_raw pointer", fn);
    if ((uintptr_t)rot & 15) AS_FAIL(LRT_ERR_ARG, "%s: rot_raw must be 16-byte aligned (its rows are read as float4)", fn);
    if (!seg || !poses || !twist) AS_FAIL(LRT_ERR_ARG, "%s: null seg_start / poses / actor_twist pointer", fn);
    if (!tau) AS_FAIL(LRT_ERR_ARG, "%s: null tau pointer", fn);
    if (!workspace || ((uintptr_t)workspace & 255)) AS_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    const long long need = work_bytes_of(P, A, W);
    if (work_bytes < need) AS_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld Gaussians in %d assets and %d columns need %lld", fn, work_bytes, P, A, W, need);
    return LRT_OK;
}

extern "C" {

int lrt_actorsweep_abi_version(void) { return LRT_ACTORSWEEP_ABI_VERSION; }

const char* lrt_actorsweep_last_error(void) { return g_err; }

long long lrt_actorsweep_work_bytes(long long P, int A, int W) { return work_bytes_of(P, A, W); }

int lrt_actorsweep_forward(int device, long long P, int A, const float* xyz, const float* rot_raw, const int32_t* seg_start, const float* poses,
                           const float* actor_twist, const double* world2sensor, const double* sensor_twist, const double* tau, int W, double off,
                           double yaw, float* xyz_s, float* rot_s, int32_t* column, long long* counts, void* workspace, long long work_bytes,
                           void* stream_)
{
    const char* fn = "lrt_actorsweep_forward";
    const int rc = check_common(fn, P, A, W, xyz, rot_raw, seg_start, poses, actor_twist, tau, workspace, work_bytes);
    if (rc) return rc;
    if (!world2sensor) AS_FAIL(LRT_ERR_ARG, "%s: null world2sensor pointer", fn);
    if (!(off >= 0.0 && off < 1.0)) AS_FAIL(LRT_ERR_ARG, "%s: pixel offset %g (0 for KITTI, 0.5 for Waymo)", fn, off);
    if (!pj_finite(yaw)) AS_FAIL(LRT_ERR_ARG, "%s: yaw %g", fn, yaw);
    if (!counts || (P > 0 && (!xyz_s || !rot_s || !column))) AS_FAIL(LRT_ERR_ARG, "%s: null xyz_s / rot_s / column / counts pointer", fn);
    if ((uintptr_t)rot_s & 15) AS_FAIL(LRT_ERR_ARG, "%s: rot_s must be 16-byte aligned (its rows are written as float4)", fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) AS_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) AS_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    double* table = (double*)workspace;
    const int n_tab = W > NC ? W : NC;
    hipLaunchKernelGGL(k_as_table, dim3((unsigned)((n_tab + NT - 1) / NT)), dim3(NT), 0, stream, W, world2sensor, sensor_twist, tau, table, counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) AS_FAIL(LRT_ERR_HIP, "%s: launch of the table failed: %s", fn, hipGetErrorString(e));
    if (P > 0) {
        FwdArgs f;
        f.P = (int)P; f.A = A; f.W = W; f.xyz = xyz; f.rot = rot_raw; f.poses = poses; f.twist = actor_twist; f.seg = seg_start;
        f.w2s = world2sensor; f.table = table; f.tau = tau; f.off = off; f.yaw = yaw; f.xyz_s = xyz_s; f.rot_s = rot_s; f.column = column; f.counts = counts;
        hipLaunchKernelGGL(k_as_fwd, dim3((unsigned)((P + NT - 1) / NT)), dim3(NT), 0, stream, f);
        e = hipGetLastError();
        if (e != hipSuccess) AS_FAIL(LRT_ERR_HIP, "%s: launch of the forward failed: %s", fn, hipGetErrorString(e));
    }
    return LRT_OK;
}

int lrt_actorsweep_backward(int device, long long P, int A, const float* xyz, const float* rot_raw, const int32_t* seg_start, const float* poses,
                            const float* actor_twist, const double* tau, int W, const int32_t* column, const float* g_xyz_s, const float* g_rot_s,
                            float* d_xyz, float* d_rot_raw, float* d_actor_twist, void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_actorsweep_backward";
    const int rc = check_common(fn, P, A, W, xyz, rot_raw, seg_start, poses, actor_twist, tau, workspace, work_bytes);
    if (rc) return rc;
    if (!d_actor_twist) AS_FAIL(LRT_ERR_ARG, "%s: null d_actor_twist pointer", fn);
    if (P > 0 && (!column || !g_xyz_s || !g_rot_s || !d_xyz || !d_rot_raw)) AS_FAIL(LRT_ERR_ARG, "%s: null column / g_xyz_s / g_rot_s / d_xyz / d_rot_raw pointer", fn);
    if (((uintptr_t)g_rot_s & 15) || ((uintptr_t)d_rot_raw & 15)) AS_FAIL(LRT_ERR_ARG, "%s: g_rot_s and d_rot_raw must be 16-byte aligned (float4 rows)", fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) AS_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) AS_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    double* part = (double*)((char*)workspace + table_bytes_of(W));
    hipError_t e;
    if (P > 0) {
        BwdArgs b;
        b.P = (int)P; b.A = A; b.W = W; b.xyz = xyz; b.rot = rot_raw; b.poses = poses; b.twist = actor_twist; b.seg = seg_start; b.tau = tau;
        b.column = column; b.g_xyz = g_xyz_s; b.g_rot = g_rot_s; b.d_xyz = d_xyz; b.d_rot = d_rot_raw; b.d_twist = d_actor_twist; b.part = part;
        hipLaunchKernelGGL(k_as_bwd, dim3((unsigned)((P + NT - 1) / NT)), dim3(NT), 0, stream, b);
        e = hipGetLastError();
        if (e != hipSuccess) AS_FAIL(LRT_ERR_HIP, "%s: launch of the backward failed: %s", fn, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(k_as_finish, dim3((unsigned)A), dim3(NT), 0, stream, (int)P, A, seg_start, poses, actor_twist, part, d_actor_twist);
    e = hipGetLastError();
    if (e != hipSuccess) AS_FAIL(LRT_ERR_HIP, "%s: launch of the finish failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
