// lrt_sweepproj.hip -- the range-image projection under the sweep model (include/lrt_sweepproj.h), gfx950.  Compiled into liblrt_sweepproj.so, a
// library of its own.  No allocation, no host wait; the rule per point is lrt_sweepproj_math.h.
//
//   k_swproj_table     one thread per frame and column: Exp(tau[w] xi_f) by sw_exp, its inverse as 12 doubles in the workspace.  Launched only
//                      with a twist.
//   k_swproj_fill      one thread per pixel of the key image: the word becomes all-ones; the first 7 F threads clear the counts.
//   k_swproj_scatter   one thread per point: its frame (a binary search in `offsets`), the column search against the frame's table (196 KB at
//                      W = 2048: it stays in L2), and ONE 64-bit unsigned atomic min of (bits(r32) << 32) | in-frame index on the pixel's
//                      word, at agent scope.  A plain load first skips the atomic when the word already holds a smaller key: the word only
//                      ever decreases, so what the load saw is an upper bound of it.  The counts points / invalid / out_of_range /
//                      out_of_view / unseen of a workgroup travel as five 12-bit fields of one 64-bit word: summed over the wave by
//                      shuffles, over the four waves in LDS, and added once per counter and frame.
//   k_swproj_resolve   one thread per pixel: the key becomes depth, mask and index, the winner's intensity is gathered.  A workgroup adds
//                      its winners to `pixels` and subtracts them from `hidden`; the workgroup that owns a frame's first pixel adds
//                      points - invalid - out_of_range - out_of_view - unseen, final since the scatter ended, to `hidden`.
//
// The fill and the resolve are those of lrt_project.hip, copied: that file is an input of a source hash of its own.  The atomics are an
// unsigned min and integer adds: they commute, so every output is independent of the arrival order.  There is no float atomic.  A workgroup
// that spans several frames (ragged offsets, H W not a multiple of 256) walks them one after the other.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <float.h>
#include "lrt_device_guard.h"
#include "lrt_sweepproj_math.h"
#include "../../include/lrt_sweepproj.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_SWEEPPROJ_BLOCK;
constexpr int NC = LRT_SWEEPPROJ_N_COUNTS;
constexpr int FIELD = 12;                                          // bits per class in the scatter's packed word: 256 points fit with room
constexpr int N_FIELDS = 5;                                        // the counters the scatter owns: C_POINTS .. C_UNSEEN
constexpr unsigned long long EMPTY = ~0ull;
enum { C_POINTS = 0, C_INVALID = 1, C_RANGE = 2, C_VIEW = 3, C_UNSEEN = 4, C_HIDDEN = 5, C_PIXELS = 6 };

static_assert(NT == 256, "the kernels below are written for four waves");
static_assert(SP_MAX_EVAL == LRT_SWEEPPROJ_MAX_EVAL && SP_TABLE == LRT_SWEEPPROJ_TABLE, "the rule's header and the C ABI disagree");
static_assert(PJ_INVALID == C_INVALID && PJ_OUT_OF_RANGE == C_RANGE && PJ_OUT_OF_VIEW == C_VIEW && SP_UNSEEN == C_UNSEEN, "a drop class is its counter's column");
static_assert(N_FIELDS * FIELD <= 64 && NT < (1 << FIELD), "the packed word");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

__device__ __forceinline__ void count_add(long long* p, long long v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The frame of row i: the last f of [0, F) with offsets[f] <= i (empty frames before it are skipped).  Within [0, F) whatever `offsets` holds.
__device__ __forceinline__ int frame_of(const long long* __restrict__ offsets, int F, long long i)
{
    int lo = 0, hi = F;                                            // the number of f in [0, F) with offsets[f] <= i
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (offsets[mid] <= i) lo = mid + 1; else hi = mid;
    }
    return lo > 0 ? lo - 1 : 0;
}

// ---- table --------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_swproj_table(long long n_cols, int W, const double* __restrict__ twist, const double* __restrict__ tau, double* __restrict__ table)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= n_cols) return;
    const long long f = i / W;
    const int w = (int)(i - f * W);
    double xi[6], E[SP_TABLE];
    for (int k = 0; k < 6; k++) xi[k] = twist[6 * f + k];
    sp_column_entry(xi, tau[w], E);
    for (int k = 0; k < SP_TABLE; k++) table[SP_TABLE * i + k] = E[k];
}

// ---- fill ---------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_swproj_fill(long long n_pix, long long n_counts, unsigned long long* __restrict__ keys, long long* __restrict__ counts)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i < n_pix) keys[i] = EMPTY;
    if (i < n_counts) counts[i] = 0;
}

// ---- scatter ------------------------------------------------------------------------------------------------------------------------------------------
struct ScatterArgs {
    long long N;
    int F;
    const float* points;
    const long long* offsets;
    const double* T;                                               // (F, 3, 4) or null
    const double* table;                                           // (F, W, 12) or null
    const double* inc;
    PjRule rule;
    long long n_pix;
    unsigned long long* keys;
    long long* counts;
};

__global__ __launch_bounds__(NT) void k_swproj_scatter(ScatterArgs a)
{
    __shared__ unsigned long long s_w[NT / 64];
    __shared__ int s_f[2];
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * NT, i = i0 + tid;
    const long long last = (a.N - i0 < NT ? a.N - i0 : NT) - 1;     // the block's last thread with a row
    const bool exists = i < a.N;
    int f = 0;
    unsigned long long word = 0;
    if (exists) {
        f = frame_of(a.offsets, a.F, i);
        const float x = a.points[4 * i], y = a.points[4 * i + 1], z = a.points[4 * i + 2];
        int w, h, evals;
        float r32;
        const int cls = sp_point(a.T ? a.T + 12 * (long long)f : nullptr, x, y, z, a.table ? a.table + (long long)f * a.rule.W * SP_TABLE : nullptr,
                                 a.rule, a.inc, &w, &h, &r32, &evals);
        word = 1ull | (cls != PJ_KEEP ? 1ull << (FIELD * cls) : 0ull);   // the drop classes 1 .. 4 are the counters' columns
        if (cls == PJ_KEEP) {
            const long long pix = ((long long)f * a.rule.H + h) * a.rule.W + w;
            const unsigned long long key = ((unsigned long long)__float_as_uint(r32) << 32) | (unsigned long long)(unsigned)(i - a.offsets[f]);
            if (pix >= 0 && pix < a.n_pix) {
                unsigned long long* p = a.keys + pix;
                if (*(volatile unsigned long long*)p > key) __hip_atomic_fetch_min(p, key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
    if (tid == 0) s_f[0] = f;
    if (tid == last) s_f[1] = f;
    __syncthreads();
    const int f_lo = s_f[0], f_hi = s_f[1];
    for (int g = f_lo; g <= f_hi; g++) {                             // uniform over the workgroup
        if (a.offsets[g + 1] <= a.offsets[g] && g != f_lo && g != f_hi) continue;     // an empty frame in between
        unsigned long long v = (exists && f == g) ? word : 0ull;
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);     // every field stays at or below 256: no carry between the 12-bit fields
        if ((tid & 63) == 0) s_w[tid >> 6] = v;
        __syncthreads();
        if (tid < N_FIELDS) {
            unsigned long long t = 0;
            for (int k = 0; k < NT / 64; k++) t += s_w[k];
            const long long n = (long long)((t >> (FIELD * tid)) & ((1ull << FIELD) - 1));
            if (n) count_add(a.counts + (long long)g * NC + tid, n);
        }
        __syncthreads();
    }
}

// ---- resolve ------------------------------------------------------------------------------------------------------------------------------------------
struct ResolveArgs {
    long long N, n_pix, hw;
    int F;
    const float* points;
    const long long* offsets;
    const unsigned long long* keys;
    float *depth, *intensity;
    unsigned char* mask;
    int* index;
    long long* counts;
};

__global__ __launch_bounds__(NT) void k_swproj_resolve(ResolveArgs a)
{
    __shared__ unsigned s_n[NT / 64];
    const int tid = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * NT, i = i0 + tid;
    const long long i1 = (a.n_pix < i0 + NT ? a.n_pix : i0 + NT) - 1; // the block's last pixel
    const bool exists = i < a.n_pix;
    int f = 0;
    bool hit = false;
    if (exists) {
        f = (int)(i / a.hw);
        const unsigned long long key = a.keys[i];
        hit = key != EMPTY;
        float d = 0.f, it = 0.f;
        int idx = -1;
        if (hit) {
            d = __uint_as_float((unsigned)(key >> 32));
            idx = (int)(unsigned)(key & 0xFFFFFFFFull);
            const long long row = a.offsets[f] + (long long)idx;
            if (row >= 0 && row < a.N) it = a.points[4 * row + 3];
        }
        a.depth[i] = d; a.intensity[i] = it; a.mask[i] = hit ? 1 : 0; a.index[i] = idx;
    }
    const int f_lo = (int)(i0 / a.hw), f_hi = (int)(i1 / a.hw);
    for (int g = f_lo; g <= f_hi; g++) {                             // uniform over the workgroup
        const unsigned long long m = __ballot(exists && hit && f == g);
        if ((tid & 63) == 0) s_n[tid >> 6] = (unsigned)__popcll(m);
        __syncthreads();
        if (tid == 0) {
            long long n = 0;
            for (int k = 0; k < NT / 64; k++) n += s_n[k];
            long long* c = a.counts + (long long)g * NC;
            if (n) count_add(c + C_PIXELS, n);
            long long hidden = -n;
            const long long first = (long long)g * a.hw;             // the frame's first pixel: this block owns it exactly when it lies in the block
            if (first >= i0 && first <= i1) hidden += c[C_POINTS] - c[C_INVALID] - c[C_RANGE] - c[C_VIEW] - c[C_UNSEEN];
            if (hidden) count_add(c + C_HIDDEN, hidden);
        }
        __syncthreads();
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define SP_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

// Bytes of the key image, or -1.
static long long key_bytes_of(long long F, int H, int W)
{
    if (F < 1 || H < 1 || W < 1) return -1;
    const long long hw = (long long)H * W;
    if (hw > LRT_SWEEPPROJ_MAX_PIXELS || F > LRT_SWEEPPROJ_MAX_PIXELS / hw) return -1;
    return F * hw * 8;
}

static long long work_bytes_of(long long F, int H, int W)
{
    const long long keys = key_bytes_of(F, H, W);
    if (keys < 0) return -1;
    return round256(keys + F * W * (long long)(SP_TABLE * sizeof(double)));
}

extern "C" {

int lrt_sweepproj_abi_version(void) { return LRT_SWEEPPROJ_ABI_VERSION; }

const char* lrt_sweepproj_last_error(void) { return g_err; }

long long lrt_sweepproj_work_bytes(long long F, int H, int W) { return work_bytes_of(F, H, W); }

int lrt_sweepproj_points(int device, long long N, const float* points, long long F, const long long* offsets, const double* points2sensor,
                         const double* twist, const double* tau, int H, int W, const double* inclination, int n_inc, double off, double yaw,
                         double min_depth, double max_depth, int wrap,
                         float* depth, float* intensity, unsigned char* mask, int* index, long long* counts,
                         void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_sweepproj_points";
    if (N < 0 || N > LRT_SWEEPPROJ_MAX_POINTS) SP_FAIL(LRT_ERR_ARG, "%s: %lld points (0 .. %lld: the in-frame index is int32)", fn, N, LRT_SWEEPPROJ_MAX_POINTS);
    const long long need = work_bytes_of(F, H, W);
    if (need < 0) SP_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d pixels (each at least 1, F H W at most %lld)", fn, F, H, W, LRT_SWEEPPROJ_MAX_PIXELS);
    if (n_inc != 2 && (n_inc != H || H < 3)) SP_FAIL(LRT_ERR_ARG, "%s: %d inclinations (2 bounds, or one per row of at least 3: %d)", fn, n_inc, H);
    if (!(off >= 0.0 && off < 1.0)) SP_FAIL(LRT_ERR_ARG, "%s: pixel offset %g (0 for KITTI, 0.5 for Waymo)", fn, off);
    if (!pj_finite(yaw)) SP_FAIL(LRT_ERR_ARG, "%s: yaw %g", fn, yaw);
    if (!(min_depth >= 0.0 && min_depth < max_depth && max_depth <= (double)FLT_MAX)) SP_FAIL(LRT_ERR_ARG, "%s: depths (%g, %g] (0 <= min < max <= FLT_MAX)", fn, min_depth, max_depth);
    if (wrap != 0 && wrap != 1) SP_FAIL(LRT_ERR_ARG, "%s: wrap %d (0 or 1)", fn, wrap);
    if (N > 0 && !points) SP_FAIL(LRT_ERR_ARG, "%s: null points pointer", fn);
    if (!offsets || !inclination) SP_FAIL(LRT_ERR_ARG, "%s: null offsets / inclination pointer", fn);
    if (twist && !tau) SP_FAIL(LRT_ERR_ARG, "%s: null tau pointer with a twist (the column times are required then)", fn);
    if (!depth || !intensity || !mask || !index || !counts) SP_FAIL(LRT_ERR_ARG, "%s: null depth / intensity / mask / index / counts pointer", fn);
    if (!workspace || ((uintptr_t)workspace & 255)) SP_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) SP_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld frames of %d x %d need %lld", fn, work_bytes, F, H, W, need);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) SP_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) SP_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const long long hw = (long long)H * W, n_pix = F * hw, n_counts = F * NC, n_cols = F * W;
    unsigned long long* keys = (unsigned long long*)workspace;
    double* table = (double*)(keys + n_pix);                       // 8-byte aligned behind the key image
    hipError_t e;
    if (twist) {
        hipLaunchKernelGGL(k_swproj_table, dim3((unsigned)((n_cols + NT - 1) / NT)), dim3(NT), 0, stream, n_cols, W, twist, tau, table);
        e = hipGetLastError();
        if (e != hipSuccess) SP_FAIL(LRT_ERR_HIP, "%s: launch of the table failed: %s", fn, hipGetErrorString(e));
    }
    const long long n_fill = n_pix > n_counts ? n_pix : n_counts;
    hipLaunchKernelGGL(k_swproj_fill, dim3((unsigned)((n_fill + NT - 1) / NT)), dim3(NT), 0, stream, n_pix, n_counts, keys, counts);
    e = hipGetLastError();
    if (e != hipSuccess) SP_FAIL(LRT_ERR_HIP, "%s: launch of the fill failed: %s", fn, hipGetErrorString(e));
    if (N > 0) {
        ScatterArgs s;
        s.N = N; s.F = (int)F; s.points = points; s.offsets = offsets; s.T = points2sensor; s.table = twist ? table : nullptr; s.inc = inclination;
        s.rule.H = H; s.rule.W = W; s.rule.n_inc = n_inc; s.rule.wrap = wrap; s.rule.off = off; s.rule.yaw = yaw; s.rule.min_depth = min_depth; s.rule.max_depth = max_depth;
        s.n_pix = n_pix; s.keys = keys; s.counts = counts;
        hipLaunchKernelGGL(k_swproj_scatter, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, stream, s);
        e = hipGetLastError();
        if (e != hipSuccess) SP_FAIL(LRT_ERR_HIP, "%s: launch of the scatter failed: %s", fn, hipGetErrorString(e));
    }
    ResolveArgs r;
    r.N = N; r.n_pix = n_pix; r.hw = hw; r.F = (int)F; r.points = points; r.offsets = offsets; r.keys = keys;
    r.depth = depth; r.intensity = intensity; r.mask = mask; r.index = index; r.counts = counts;
    hipLaunchKernelGGL(k_swproj_resolve, dim3((unsigned)((n_pix + NT - 1) / NT)), dim3(NT), 0, stream, r);
    e = hipGetLastError();
    if (e != hipSuccess) SP_FAIL(LRT_ERR_HIP, "%s: launch of the resolve failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
