// lrt_unproject.hip -- the point clouds of range images (include/lrt_unproject.h), gfx950.  Compiled into liblrt_unproject.so, a library of its
// own.  No allocation, no host wait, no atomic; the rule per pixel is lrt_unproject_math.h.
//
//   k_up_count   256-thread workgroups; a workgroup owns 256 consecutive pixels of ONE frame (the grid is F * ceil(H W / 256), the last workgroup
//                of a frame may be partly empty).  The class of every pixel, one wave64 ballot and popcount per class, the four waves summed
//                through LDS: one record (kept, invalid, masked, out_of_range) per workgroup.
//   k_up_scan    ONE workgroup walks the records in chunks of 256 and carries the four running totals in int64: every workgroup's base row,
//                `offsets` at the first workgroup of a frame, the running totals at the last one; then `counts` from the differences.
//   k_up_write   the class again -- a pure function of the inputs, so both passes agree -- the rank inside the wave from the ballot's lower
//                lanes, the waves' offsets through LDS, and one 16-byte row plus one int32 per kept pixel.
//
// Every row has one writer and nothing is accumulated in memory: the result does not depend on the order in which workgroups run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <float.h>
#include "lrt_device_guard.h"
#include "lrt_unproject_math.h"
#include "../../include/lrt_unproject.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_UNPROJECT_BLOCK;
constexpr int NW = NT / 64;
constexpr int NC = LRT_UNPROJECT_N_COUNTS;
enum { C_PIXELS = 0, C_INVALID = 1, C_MASKED = 2, C_RANGE = 3, C_POINTS = 4 };

static_assert(NT == 256, "the kernels below are written for four waves");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

struct UpArgs {
    long long hw, cap;                                             // pixels of a frame, of all frames
    unsigned nb;                                                   // workgroups per frame
    int W;
    const float *depth, *rays_o, *rays_d, *intensity, *raydrop;
    const unsigned char* keep;
    const double* T;                                               // null, (F, 3, 4) or (F, W, 3, 4)
    int per_column;
    UpRule rule;
    uint4* wg;                                                     // per workgroup: kept, invalid, masked, out_of_range
    const long long* base;                                         // per workgroup: its first row
    float4* points;
    int* pixel;
};

// The class of pixel p of frame f (p < hw); r, o and d are what it read.
__device__ __forceinline__ int class_at(const UpArgs& a, long long i, float* r, float* o, float* d)
{
    *r = a.depth[i];
    for (int k = 0; k < 3; k++) { o[k] = a.rays_o[3 * i + k]; d[k] = a.rays_d[3 * i + k]; }
    const unsigned char keep = a.rule.has_keep ? a.keep[i] : (unsigned char)1;
    const float drop = a.rule.has_drop ? a.raydrop[i] : 0.f;
    return up_classify(*r, o, d, keep, drop, a.rule);
}

// ---- count --------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_up_count(UpArgs a)
{
    __shared__ unsigned s_n[4][NW];
    const int tid = threadIdx.x;
    const unsigned b = blockIdx.x, f = b / a.nb, j = b - f * a.nb;
    const long long p = (long long)j * NT + tid;
    int cls = -1;
    if (p < a.hw) {
        float r, o[3], d[3];
        cls = class_at(a, (long long)f * a.hw + p, &r, o, d);
    }
    const unsigned long long m0 = __ballot(cls == UP_KEEP), m1 = __ballot(cls == UP_INVALID), m2 = __ballot(cls == UP_MASKED), m3 = __ballot(cls == UP_OUT_OF_RANGE);
    if ((tid & 63) == 0) {
        const int w = tid >> 6;
        s_n[0][w] = (unsigned)__popcll(m0); s_n[1][w] = (unsigned)__popcll(m1); s_n[2][w] = (unsigned)__popcll(m2); s_n[3][w] = (unsigned)__popcll(m3);
    }
    __syncthreads();
    if (tid == 0) {
        unsigned t[4];
        for (int k = 0; k < 4; k++) { t[k] = 0; for (int w = 0; w < NW; w++) t[k] += s_n[k][w]; }
        a.wg[b] = make_uint4(t[0], t[1], t[2], t[3]);
    }
}

// ---- scan ---------------------------------------------------------------------------------------------------------------------------------------------
struct ScanArgs {
    long long G, F, hw;                                            // workgroups of the count, frames, pixels of a frame
    unsigned nb;
    const uint4* wg;
    long long *base, *cum;                                         // cum (F, 4): the running totals behind a frame's last workgroup
    long long *offsets, *counts;
};

__global__ __launch_bounds__(NT) void k_up_scan(ScanArgs a)
{
    __shared__ unsigned s_w[NW][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry[4] = {0, 0, 0, 0};                             // uniform over the workgroup
    for (long long c0 = 0; c0 < a.G; c0 += NT) {
        const long long b = c0 + tid;
        const uint4 own = b < a.G ? a.wg[b] : make_uint4(0, 0, 0, 0);
        unsigned v[4] = {own.x, own.y, own.z, own.w};               // a chunk's totals are at most 256 * 256: 32 bits hold them
        for (int d = 1; d < 64; d <<= 1)
            for (int k = 0; k < 4; k++) {
                const unsigned t = __shfl_up(v[k], d);
                if (lane >= d) v[k] += t;
            }
        if (lane == 63) for (int k = 0; k < 4; k++) s_w[wave][k] = v[k];
        __syncthreads();
        unsigned tot[4];
        for (int k = 0; k < 4; k++) {
            unsigned before = 0, all = 0;
            for (int w = 0; w < NW; w++) { if (w < wave) before += s_w[w][k]; all += s_w[w][k]; }
            v[k] += before; tot[k] = all;
        }
        if (b < a.G) {
            const long long first = carry[0] + (long long)(v[0] - own.x);
            a.base[b] = first;
            const long long f = b / a.nb, j = b - f * a.nb;
            if (j == 0) a.offsets[f] = first;
            if (j == (long long)a.nb - 1) for (int k = 0; k < 4; k++) a.cum[4 * f + k] = carry[k] + (long long)v[k];
        }
        for (int k = 0; k < 4; k++) carry[k] += (long long)tot[k];
        __syncthreads();                                            // s_w is written again by the next chunk
    }
    if (tid == 0) a.offsets[a.F] = carry[0];
    __syncthreads();                                                // cum: written above by this workgroup, read below by other threads of it
    for (long long f = tid; f < a.F; f += NT) {
        long long c[4];
        for (int k = 0; k < 4; k++) c[k] = a.cum[4 * f + k] - (f > 0 ? a.cum[4 * (f - 1) + k] : 0);
        long long* o = a.counts + f * NC;
        o[C_PIXELS] = a.hw; o[C_INVALID] = c[1]; o[C_MASKED] = c[2]; o[C_RANGE] = c[3]; o[C_POINTS] = c[0];
    }
}

// ---- write --------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_up_write(UpArgs a)
{
    __shared__ unsigned s_n[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const unsigned b = blockIdx.x, f = b / a.nb, j = b - f * a.nb;
    const long long p = (long long)j * NT + tid;
    const long long i = (long long)f * a.hw + p;
    bool kept = false;
    float r = 0.f, o[3], d[3];
    if (p < a.hw) kept = class_at(a, i, &r, o, d) == UP_KEEP;
    const unsigned long long m = __ballot(kept);
    if (lane == 0) s_n[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (!kept) return;
    unsigned before = 0;
    for (int w = 0; w < NW; w++) if (w < wave) before += s_n[w];
    const long long row = a.base[b] + (long long)before + (long long)__popcll(m & ((1ull << lane) - 1ull));
    if (row < 0 || row >= a.cap) return;                            // never taken: the bases are the scan of these very counts
    float q[3];
    if (a.T) {
        const long long t = a.per_column ? (long long)f * a.W + (p % a.W) : (long long)f;
        up_point64(r, o, d, a.T + 12 * t, q);
    } else {
        up_point32(r, o, d, q);
    }
    a.points[row] = make_float4(q[0], q[1], q[2], a.intensity ? a.intensity[i] : 0.f);
    a.pixel[row] = (int)p;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define UP_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

// The workgroups per frame and the number of workgroups; false for sizes outside the ABI.
static bool sizes_of(long long F, int H, int W, long long* hw, long long* nb, long long* G)
{
    if (F < 1 || H < 1 || W < 1) return false;
    *hw = (long long)H * W;
    if (*hw > LRT_UNPROJECT_MAX_PIXELS || F > LRT_UNPROJECT_MAX_PIXELS / *hw) return false;
    *nb = (*hw + NT - 1) / NT;
    *G = F * *nb;                                                   // at most F H W
    return *G <= LRT_UNPROJECT_MAX_WORKGROUPS;                       // the grid: G workgroups of 256 threads, below 2^32 threads
}

static long long work_bytes_of(long long F, int H, int W)
{
    long long hw, nb, G;
    if (!sizes_of(F, H, W, &hw, &nb, &G)) return -1;
    return round256(G * 16) + round256(G * 8) + round256(F * 32);
}

extern "C" {

int lrt_unproject_abi_version(void) { return LRT_UNPROJECT_ABI_VERSION; }

const char* lrt_unproject_last_error(void) { return g_err; }

long long lrt_unproject_work_bytes(long long F, int H, int W) { return work_bytes_of(F, H, W); }

int lrt_unproject_points(int device, long long F, int H, int W, const float* depth, const float* rays_o, const float* rays_d, const float* intensity,
                         const unsigned char* keep, const float* raydrop, double raydrop_ratio, const double* world2out, int per_column,
                         double min_depth, double max_depth, float* points, int* pixel, long long* offsets, long long* counts,
                         void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_unproject_points";
    long long hw, nb, G;
    if (!sizes_of(F, H, W, &hw, &nb, &G)) UP_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d pixels (each at least 1, F H W at most %lld, F ceil(H W / %d) at most %lld)", fn, F, H, W, LRT_UNPROJECT_MAX_PIXELS, NT, LRT_UNPROJECT_MAX_WORKGROUPS);
    const long long need = work_bytes_of(F, H, W);
    if (!(min_depth >= 0.0 && min_depth < max_depth && max_depth <= (double)FLT_MAX)) UP_FAIL(LRT_ERR_ARG, "%s: depths (%g, %g] (0 <= min < max <= FLT_MAX)", fn, min_depth, max_depth);
    if (raydrop && !(raydrop_ratio == raydrop_ratio)) UP_FAIL(LRT_ERR_ARG, "%s: a NaN ray-drop ratio", fn);
    if (per_column != 0 && per_column != 1) UP_FAIL(LRT_ERR_ARG, "%s: per_column %d (0 or 1)", fn, per_column);
    if (per_column && !world2out) UP_FAIL(LRT_ERR_ARG, "%s: per_column without a transform table", fn);
    if (!depth || !rays_o || !rays_d) UP_FAIL(LRT_ERR_ARG, "%s: null depth / rays_o / rays_d pointer", fn);
    if (!points || !pixel || !offsets || !counts) UP_FAIL(LRT_ERR_ARG, "%s: null points / pixel / offsets / counts pointer", fn);
    if ((uintptr_t)points & 15) UP_FAIL(LRT_ERR_ARG, "%s: points must be 16-byte aligned (a row is stored as one word)", fn);
    if (!workspace || ((uintptr_t)workspace & 255)) UP_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) UP_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld frames of %d x %d need %lld", fn, work_bytes, F, H, W, need);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) UP_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) UP_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    uint4* wg = (uint4*)ws;
    long long* base = (long long*)(ws + round256(G * 16));
    long long* cum = (long long*)(ws + round256(G * 16) + round256(G * 8));
    UpArgs a;
    a.hw = hw; a.cap = F * hw; a.nb = (unsigned)nb; a.W = W;
    a.depth = depth; a.rays_o = rays_o; a.rays_d = rays_d; a.intensity = intensity; a.raydrop = raydrop; a.keep = keep;
    a.T = world2out; a.per_column = per_column;
    a.rule.has_keep = keep ? 1 : 0; a.rule.has_drop = raydrop ? 1 : 0; a.rule.ratio = raydrop ? (float)raydrop_ratio : 0.f;
    a.rule.min_depth = min_depth; a.rule.max_depth = max_depth;
    a.wg = wg; a.base = base; a.points = (float4*)points; a.pixel = pixel;
    hipLaunchKernelGGL(k_up_count, dim3((unsigned)G), dim3(NT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) UP_FAIL(LRT_ERR_HIP, "%s: launch of the count failed: %s", fn, hipGetErrorString(e));
    ScanArgs s;
    s.G = G; s.F = F; s.hw = hw; s.nb = (unsigned)nb; s.wg = wg; s.base = base; s.cum = cum; s.offsets = offsets; s.counts = counts;
    hipLaunchKernelGGL(k_up_scan, dim3(1), dim3(NT), 0, stream, s);
    e = hipGetLastError();
    if (e != hipSuccess) UP_FAIL(LRT_ERR_HIP, "%s: launch of the scan failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_up_write, dim3((unsigned)G), dim3(NT), 0, stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) UP_FAIL(LRT_ERR_HIP, "%s: launch of the write failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
