// lrt_segment.hip -- the range-image segmentation (include/lrt_segment.h), gfx950.  Compiled into liblrt_segment.so, a library of its own.  No
// allocation, no host wait, no float atomic; the rules are lrt_segment_math.h on top of lrt_project_math.h.
//
//   k_seg_ground         one lane per (frame, column), consecutive lanes on consecutive columns: every row step is one coalesced load of a wave.
//   k_seg_label_init     one lane per pixel, lanes along w.  A lane that is joined to its left neighbour IN THE SAME WAVE learns the start of its
//                        run from one ballot: label = the run's first index (a parent that is smaller and of the same component), -1 if not kept.
//   k_seg_label_merge    the pairs the ballot did not see -- the left neighbour across a wave's edge, the upper neighbour, the seam (h, 0) <->
//                        (h, W - 1) -- by union-find in `label`: find without compression, atomicMin on the larger root, retried with what it
//                        displaced.  Parents only decrease, every retry makes progress somewhere: lock-free, a fixed three launches.
//   k_seg_label_flatten  label = the root.  A root is the smallest index of its component (the smallest has no smaller parent), so the bits do
//                        not depend on the arrival order.
//   k_seg_freespace      one lane per source pixel, as k_reg_linearize walks its window.
//   k_seg_fill           the table's zeros;  k_seg_bounds_fill  the bounds' sentinels and the zero counts.
//   k_seg_count / k_seg_scan / k_seg_number   the ballot count, one-workgroup scan (per frame) and write shape of lrt_unproject.hip, restated: the
//                        roots of a frame numbered in ascending index; k_seg_number also starts the rows of the table.
//   k_seg_accumulate     one lane per pixel: its segment's dense id from the root's, then 64-bit integer atomics into the row (add, min, max of
//                        integers: the order cannot show).  Not pre-aggregated per wave: see profiles/segmentation.md.
//   k_seg_bounds         one lane per pixel of a tracked segment: integer min / max / count per track.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_segment_math.h"
#include "../../include/lrt_segment.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_SEGMENT_BLOCK;
constexpr int NW = NT / 64;
constexpr int NC = LRT_SEGMENT_NCOL;

static_assert(NT == 256, "the kernels below are written for four waves");
static_assert(NC == SG_NCOL, "the header and the rule disagree");

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }

// ---- ground -------------------------------------------------------------------------------------------------------------------------------------------
struct GroundArgs {
    int H, W, n_inc;
    const double* inc;
    const float* points;
    const unsigned char* mask;
    double up[3], z_lo, z_hi, slope;
    unsigned char* ground;
};

__global__ __launch_bounds__(64) void k_seg_ground(GroundArgs a)
{
    const int w = blockIdx.x * 64 + threadIdx.x;
    if (w >= a.W) return;
    const long long base = (long long)blockIdx.y * a.H * a.W;
    const double ends[2] = {a.inc[0], a.inc[a.n_inc - 1]};            // read once: the direction of the row order
    const double up[3] = {a.up[0], a.up[1], a.up[2]};
    SgGround s;
    s.have = 0; s.h = 0.0; s.g[0] = 0.0; s.g[1] = 0.0; s.g[2] = 0.0;
    for (int k = 0; k < a.H; k++) {
        const long long i = base + (long long)sg_row_at(k, a.H, ends, 2) * a.W + w;
        unsigned char g = 0;
        if (a.mask[i]) {
            const float p[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
            g = (unsigned char)sg_ground_step(p, up, a.z_lo, a.z_hi, a.slope, &s);
        }
        a.ground[i] = g;
    }
}

// ---- labels -------------------------------------------------------------------------------------------------------------------------------------------
struct LabelArgs {
    int H, W, HW;
    const float* points;
    const unsigned char *mask, *exclude;
    float dabs2, ch2, cv2;
    int* label;
};

__device__ __forceinline__ bool kept_at(const LabelArgs& a, long long i) { return a.mask[i] && !(a.exclude && a.exclude[i]); }

__device__ __forceinline__ bool joined(const LabelArgs& a, long long i, long long j, float cdir2)
{
    const float p[3] = {a.points[3 * i], a.points[3 * i + 1], a.points[3 * i + 2]};
    const float q[3] = {a.points[3 * j], a.points[3 * j + 1], a.points[3 * j + 2]};
    return sg_join(p, q, a.dabs2, cdir2);
}

__global__ __launch_bounds__(NT) void k_seg_label_init(LabelArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * NT + threadIdx.x;                      // a workgroup starts at a multiple of 256: lane == i & 63
    const long long base = (long long)blockIdx.y * a.HW;
    const bool in = i < a.HW;
    const bool kept = in && kept_at(a, base + i);
    bool jl = false;                                                  // joined to the pixel one lane below, in the same row
    if (kept && lane > 0 && (i % a.W) > 0 && kept_at(a, base + i - 1)) jl = joined(a, base + i, base + i - 1, a.ch2);
    const unsigned long long heads = __ballot(!jl);                   // lane 0 is always one
    const unsigned long long below = heads & (lane == 63 ? ~0ull : ((2ull << lane) - 1ull));
    const int start = 63 - __clzll((long long)below);
    if (in) a.label[base + i] = kept ? i - (lane - start) : -1;
}

__device__ __forceinline__ int uf_find(int* L, int x)
{
    int p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    while (p != x) { x = p; p = __hip_atomic_load(L + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
    return x;
}

__device__ __forceinline__ void uf_union(int* L, int x, int y)
{
    for (;;) {
        x = uf_find(L, x); y = uf_find(L, y);
        if (x == y) return;
        if (x > y) { const int t = x; x = y; y = t; }                  // x < y: the larger root is hung under the smaller
        const int old = atomicMin(L + y, x);
        if (old == y) return;                                         // y was still a root
        y = old;                                                      // someone hung y elsewhere first: what it points to now is joined with x next
    }
}

__global__ __launch_bounds__(NT) void k_seg_label_merge(LabelArgs a)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.HW) return;
    const long long base = (long long)blockIdx.y * a.HW;
    if (!kept_at(a, base + i)) return;
    int* L = a.label + base;
    const int h = i / a.W, w = i - h * a.W;
    if (w > 0 && lane == 0 && kept_at(a, base + i - 1) && joined(a, base + i, base + i - 1, a.ch2)) uf_union(L, i, i - 1);
    if (w == 0 && a.W > 1 && kept_at(a, base + i + a.W - 1) && joined(a, base + i, base + i + a.W - 1, a.ch2)) uf_union(L, i, i + a.W - 1);
    if (h > 0 && kept_at(a, base + i - a.W) && joined(a, base + i, base + i - a.W, a.cv2)) uf_union(L, i, i - a.W);
}

__global__ __launch_bounds__(NT) void k_seg_label_flatten(LabelArgs a)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.HW) return;
    int* L = a.label + (long long)blockIdx.y * a.HW;
    if (__hip_atomic_load(L + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
    const int r = uf_find(L, i);
    __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // a root for an ancestor: other lanes' walks stay right
}

// ---- free space ---------------------------------------------------------------------------------------------------------------------------------------
struct FreeArgs {
    int HW;
    PjRule rule;
    const double* inc;
    const float *sp, *tr;
    const unsigned char *sm, *tm;
    const double* X;
    int rh, rw;
    double m_abs, m_rel;
    signed char* ev;
};

__global__ __launch_bounds__(NT) void k_seg_freespace(FreeArgs a)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.HW) return;
    const long long f = blockIdx.y, base = f * a.HW;
    int ev = -1;
    if (a.sm[base + i]) {
        const float p[3] = {a.sp[3 * (base + i)], a.sp[3 * (base + i) + 1], a.sp[3 * (base + i) + 2]};
        ev = sg_freespace(a.X + 12 * f, p, a.rule, a.inc, a.tr + base, a.tm + base, a.rh, a.rw, a.m_abs, a.m_rel);
    }
    a.ev[base + i] = (signed char)ev;
}

// ---- the table ----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_seg_fill(long long* out, long long n)
{
    for (long long k = (long long)blockIdx.x * NT + threadIdx.x; k < n; k += (long long)gridDim.x * NT) out[k] = 0;
}

struct StatArgs {
    int HW, nb, S_max;
    const float* points;
    const int* label;
    const signed char *ev0, *ev1;
    unsigned* wg;                                                    // (F, nb): roots per workgroup
    unsigned* first;                                                 // (F, nb): the rank of a workgroup's first root
    int *seg, *n_seg, *overflow;
    long long* table;
};

__device__ __forceinline__ bool root_at(const StatArgs& a, long long base, int i) { return i < a.HW && a.label[base + i] == i; }

__global__ __launch_bounds__(NT) void k_seg_count(StatArgs a)
{
    __shared__ unsigned s_n[NW];
    const int tid = threadIdx.x;
    const int i = blockIdx.x * NT + tid;
    const long long base = (long long)blockIdx.y * a.HW;
    const unsigned long long m = __ballot(root_at(a, base, i));
    if ((tid & 63) == 0) s_n[tid >> 6] = (unsigned)__popcll(m);
    __syncthreads();
    if (tid == 0) a.wg[(long long)blockIdx.y * a.nb + blockIdx.x] = s_n[0] + s_n[1] + s_n[2] + s_n[3];
}

__global__ __launch_bounds__(NT) void k_seg_scan(StatArgs a)
{
    __shared__ unsigned s_w[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long f = blockIdx.x;
    unsigned carry = 0;                                               // uniform over the workgroup; a frame has fewer than 2^31 pixels
    for (int c0 = 0; c0 < a.nb; c0 += NT) {
        const int b = c0 + tid;
        const unsigned own = b < a.nb ? a.wg[f * a.nb + b] : 0u;
        unsigned v = own;
        for (int d = 1; d < 64; d <<= 1) {
            const unsigned t = __shfl_up(v, d);
            if (lane >= d) v += t;
        }
        if (lane == 63) s_w[wave] = v;
        __syncthreads();
        unsigned before = 0, all = 0;
        for (int w = 0; w < NW; w++) { if (w < wave) before += s_w[w]; all += s_w[w]; }
        if (b < a.nb) a.first[f * a.nb + b] = carry + before + v - own;
        carry += all;
        __syncthreads();                                              // s_w is written again by the next chunk
    }
    if (tid == 0) {
        const unsigned cap = (unsigned)a.S_max;
        a.n_seg[f] = (int)(carry < cap ? carry : cap);
        a.overflow[f] = (int)(carry > cap ? carry - cap : 0u);
    }
}

__global__ __launch_bounds__(NT) void k_seg_number(StatArgs a)
{
    __shared__ unsigned s_n[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int i = blockIdx.x * NT + tid;
    const long long f = blockIdx.y, base = f * a.HW;
    const bool root = root_at(a, base, i);
    const unsigned long long m = __ballot(root);
    if (lane == 0) s_n[wave] = (unsigned)__popcll(m);
    __syncthreads();
    if (i >= a.HW) return;
    int id = -1;
    if (root) {
        unsigned before = 0;
        for (int w = 0; w < NW; w++) if (w < wave) before += s_n[w];
        const unsigned rank = a.first[f * a.nb + blockIdx.x] + before + (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (rank < (unsigned)a.S_max) {
            id = (int)rank;
            long long* row = a.table + (f * a.S_max + id) * NC;       // the fill has zeroed it
            row[SG_ROOT] = i;
            for (int k = 0; k < 3; k++) { row[SG_MIN + k] = INT64_MAX; row[SG_MAX + k] = INT64_MIN; }
        }
    }
    a.seg[base + i] = id;
}

__device__ __forceinline__ void add64(long long* p, long long v)
{
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(NT) void k_seg_accumulate(StatArgs a)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.HW) return;
    const long long f = blockIdx.y, base = f * a.HW;
    const int r = a.label[base + i];
    if (r < 0 || r >= a.HW) return;                                   // not kept: k_seg_number wrote its -1
    const int id = a.seg[base + r];                                   // a root's entry: written by k_seg_number, by no lane of this launch
    if (r != i) a.seg[base + i] = id;
    if (id < 0 || id >= a.S_max) return;
    long long* row = a.table + (f * a.S_max + id) * NC;
    add64(row + SG_COUNT, 1);
    if (a.ev0) { const int e = a.ev0[base + i]; if (e == 1) add64(row + SG_EV, 1); if (e >= 0) add64(row + SG_EV + 1, 1); }
    if (a.ev1) { const int e = a.ev1[base + i]; if (e == 1) add64(row + SG_EV + 2, 1); if (e >= 0) add64(row + SG_EV + 3, 1); }
    for (int k = 0; k < 3; k++) {
        const long long q = sg_quant(a.points[3 * (base + i) + k]);
        add64(row + SG_SUM + k, q);
        __hip_atomic_fetch_min(row + SG_MIN + k, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(row + SG_MAX + k, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---- track bounds -------------------------------------------------------------------------------------------------------------------------------------
struct BoundArgs {
    int HW, S_max, NTR;
    long long F;
    const float* points;
    const int *seg, *track_of;
    const double* pose;
    long long *bounds, *count;
};

__global__ __launch_bounds__(NT) void k_seg_bounds(BoundArgs a)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= a.HW) return;
    const long long f = blockIdx.y, base = f * a.HW;
    const int s = a.seg[base + i];
    if (s < 0 || s >= a.S_max) return;
    const int t = a.track_of[f * a.S_max + s];
    if (t < 0 || t >= a.NTR) return;
    const float p[3] = {a.points[3 * (base + i)], a.points[3 * (base + i) + 1], a.points[3 * (base + i) + 2]};
    double c[3];
    sg_actor_point(a.pose + ((long long)t * a.F + f) * 12, p, c);
    for (int k = 0; k < 3; k++) {
        const long long q = sg_quant64(c[k]);
        __hip_atomic_fetch_min(a.bounds + 6 * t + k, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_max(a.bounds + 6 * t + 3 + k, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    add64(a.count + t, 1);
}

__global__ __launch_bounds__(NT) void k_seg_bounds_fill(long long* bounds, long long* count, int n)
{
    const int t = blockIdx.x * NT + threadIdx.x;
    if (t >= n) return;
    for (int k = 0; k < 3; k++) { bounds[6 * t + k] = INT64_MAX; bounds[6 * t + 3 + k] = INT64_MIN; }
    count[t] = 0;
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define SG_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)
#define SG_LAUNCHED(what) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) SG_FAIL(LRT_ERR_HIP, "%s: launch of %s failed: %s", fn, what, hipGetErrorString(e_)); } while (0)

static inline long long n_wg_of(long long hw) { return (hw + NT - 1) / NT; }

static bool sizes_ok(long long F, int H, int W)
{
    if (F < 1 || H < 1 || W < 1 || F > LRT_SEGMENT_MAX_FRAMES) return false;
    const long long hw = (long long)H * W;
    return hw <= LRT_SEGMENT_MAX_PIXELS && F <= LRT_SEGMENT_MAX_PIXELS / hw;
}

static long long work_bytes_of(long long F, int H, int W)
{
    if (!sizes_ok(F, H, W)) return -1;
    return 2 * round256(4 * F * n_wg_of((long long)H * W));
}

static bool finite_d(double x) { return x - x == 0.0; }

static int check_sizes(const char* fn, long long F, int H, int W)
{
    if (!sizes_ok(F, H, W))
        SG_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d pixels (each at least 1, at most %d frames, F H W at most %lld)", fn, F, H, W, LRT_SEGMENT_MAX_FRAMES,
                LRT_SEGMENT_MAX_PIXELS);
    return LRT_OK;
}

static int check_inclination(const char* fn, const double* inclination, int n_inc, int H)
{
    if (n_inc != 2 && (n_inc != H || H < 3)) SG_FAIL(LRT_ERR_ARG, "%s: %d inclinations (2 bounds, or one per row of at least 3: %d)", fn, n_inc, H);
    if (!inclination) SG_FAIL(LRT_ERR_ARG, "%s: null inclination pointer", fn);
    return LRT_OK;
}

static int select_device(const char* fn, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) SG_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    return LRT_OK;
}

extern "C" {

int lrt_segment_abi_version(void) { return LRT_SEGMENT_ABI_VERSION; }

const char* lrt_segment_last_error(void) { return g_err; }

long long lrt_seg_work_bytes(long long F, int H, int W) { return work_bytes_of(F, H, W); }

int lrt_seg_ground(int device, long long F, int H, int W, const double* inclination, int n_inc, const float* points, const unsigned char* mask,
                   double up_x, double up_y, double up_z, double z_lo, double z_hi, double slope, unsigned char* ground, void* stream_)
{
    const char* fn = "lrt_seg_ground";
    int rc;
    if ((rc = check_sizes(fn, F, H, W)) != LRT_OK) return rc;
    if ((rc = check_inclination(fn, inclination, n_inc, H)) != LRT_OK) return rc;
    if (!points || !mask || !ground) SG_FAIL(LRT_ERR_ARG, "%s: null points / mask / ground pointer", fn);
    const double n2 = up_x * up_x + up_y * up_y + up_z * up_z;
    if (!(n2 > 1.0 - 1e-6 && n2 < 1.0 + 1e-6)) SG_FAIL(LRT_ERR_ARG, "%s: up (%g, %g, %g) is not a unit vector", fn, up_x, up_y, up_z);
    if (!(finite_d(z_lo) && finite_d(z_hi) && z_lo <= z_hi)) SG_FAIL(LRT_ERR_ARG, "%s: the height band [%g, %g] (z_lo <= z_hi)", fn, z_lo, z_hi);
    if (!(slope >= 0.0 && finite_d(slope))) SG_FAIL(LRT_ERR_ARG, "%s: slope %g (not negative)", fn, slope);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) SG_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    GroundArgs a;
    a.H = H; a.W = W; a.n_inc = n_inc; a.inc = inclination; a.points = points; a.mask = mask;
    a.up[0] = up_x; a.up[1] = up_y; a.up[2] = up_z; a.z_lo = z_lo; a.z_hi = z_hi; a.slope = slope; a.ground = ground;
    hipLaunchKernelGGL(k_seg_ground, dim3((unsigned)((W + 63) / 64), (unsigned)F), dim3(64), 0, (hipStream_t)stream_, a);
    SG_LAUNCHED("the column scan");
    return LRT_OK;
}

int lrt_seg_label(int device, long long F, int H, int W, const float* points, const unsigned char* mask, const unsigned char* exclude,
                  double d_abs, double c_h, double c_v, int* label, void* stream_)
{
    const char* fn = "lrt_seg_label";
    int rc;
    if ((rc = check_sizes(fn, F, H, W)) != LRT_OK) return rc;
    if (!points || !mask || !label) SG_FAIL(LRT_ERR_ARG, "%s: null points / mask / label pointer", fn);
    if (!(d_abs >= 0.0 && finite_d(d_abs) && c_h >= 0.0 && finite_d(c_h) && c_v >= 0.0 && finite_d(c_v)))
        SG_FAIL(LRT_ERR_ARG, "%s: thresholds d_abs %g, c_h %g, c_v %g (not negative)", fn, d_abs, c_h, c_v);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) SG_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    LabelArgs a;
    a.H = H; a.W = W; a.HW = H * W; a.points = points; a.mask = mask; a.exclude = exclude; a.label = label;
    const float da = (float)d_abs, ch = (float)c_h, cv = (float)c_v;
    a.dabs2 = da * da; a.ch2 = ch * ch; a.cv2 = cv * cv;
    const dim3 grid((unsigned)n_wg_of(a.HW), (unsigned)F);
    hipLaunchKernelGGL(k_seg_label_init, grid, dim3(NT), 0, stream, a);
    SG_LAUNCHED("the run labels");
    hipLaunchKernelGGL(k_seg_label_merge, grid, dim3(NT), 0, stream, a);
    SG_LAUNCHED("the merge");
    hipLaunchKernelGGL(k_seg_label_flatten, grid, dim3(NT), 0, stream, a);
    SG_LAUNCHED("the flatten pass");
    return LRT_OK;
}

int lrt_seg_freespace(int device, long long F, int H, int W, const double* inclination, int n_inc, double off, double yaw, double min_depth,
                      double max_depth, const float* src_points, const unsigned char* src_mask, const float* tgt_range, const unsigned char* tgt_mask,
                      const double* X, int rh, int rw, double m_abs, double m_rel, signed char* ev, void* stream_)
{
    const char* fn = "lrt_seg_freespace";
    int rc;
    if ((rc = check_sizes(fn, F, H, W)) != LRT_OK) return rc;
    if ((rc = check_inclination(fn, inclination, n_inc, H)) != LRT_OK) return rc;
    if (!(off >= 0.0 && off < 1.0)) SG_FAIL(LRT_ERR_ARG, "%s: pixel offset %g (0 for KITTI, 0.5 for Waymo)", fn, off);
    if (!finite_d(yaw)) SG_FAIL(LRT_ERR_ARG, "%s: yaw %g", fn, yaw);
    if (!(min_depth >= 0.0 && min_depth < max_depth && finite_d(max_depth))) SG_FAIL(LRT_ERR_ARG, "%s: depths (%g, %g] (0 <= min < max)", fn, min_depth, max_depth);
    if (!src_points || !src_mask) SG_FAIL(LRT_ERR_ARG, "%s: null src_points / src_mask pointer", fn);
    if (!tgt_range || !tgt_mask) SG_FAIL(LRT_ERR_ARG, "%s: null tgt_range / tgt_mask pointer", fn);
    if (!X || !ev) SG_FAIL(LRT_ERR_ARG, "%s: null X / ev pointer", fn);
    if (rh < 0 || rh > LRT_SEGMENT_MAX_RH || rw < 0 || rw > LRT_SEGMENT_MAX_RW)
        SG_FAIL(LRT_ERR_ARG, "%s: a window of %d rows and %d columns either side (at most %d and %d)", fn, rh, rw, LRT_SEGMENT_MAX_RH, LRT_SEGMENT_MAX_RW);
    if (!(m_abs >= 0.0 && finite_d(m_abs) && m_rel >= 0.0 && finite_d(m_rel))) SG_FAIL(LRT_ERR_ARG, "%s: margins m_abs %g, m_rel %g (not negative)", fn, m_abs, m_rel);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) SG_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    FreeArgs a;
    a.HW = H * W;
    a.rule.H = H; a.rule.W = W; a.rule.n_inc = n_inc; a.rule.wrap = 1;
    a.rule.off = off; a.rule.yaw = yaw; a.rule.min_depth = min_depth; a.rule.max_depth = max_depth;
    a.inc = inclination; a.sp = src_points; a.sm = src_mask; a.tr = tgt_range; a.tm = tgt_mask; a.X = X; a.rh = rh; a.rw = rw;
    a.m_abs = m_abs; a.m_rel = m_rel; a.ev = ev;
    hipLaunchKernelGGL(k_seg_freespace, dim3((unsigned)n_wg_of(a.HW), (unsigned)F), dim3(NT), 0, (hipStream_t)stream_, a);
    SG_LAUNCHED("the free-space test");
    return LRT_OK;
}

static unsigned fill_grid(long long n) { const long long g = (n + NT - 1) / NT; return (unsigned)(g < 1 ? 1 : g > 4096 ? 4096 : g); }

int lrt_seg_stats(int device, long long F, int H, int W, const float* points, const int* label, const signed char* ev0, const signed char* ev1,
                  int S_max, int* seg, int* n_seg, int* overflow, long long* table, void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_seg_stats";
    int rc;
    if ((rc = check_sizes(fn, F, H, W)) != LRT_OK) return rc;
    const long long need = work_bytes_of(F, H, W);
    if (S_max < 1 || S_max > LRT_SEGMENT_MAX_SEGMENTS || F > LRT_SEGMENT_MAX_PIXELS / S_max)
        SG_FAIL(LRT_ERR_ARG, "%s: a capacity of %d segments per frame (1 to %d, F S_max at most %lld)", fn, S_max, LRT_SEGMENT_MAX_SEGMENTS, LRT_SEGMENT_MAX_PIXELS);
    if (!points || !label) SG_FAIL(LRT_ERR_ARG, "%s: null points / label pointer", fn);
    if (!seg || !n_seg || !overflow || !table) SG_FAIL(LRT_ERR_ARG, "%s: null seg / n_seg / overflow / table pointer", fn);
    if (!workspace || ((uintptr_t)workspace & 255)) SG_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) SG_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld frames of %d x %d need %lld", fn, work_bytes, F, H, W, need);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) SG_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    StatArgs a;
    a.HW = H * W; a.nb = (int)n_wg_of(a.HW); a.S_max = S_max; a.points = points; a.label = label; a.ev0 = ev0; a.ev1 = ev1;
    a.wg = (unsigned*)workspace;
    a.first = (unsigned*)((char*)workspace + round256(4 * F * a.nb));
    a.seg = seg; a.n_seg = n_seg; a.overflow = overflow; a.table = table;
    const long long n = F * S_max * NC;
    const dim3 grid((unsigned)a.nb, (unsigned)F);
    hipLaunchKernelGGL(k_seg_fill, dim3(fill_grid(n)), dim3(NT), 0, stream, table, n);
    SG_LAUNCHED("the fill");
    hipLaunchKernelGGL(k_seg_count, grid, dim3(NT), 0, stream, a);
    SG_LAUNCHED("the count");
    hipLaunchKernelGGL(k_seg_scan, dim3((unsigned)F), dim3(NT), 0, stream, a);
    SG_LAUNCHED("the scan");
    hipLaunchKernelGGL(k_seg_number, grid, dim3(NT), 0, stream, a);
    SG_LAUNCHED("the numbering");
    hipLaunchKernelGGL(k_seg_accumulate, grid, dim3(NT), 0, stream, a);
    SG_LAUNCHED("the accumulation");
    return LRT_OK;
}

int lrt_seg_track_bounds(int device, long long F, int H, int W, const float* points, const int* seg, int S_max, const int* track_of, int NTR,
                         const double* pose, long long* bounds, long long* count, void* stream_)
{
    const char* fn = "lrt_seg_track_bounds";
    int rc;
    if ((rc = check_sizes(fn, F, H, W)) != LRT_OK) return rc;
    if (S_max < 1 || S_max > LRT_SEGMENT_MAX_SEGMENTS || F > LRT_SEGMENT_MAX_PIXELS / S_max)
        SG_FAIL(LRT_ERR_ARG, "%s: a capacity of %d segments per frame (1 to %d, F S_max at most %lld)", fn, S_max, LRT_SEGMENT_MAX_SEGMENTS, LRT_SEGMENT_MAX_PIXELS);
    if (NTR < 1 || NTR > LRT_SEGMENT_MAX_TRACKS) SG_FAIL(LRT_ERR_ARG, "%s: %d tracks (1 to %d)", fn, NTR, LRT_SEGMENT_MAX_TRACKS);
    if (!points || !seg || !track_of || !pose) SG_FAIL(LRT_ERR_ARG, "%s: null points / seg / track_of / pose pointer", fn);
    if (!bounds || !count) SG_FAIL(LRT_ERR_ARG, "%s: null bounds / count pointer", fn);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) SG_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    BoundArgs a;
    a.HW = H * W; a.S_max = S_max; a.NTR = NTR; a.F = F; a.points = points; a.seg = seg; a.track_of = track_of; a.pose = pose; a.bounds = bounds; a.count = count;
    hipLaunchKernelGGL(k_seg_bounds_fill, dim3((unsigned)((NTR + NT - 1) / NT)), dim3(NT), 0, stream, bounds, count, NTR);
    SG_LAUNCHED("the fill");
    hipLaunchKernelGGL(k_seg_bounds, dim3((unsigned)n_wg_of(a.HW), (unsigned)F), dim3(NT), 0, stream, a);
    SG_LAUNCHED("the bounds");
    return LRT_OK;
}

}  // extern "C"
