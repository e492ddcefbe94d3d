// lrt_densify.hip -- the fused densify-and-prune of one Gaussian asset (include/lrt_densify.h), gfx950.  Compiled into liblrt_densify.so, a library
// of its own.  No atomics, no allocation, no host wait; the per-row rule is lrt_densify_math.h.
//
//   k_densify_stats   one thread per row: accum += |mean_grad|, denom += (weight > 0).
//   k_densify_plan    a workgroup of 256 threads owns 256 consecutive rows, one per thread: the row's code (one byte: kind and the two prune marks) and
//                     the block's twelve counts -- the four output segments with the marks applied, the same four without, n_scale, n_opa, n_outside
//                     and the number of marked outputs -- summed over the wave in three 64-bit words of four 16-bit fields and over the four waves
//                     in LDS.
//   k_densify_scan    ONE workgroup of 1024 threads walks the block counts 1024 blocks per pass (a thread per block: wave scan by shuffles, the
//                     sixteen wave totals in LDS, the carry of the earlier passes added) and writes every block's exclusive offsets for both
//                     variants; then the decision whether the marks are applied (not when they would remove every output), the bases of the four
//                     segments and the totals.
//   k_densify_apply   the same blocking as the plan.  A block turns its 256 codes into destination rows (ballot ranks + its offsets + the segment
//                     base) in LDS, computes the children's positions of its split rows there, and then walks, group after group, the contiguous
//                     256 * width floats of its source rows with the lanes ALONG the row: element e of the block belongs to row e / width (a
//                     multiply-high by the group's reciprocal), is loaded once if one of the row's outputs survives and stored to slot 0's and slot 1's
//                     destination row at the same column.  Surviving rows that are consecutive in the source are consecutive in the destination, so
//                     a wave's stores are runs of whole rows.  A moment is loaded only for a surviving original; clones and children get zeros.
//                     Four elements per thread are in flight.  Every access is 4 bytes per lane (256 bytes per wave instruction) whatever the
//                     pointers' alignment.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_densify_math.h"
#include "../../include/lrt_densify.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_DENSIFY_BLOCK_ROWS;     // threads = rows per workgroup of stats, plan and apply
constexpr int SCAN_NT = LRT_DENSIFY_SCAN_BLOCKS;
constexpr int NC = 12;                         // counts per block
constexpr int NOFF = 8;                        // offsets per block: the four segments with the marks applied, then without
constexpr unsigned NONE = 0xFFFFFFFFu;
// head words of the workspace
constexpr int H_BASE = 0, H_APPLIED = 4;

static_assert(NT == 256 && SCAN_NT == 1024, "the kernels below are written for these");

struct Workspace {
    unsigned* head;                            // 64 words
    unsigned char* code;                       // P
    unsigned* cnt;                             // nblk * NC
    unsigned* off;                             // nblk * NOFF
};

static inline long long round256(long long x) { return (x + 255) / 256 * 256; }
static inline long long n_blocks(long long P) { return (P + NT - 1) / NT; }

static long long workspace_bytes(long long P)
{
    const long long nb = n_blocks(P);
    return 256 + round256(P) + round256(nb * NC * 4) + round256(nb * NOFF * 4);
}

static Workspace carve(void* ws, long long P)
{
    const long long nb = n_blocks(P);
    char* p = (char*)ws;
    Workspace w;
    w.head = (unsigned*)p; p += 256;
    w.code = (unsigned char*)p; p += round256(P);
    w.cnt = (unsigned*)p; p += round256(nb * NC * 4);
    w.off = (unsigned*)p;
    return w;
}

// ---- statistics -----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_densify_stats(long long P, const float* __restrict__ grads, const float* __restrict__ weights,
                                                      float* __restrict__ accum, float* __restrict__ denom)
{
    const long long i = (long long)blockIdx.x * NT + threadIdx.x;
    if (i >= P) return;
    accum[i] = lrt_densify_accumulate(accum[i], grads[3 * i], grads[3 * i + 1], grads[3 * i + 2]);
    if (weights[i] > 0.f) denom[i] += 1.f;
}

// ---- plan -------------------------------------------------------------------------------------------------------------------------------------------------
struct PlanArgs {
    long long P;
    int S;
    const float *xyz, *scaling, *rotation, *opacity, *accum, *denom, *split_noise, *box_noise;
    LrtDensifyRule rule;
    unsigned char* code;
    unsigned* cnt;
};

__global__ __launch_bounds__(NT) void k_densify_plan(PlanArgs a)
{
    __shared__ unsigned long long s_w[NT / 64][3];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * NT + tid;
    const bool exists = i < a.P;
    unsigned code = 0;
    if (exists) {
        float xyz[3], s[3] = {0.f, 0.f, 0.f}, q[4], sn[6], bn[12];
        for (int k = 0; k < 3; k++) xyz[k] = a.xyz[3 * i + k];
        for (int k = 0; k < a.S; k++) s[k] = a.scaling[(long long)a.S * i + k];
        for (int k = 0; k < 4; k++) q[k] = a.rotation[4 * i + k];
        for (int k = 0; k < 6; k++) sn[k] = a.split_noise[6 * i + k];
        const bool box = a.rule.size_limit && a.rule.has_box;
        for (int k = 0; k < 12; k++) bn[k] = box ? a.box_noise[12 * i + k] : 0.f;
        code = lrt_densify_row(xyz, s, a.S, q, a.opacity[i], a.accum[i], a.denom[i], sn, bn, a.rule);
        a.code[i] = (unsigned char)(code & 0xFFu);
    }
    const unsigned kind = code & LRT_DENSIFY_KIND_MASK;
    const unsigned p0 = (code & LRT_DENSIFY_PRUNE0) ? 1u : 0u, p1 = (code & LRT_DENSIFY_PRUNE1) ? 1u : 0u;
    const unsigned e0 = exists ? 1u : 0u;
    const unsigned orig = e0 & (kind != LRT_DENSIFY_SPLIT), cl = kind == LRT_DENSIFY_CLONE, sp = kind == LRT_DENSIFY_SPLIT;
#define B(m) ((code & (m)) ? 1ull : 0ull)
    unsigned long long w0 = (unsigned long long)(orig & (1u - p0)) | ((unsigned long long)(cl & (1u - p1)) << 16) | ((unsigned long long)(sp & (1u - p0)) << 32)
                            | ((unsigned long long)(sp & (1u - p1)) << 48);
    unsigned long long w1 = (unsigned long long)orig | ((unsigned long long)cl << 16) | ((unsigned long long)sp << 32) | ((unsigned long long)sp << 48);
    unsigned long long w2 = (B(LRT_DENSIFY_HUGE0) + B(LRT_DENSIFY_HUGE1)) | ((B(LRT_DENSIFY_LOW0) + B(LRT_DENSIFY_LOW1)) << 16)
                            | ((B(LRT_DENSIFY_OUT0) + B(LRT_DENSIFY_OUT1)) << 32) | ((unsigned long long)(p0 + p1) << 48);
#undef B
    for (int d = 32; d >= 1; d >>= 1) {        // every field stays below 2 * 256: no carry between the 16-bit fields
        w0 += __shfl_xor(w0, d); w1 += __shfl_xor(w1, d); w2 += __shfl_xor(w2, d);
    }
    if ((tid & 63) == 0) { s_w[tid >> 6][0] = w0; s_w[tid >> 6][1] = w1; s_w[tid >> 6][2] = w2; }
    __syncthreads();
    if (tid < NC) {
        const int word = tid >> 2, sh = 16 * (tid & 3);
        unsigned long long t = 0;
        for (int w = 0; w < NT / 64; w++) t += s_w[w][word];
        a.cnt[(long long)blockIdx.x * NC + tid] = (unsigned)((t >> sh) & 0xFFFFull);
    }
}

// ---- scan -------------------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(SCAN_NT) void k_densify_scan(long long nblk, const unsigned* __restrict__ cnt, unsigned* __restrict__ off,
                                                          unsigned* __restrict__ head, long long* __restrict__ totals)
{
    __shared__ unsigned s_w[SCAN_NT / 64][NC];
    __shared__ unsigned s_carry[NC];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < NC) s_carry[tid] = 0;
    __syncthreads();
    for (long long base = 0; base < nblk; base += SCAN_NT) {
        const long long b = base + tid;
        unsigned v[NC], inc[NC];
#pragma unroll
        for (int j = 0; j < NC; j++) {
            v[j] = b < nblk ? cnt[b * NC + j] : 0u;
            unsigned x = v[j];
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            inc[j] = x;
            if (lane == 63) s_w[wave][j] = x;
        }
        __syncthreads();
        if (b < nblk) {
#pragma unroll
            for (int j = 0; j < NOFF; j++) {
                unsigned pre = s_carry[j];
                for (int w = 0; w < wave; w++) pre += s_w[w][j];
                off[b * NOFF + j] = pre + inc[j] - v[j];
            }
        }
        __syncthreads();
        if (tid < NC) {
            unsigned t = s_carry[tid];
            for (int w = 0; w < SCAN_NT / 64; w++) t += s_w[w][tid];
            s_carry[tid] = t;
        }
        __syncthreads();
    }
    if (tid == 0) {
        const unsigned* c = s_carry;
        const unsigned long long n_out = (unsigned long long)c[4] + c[5] + c[6] + c[7];
        const unsigned applied = (unsigned long long)c[11] < n_out ? 1u : 0u;          // marks that would remove every output are not applied
        const unsigned* seg = applied ? c : c + 4;
        unsigned acc = 0;
        for (int k = 0; k < 4; k++) { head[H_BASE + k] = acc; acc += seg[k]; }
        head[H_APPLIED] = applied;
        totals[0] = (long long)acc; totals[1] = c[5]; totals[2] = c[6]; totals[3] = c[8]; totals[4] = c[9]; totals[5] = c[10]; totals[6] = applied; totals[7] = 0;
    }
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------------------------------
struct ApGroup {
    const float *src, *src_m, *src_v;
    float *dst, *dst_m, *dst_v;
    unsigned width, inv;                       // inv = floor(2^32 / width) + 1 (width > 1): e / width == umulhi(e, inv) for e * width < 2^32
    int role;
};

struct ApplyArgs {
    ApGroup grp[LRT_DENSIFY_MAX_GROUPS];
    long long P, P_new;
    int S, n_groups;
    const float *xyz, *scaling, *rotation, *split_noise;
    const unsigned char* code;
    const unsigned* off;
    const unsigned* head;
};

struct ApRows {                                // the block's rows in LDS
    unsigned d0[NT], d1[NT];                   // destination row of slot 0 / slot 1, NONE: no such output
    unsigned char kind[NT];
    float cx[6][NT];                           // a split row's children: [3 * child + component][row]
};

// One tensor of one group.  MOMENT: slot 0 of a surviving original is copied, every other output is zero.
template <bool MOMENT>
__device__ __forceinline__ void walk(const float* __restrict__ src, float* __restrict__ dst, int nel, unsigned w, unsigned inv, int role, const ApRows& R, int tid)
{
    constexpr int U = 4;
    for (int e0 = tid; e0 < nel; e0 += U * NT) {
        float v[U];
        unsigned r[U], c[U];
#pragma unroll
        for (int k = 0; k < U; k++) {
            const unsigned e = (unsigned)(e0 + k * NT);
            v[k] = 0.f; r[k] = NONE; c[k] = 0;
            if (e < (unsigned)nel) {
                const unsigned row = w == 1 ? e : __umulhi(e, inv);
                r[k] = row; c[k] = e - row * w;
                const bool need = MOMENT ? (R.d0[row] != NONE && R.kind[row] != LRT_DENSIFY_SPLIT) : (R.d0[row] != NONE || R.d1[row] != NONE);
                if (need) v[k] = src[e];
            }
        }
#pragma unroll
        for (int k = 0; k < U; k++) {
            if (r[k] == NONE) continue;
            const unsigned row = r[k], d0 = R.d0[row], d1 = R.d1[row];
            float v0 = v[k], v1 = v[k];
            if (R.kind[row] == LRT_DENSIFY_SPLIT) {
                if (MOMENT) v0 = 0.f;
                else if (role == LRT_DENSIFY_ROLE_XYZ) { v0 = R.cx[c[k]][row]; v1 = R.cx[3 + c[k]][row]; }
                else if (role == LRT_DENSIFY_ROLE_SCALING) v0 = v1 = lrt_densify_child_scaling(v[k]);
            }
            if (MOMENT) v1 = 0.f;
            if (d0 != NONE) dst[(size_t)d0 * w + c[k]] = v0;
            if (d1 != NONE) dst[(size_t)d1 * w + c[k]] = v1;
        }
    }
}

__global__ __launch_bounds__(NT) void k_densify_apply(ApplyArgs a)
{
    __shared__ ApRows R;
    __shared__ unsigned s_wt[NT / 64][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long row0 = (long long)blockIdx.x * NT;
    const long long i = row0 + tid;
    const bool exists = i < a.P;
    const unsigned code = exists ? a.code[i] : 0u;
    const unsigned kind = code & LRT_DENSIFY_KIND_MASK;
    const unsigned applied = a.head[H_APPLIED];
    const bool s0 = exists && !(applied && (code & LRT_DENSIFY_PRUNE0));
    const bool s1 = exists && kind != LRT_DENSIFY_KEEP && !(applied && (code & LRT_DENSIFY_PRUNE1));
    const bool f[4] = {s0 && kind != LRT_DENSIFY_SPLIT, s1 && kind == LRT_DENSIFY_CLONE, s0 && kind == LRT_DENSIFY_SPLIT, s1 && kind == LRT_DENSIFY_SPLIT};
    unsigned rank[4];
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long m = __ballot(f[k]);
        rank[k] = (unsigned)__popcll(m & below);
        if (lane == 0) s_wt[wave][k] = (unsigned)__popcll(m);
    }
    __syncthreads();
    const unsigned* off = a.off + (long long)blockIdx.x * NOFF + (applied ? 0 : 4);
    unsigned d[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
        unsigned pre = a.head[H_BASE + k] + off[k];
        for (int w = 0; w < wave; w++) pre += s_wt[w][k];
        d[k] = pre + rank[k];
        if (!f[k] || (long long)d[k] >= a.P_new) d[k] = NONE;             // no row at or beyond P_new is written, whatever the caller passed
    }
    R.d0[tid] = f[0] ? d[0] : d[2];
    R.d1[tid] = f[1] ? d[1] : d[3];
    R.kind[tid] = (unsigned char)kind;
    if (kind == LRT_DENSIFY_SPLIT && (f[2] || f[3])) {
        float xyz[3], s[3] = {0.f, 0.f, 0.f}, q[4], sn[6], cx[6];
        for (int k = 0; k < 3; k++) xyz[k] = a.xyz[3 * i + k];
        for (int k = 0; k < a.S; k++) s[k] = a.scaling[(long long)a.S * i + k];
        for (int k = 0; k < 4; k++) q[k] = a.rotation[4 * i + k];
        for (int k = 0; k < 6; k++) sn[k] = a.split_noise[6 * i + k];
        lrt_densify_children(xyz, s, a.S, q, sn, cx);
        for (int k = 0; k < 6; k++) R.cx[k][tid] = cx[k];
    }
    __syncthreads();
    const long long left = a.P - row0;
    const int rows = left < NT ? (int)left : NT;
#pragma unroll 1
    for (int gi = 0; gi < a.n_groups; gi++) {
        const ApGroup& G = a.grp[gi];
        const int nel = rows * (int)G.width;                              // at most 256 * LRT_DENSIFY_MAX_WIDTH = 2^18
        const size_t base = (size_t)row0 * G.width;
        walk<false>(G.src + base, G.dst, nel, G.width, G.inv, G.role, R, tid);
        if (G.src_m) {
            walk<true>(G.src_m + base, G.dst_m, nel, G.width, G.inv, G.role, R, tid);
            walk<true>(G.src_v + base, G.dst_v, nel, G.width, G.inv, G.role, R, tid);
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define DN_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static int check_device(const char* fn, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) DN_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    return LRT_OK;
}

extern "C" {

int lrt_densify_abi_version(void) { return LRT_DENSIFY_ABI_VERSION; }

const char* lrt_densify_last_error(void) { return g_err; }

long long lrt_densify_workspace_bytes(long long P)
{
    if (P < 0 || P > LRT_DENSIFY_MAX_ROWS) return -1;
    return workspace_bytes(P);
}

int lrt_densify_stats(int device, long long P, const float* mean_grads, const float* weights, float* accum, float* denom, void* stream_)
{
    const char* fn = "lrt_densify_stats";
    if (P < 0 || P > LRT_DENSIFY_MAX_ROWS) DN_FAIL(LRT_ERR_ARG, "%s: %lld rows (0 .. %lld)", fn, P, LRT_DENSIFY_MAX_ROWS);
    if (P > 0 && (!mean_grads || !weights || !accum || !denom)) DN_FAIL(LRT_ERR_ARG, "%s: null mean_grads / weights / accum / denom pointer", fn);
    if (check_device(fn, device) != LRT_OK) return LRT_ERR_ARG;
    if (P == 0) return LRT_OK;
    LrtDeviceGuard guard(device);
    if (!guard.ok) DN_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipLaunchKernelGGL(k_densify_stats, dim3((unsigned)n_blocks(P)), dim3(NT), 0, (hipStream_t)stream_, P, mean_grads, weights, accum, denom);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) DN_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_densify_plan(int device, long long P, int S, const float* xyz, const float* scaling, const float* rotation, const float* opacity,
                     const float* accum, const float* denom, const float* split_noise, const float* box_noise, const lrt_densify_rule* rule,
                     void* workspace, long long ws_bytes, long long* totals, void* stream_)
{
    const char* fn = "lrt_densify_plan";
    if (P < 0 || P > LRT_DENSIFY_MAX_ROWS) DN_FAIL(LRT_ERR_ARG, "%s: %lld rows (0 .. %lld)", fn, P, LRT_DENSIFY_MAX_ROWS);
    if (S != 2 && S != 3) DN_FAIL(LRT_ERR_ARG, "%s: %d floats per scaling row (2 or 3)", fn, S);
    if (!rule) DN_FAIL(LRT_ERR_ARG, "%s: null rule", fn);
    if (!totals) DN_FAIL(LRT_ERR_ARG, "%s: null totals pointer", fn);
    if (rule->grad_thr != rule->grad_thr || rule->big_thr != rule->big_thr || rule->huge_thr != rule->huge_thr || rule->opa_thr != rule->opa_thr)
        DN_FAIL(LRT_ERR_ARG, "%s: a threshold is NaN (grad %g, big %g, huge %g, opacity %g)", fn, rule->grad_thr, rule->big_thr, rule->huge_thr, rule->opa_thr);
    const bool box = rule->size_limit && rule->has_box;
    if (box) for (int k = 0; k < 3; k++) if (!(rule->box_min[k] <= rule->box_max[k])) DN_FAIL(LRT_ERR_ARG, "%s: box_min[%d] = %g, box_max[%d] = %g", fn, k, rule->box_min[k], k, rule->box_max[k]);
    if (P > 0) {
        if (!xyz || !scaling || !rotation || !opacity || !accum || !denom || !split_noise) DN_FAIL(LRT_ERR_ARG, "%s: null xyz / scaling / rotation / opacity / accum / denom / split_noise pointer", fn);
        if (box && !box_noise) DN_FAIL(LRT_ERR_ARG, "%s: a box without box_noise", fn);
        if (!workspace || ((uintptr_t)workspace & 255)) DN_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
        if (ws_bytes < workspace_bytes(P)) DN_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld rows need %lld", fn, ws_bytes, P, workspace_bytes(P));
    }
    if (check_device(fn, device) != LRT_OK) return LRT_ERR_ARG;
    LrtDeviceGuard guard(device);
    if (!guard.ok) DN_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    if (P == 0) {
        if (hipMemsetAsync(totals, 0, LRT_DENSIFY_N_TOTALS * sizeof(long long), stream) != hipSuccess) DN_FAIL(LRT_ERR_HIP, "%s: cannot clear the totals", fn);
        return LRT_OK;
    }
    const Workspace w = carve(workspace, P);
    PlanArgs a;
    a.P = P; a.S = S; a.xyz = xyz; a.scaling = scaling; a.rotation = rotation; a.opacity = opacity; a.accum = accum; a.denom = denom;
    a.split_noise = split_noise; a.box_noise = box_noise;
    a.rule.grad_thr = rule->grad_thr; a.rule.big_thr = rule->big_thr; a.rule.huge_thr = rule->huge_thr; a.rule.opa_thr = rule->opa_thr;
    a.rule.size_limit = rule->size_limit != 0; a.rule.has_box = rule->has_box != 0;
    for (int k = 0; k < 3; k++) { a.rule.box_min[k] = rule->box_min[k]; a.rule.box_max[k] = rule->box_max[k]; }
    a.code = w.code; a.cnt = w.cnt;
    const long long nb = n_blocks(P);
    hipLaunchKernelGGL(k_densify_plan, dim3((unsigned)nb), dim3(NT), 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) DN_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(k_densify_scan, dim3(1), dim3(SCAN_NT), 0, stream, nb, (const unsigned*)w.cnt, w.off, w.head, totals);
    e = hipGetLastError();
    if (e != hipSuccess) DN_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_densify_apply(int device, long long P, long long P_new, int S, const float* rotation, const float* split_noise, int n_groups,
                      const lrt_densify_group* groups, const void* workspace, long long ws_bytes, void* stream_)
{
    const char* fn = "lrt_densify_apply";
    if (P < 0 || P > LRT_DENSIFY_MAX_ROWS) DN_FAIL(LRT_ERR_ARG, "%s: %lld rows (0 .. %lld)", fn, P, LRT_DENSIFY_MAX_ROWS);
    if (P_new < 0 || P_new > 2 * P) DN_FAIL(LRT_ERR_ARG, "%s: %lld rows out of %lld (0 .. %lld)", fn, P_new, P, 2 * P);
    if (S != 2 && S != 3) DN_FAIL(LRT_ERR_ARG, "%s: %d floats per scaling row (2 or 3)", fn, S);
    if (n_groups < 1 || n_groups > LRT_DENSIFY_MAX_GROUPS) DN_FAIL(LRT_ERR_ARG, "%s: %d groups (1 .. %d in one call)", fn, n_groups, LRT_DENSIFY_MAX_GROUPS);
    if (!groups) DN_FAIL(LRT_ERR_ARG, "%s: null group table", fn);
    ApplyArgs a;
    int i_xyz = -1, i_scaling = -1;
    for (int i = 0; i < n_groups; i++) {
        const lrt_densify_group& s = groups[i];
        if (s.width < 1 || s.width > LRT_DENSIFY_MAX_WIDTH) DN_FAIL(LRT_ERR_ARG, "%s: group %d: width %d (1 .. %d floats per row)", fn, i, s.width, LRT_DENSIFY_MAX_WIDTH);
        if (P > 0 && !s.src) DN_FAIL(LRT_ERR_ARG, "%s: group %d: null source pointer", fn, i);
        if (P_new > 0 && !s.dst) DN_FAIL(LRT_ERR_ARG, "%s: group %d: null destination pointer", fn, i);
        if ((s.src_exp_avg != nullptr) != (s.src_exp_avg_sq != nullptr)) DN_FAIL(LRT_ERR_ARG, "%s: group %d: one moment without the other", fn, i);
        if (s.src_exp_avg && P_new > 0 && (!s.dst_exp_avg || !s.dst_exp_avg_sq)) DN_FAIL(LRT_ERR_ARG, "%s: group %d: source moments without destination moments", fn, i);
        if (s.role == LRT_DENSIFY_ROLE_XYZ) {
            if (i_xyz >= 0 || s.width != 3) DN_FAIL(LRT_ERR_ARG, "%s: group %d: the role xyz belongs to one group of width 3", fn, i);
            i_xyz = i;
        } else if (s.role == LRT_DENSIFY_ROLE_SCALING) {
            if (i_scaling >= 0 || s.width != S) DN_FAIL(LRT_ERR_ARG, "%s: group %d: the role scaling belongs to one group of width %d", fn, i, S);
            i_scaling = i;
        } else if (s.role != LRT_DENSIFY_ROLE_COPY) DN_FAIL(LRT_ERR_ARG, "%s: group %d: role %d", fn, i, s.role);
        ApGroup& d = a.grp[i];
        d.src = s.src; d.src_m = s.src_exp_avg; d.src_v = s.src_exp_avg_sq; d.dst = s.dst; d.dst_m = s.dst_exp_avg; d.dst_v = s.dst_exp_avg_sq;
        d.width = (unsigned)s.width; d.inv = s.width > 1 ? (unsigned)((1ull << 32) / (unsigned)s.width) + 1u : 0u; d.role = s.role;
    }
    if (i_xyz < 0 || i_scaling < 0) DN_FAIL(LRT_ERR_ARG, "%s: the table needs a group with the role xyz and one with the role scaling", fn);
    for (int i = n_groups; i < LRT_DENSIFY_MAX_GROUPS; i++) { ApGroup& d = a.grp[i]; d.src = d.src_m = d.src_v = nullptr; d.dst = d.dst_m = d.dst_v = nullptr; d.width = 1; d.inv = 0; d.role = 0; }
    if (P > 0) {
        if (!rotation || !split_noise) DN_FAIL(LRT_ERR_ARG, "%s: null rotation / split_noise pointer", fn);
        if (!workspace || ((uintptr_t)workspace & 255)) DN_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
        if (ws_bytes < workspace_bytes(P)) DN_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, %lld rows need %lld", fn, ws_bytes, P, workspace_bytes(P));
    }
    if (check_device(fn, device) != LRT_OK) return LRT_ERR_ARG;
    if (P == 0 || P_new == 0) return LRT_OK;
    LrtDeviceGuard guard(device);
    if (!guard.ok) DN_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    const Workspace w = carve(const_cast<void*>(workspace), P);
    a.P = P; a.P_new = P_new; a.S = S; a.n_groups = n_groups;
    a.xyz = groups[i_xyz].src; a.scaling = groups[i_scaling].src; a.rotation = rotation; a.split_noise = split_noise;
    a.code = w.code; a.off = w.off; a.head = w.head;
    hipLaunchKernelGGL(k_densify_apply, dim3((unsigned)n_blocks(P)), dim3(NT), 0, (hipStream_t)stream_, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) DN_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
