// lrt_init.hip -- scene initialisation from range images (include/lrt_init.h), gfx950.  Compiled into liblrt_init.so, a library of its own.
//
// lrt_init_normals, three launches:
//   k_in_points  one workgroup per 8 x 32 tile of the image: the tile's points (lrt_gridcd_math.h: gc_point) as float4 (x, y, z, linear pixel
//                index) in tile-major order and the AABB over its valid points.  A pixel that is masked out or outside the image is a padding
//                point at GC_EMPTY; a tile without valid points gets an inverted box.  (k_gc_points of lrt_gridcd.hip for ONE cloud.)
//   k_in_knn     one workgroup per tile, one WAVEFRONT per 64 queries.  Each lane keeps its IN_KMAX best (distance bits << 32 | pixel index)
//                keys in ascending order in registers; the 8th is its pruning radius whatever k is (a looser radius only adds candidates a
//                brute-force scan would also see, and the first k of the best 8 are the best k).  The wave scans the tile it lies in, then
//                every other tile whose bound (gc_bound on the tile's box) is <= the radius of ANY of its lanes, pre-screened 64 tiles at a
//                time against the wave's query box (gc_bound_box): the structure of k_gc_search.  The visit is wave-uniform, so candidates
//                come through uniform (scalar) loads.  Every candidate is seen at most once, keys are distinct (the index is part of them), so
//                the list does not depend on the visiting order and ties go to the lower pixel index.
//   k_in_normal  one thread per pixel: the listed points again from (o, d, range), covariance and eigenvector in float64
//                (lrt_init_math.h), one rounding, the sign rule.
// lrt_init_assign: k_in_assign, one thread per pixel, the pose table through uniform loads.
// lrt_init_voxel_keys: k_in_vx_min (per-block minima, grid-stride), k_in_vx_origin (their minimum -> the float64 origin; clears the status),
//   k_in_vx_keys.  lrt_init_voxel_mean: k_in_vx_heads (segment heads of the sorted keys), k_in_scan_blk / k_in_scan_top (exclusive scan; the
//   total is M), k_in_vx_starts (first sorted position of each voxel), k_in_vx_mean (one thread per output row: its voxel's members in sorted
//   = ascending input order, float64 sums, one rounding; zeros from row M on).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_init_math.h"
#include "../../include/lrt_init.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int TH = 8, TW = 32, TP = TH * TW, NT = 256, NW = NT / 64;
constexpr int IN_NOIDX = 0x7fffffff;
constexpr int SCAN_ITEMS = 4, SCAN_BLK = NT * SCAN_ITEMS;
constexpr int MIN_BLOCKS = 512;
constexpr int KEY_BITS = 21;

struct InFrame {
    int H, W, ntx, nT;
    const float* o; const float* d; const float* r; const uint8_t* m;
};

__device__ __forceinline__ void in_pixel_point(const InFrame& a, size_t p, float& x, float& y, float& z)
{
    const float r = a.r[p];
    x = gc_point(a.o[3 * p], a.d[3 * p], r); y = gc_point(a.o[3 * p + 1], a.d[3 * p + 1], r); z = gc_point(a.o[3 * p + 2], a.d[3 * p + 2], r);
}

// ---- normals -----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_in_points(InFrame a, float4* __restrict__ pts, float* __restrict__ boxes)
{
    __shared__ float s_lo[3][NW], s_hi[3][NW];
    const int tile = blockIdx.x, tid = threadIdx.x, ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const int y = ty * TH + tid / TW, x = tx * TW + (tid & (TW - 1));
    const bool in = y < a.H && x < a.W;
    const size_t p = in ? (size_t)y * a.W + x : 0;
    const bool v = in && a.m[p] != 0;
    float4 q = make_float4(GC_EMPTY, GC_EMPTY, GC_EMPTY, __int_as_float(IN_NOIDX));
    float lo[3] = {GC_EMPTY, GC_EMPTY, GC_EMPTY}, hi[3] = {-GC_EMPTY, -GC_EMPTY, -GC_EMPTY};
    if (v) {
        in_pixel_point(a, p, q.x, q.y, q.z);
        q.w = __int_as_float((int)p);
        lo[0] = hi[0] = q.x; lo[1] = hi[1] = q.y; lo[2] = hi[2] = q.z;
    }
    pts[(size_t)tile * TP + tid] = q;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo[i] = fminf(lo[i], __shfl_xor(lo[i], o, 64)); hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], o, 64)); }
        if ((tid & 63) == 0) { s_lo[i][tid >> 6] = lo[i]; s_hi[i][tid >> 6] = hi[i]; }
    }
    __syncthreads();
    if (tid < 3) {
        float l = s_lo[tid][0], h = s_hi[tid][0];
#pragma unroll
        for (int w = 1; w < NW; w++) { l = fminf(l, s_lo[tid][w]); h = fmaxf(h, s_hi[tid][w]); }
        float* b = boxes + (size_t)tile * 8;
        b[tid] = l; b[4 + tid] = h;                             // an empty tile keeps lo = +GC_EMPTY, hi = -GC_EMPTY: the inverted box
        if (tid == 0) { b[3] = 0.f; b[7] = 0.f; }
    }
}

__device__ __forceinline__ float in_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

typedef unsigned long long u64;

__device__ __forceinline__ void in_scan_tile(const float4* __restrict__ pp, float qx, float qy, float qz, u64 (&bk)[IN_KMAX])
{
#pragma unroll 4
    for (int e = 0; e < TP; e++) {
        const float4 v = pp[e];                                // uniform address: scalar load
        const float d = gc_d2(gc_sub(v.x, qx), gc_sub(v.y, qy), gc_sub(v.z, qz));
        const u64 key = ((u64)__float_as_uint(d) << 32) | (unsigned)__float_as_int(v.w);   // d >= +0: bit order = value order
        if (key < bk[IN_KMAX - 1]) {                           // a padding point's distance is +inf: above the initial keys
            bk[IN_KMAX - 1] = key;
#pragma unroll
            for (int i = IN_KMAX - 1; i > 0; i--) {
                const u64 hi = bk[i], lo = bk[i - 1];
                const bool sw = hi < lo;
                bk[i] = sw ? lo : hi; bk[i - 1] = sw ? hi : lo;
            }
        }
    }
}

__global__ __launch_bounds__(NT) void k_in_knn(int H, int W, int ntx, int nT, int k, const float4* __restrict__ pts, const float* __restrict__ boxes,
                                               int* __restrict__ nbr)
{
    const int tile = blockIdx.x, tid = threadIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y = ty * TH + tid / TW, x = tx * TW + (tid & (TW - 1));
    const bool in = y < H && x < W;
    const float4 q = pts[(size_t)tile * TP + tid];
    const bool valid = __float_as_int(q.w) != IN_NOIDX;
    u64 bk[IN_KMAX];
#pragma unroll
    for (int i = 0; i < IN_KMAX; i++) bk[i] = ((u64)__float_as_uint(GC_BIG) << 32) | (unsigned)IN_NOIDX;
    if (__ballot(valid) != 0) {                                // wave-uniform from here on
        const int lane = tid & 63;
        float ql[3] = {valid ? q.x : GC_EMPTY, valid ? q.y : GC_EMPTY, valid ? q.z : GC_EMPTY};
        float qh[3] = {valid ? q.x : -GC_EMPTY, valid ? q.y : -GC_EMPTY, valid ? q.z : -GC_EMPTY};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { ql[i] = fminf(ql[i], __shfl_xor(ql[i], o, 64)); qh[i] = fmaxf(qh[i], __shfl_xor(qh[i], o, 64)); }
        in_scan_tile(pts + (size_t)tile * TP, q.x, q.y, q.z, bk);
        float wmax = in_wave_max(valid ? __uint_as_float((unsigned)(bk[IN_KMAX - 1] >> 32)) : 0.f);
        for (int c0 = 0; c0 < nT; c0 += 64) {
            const int tl = c0 + lane;
            float bb = __uint_as_float(0x7f800000u);
            if (tl < nT && tl != tile) {
                const float4 blo = *reinterpret_cast<const float4*>(boxes + (size_t)tl * 8), bhi = *reinterpret_cast<const float4*>(boxes + (size_t)tl * 8 + 4);
                bb = gc_bound_box(blo.x, blo.y, blo.z, bhi.x, bhi.y, bhi.z, ql[0], ql[1], ql[2], qh[0], qh[1], qh[2]);
            }
            u64 m = __ballot(bb <= wmax);                      // wmax only falls while the chunk is worked off: a stale value visits more, never less
            while (m != 0) {
                const int t = __builtin_amdgcn_readfirstlane(c0 + (int)__ffsll((long long)m) - 1);
                m &= m - 1;
                const float* __restrict__ b = boxes + (size_t)t * 8;
                const float lb = gc_bound(b[0], b[1], b[2], b[4], b[5], b[6], q.x, q.y, q.z);
                // <=, not <: a tile at exactly the radius may hold a tie with a lower pixel index
                if (__ballot(valid && lb <= __uint_as_float((unsigned)(bk[IN_KMAX - 1] >> 32))) == 0) continue;
                in_scan_tile(pts + (size_t)t * TP, q.x, q.y, q.z, bk);
                wmax = in_wave_max(valid ? __uint_as_float((unsigned)(bk[IN_KMAX - 1] >> 32)) : 0.f);
            }
        }
    }
    if (in) {
        int* out = nbr + ((size_t)y * W + x) * IN_KMAX;
        int v[IN_KMAX];
#pragma unroll
        for (int i = 0; i < IN_KMAX; i++) {
            const int idx = (int)(unsigned)bk[i];
            v[i] = (valid && i < k && idx != IN_NOIDX) ? idx : -1;
        }
        *reinterpret_cast<int4*>(out) = make_int4(v[0], v[1], v[2], v[3]);
        *reinterpret_cast<int4*>(out + 4) = make_int4(v[4], v[5], v[6], v[7]);
    }
}

__global__ __launch_bounds__(NT) void k_in_normal(InFrame a, const int* __restrict__ nbr, float* __restrict__ normal)
{
    const int HW = a.H * a.W, p = blockIdx.x * NT + threadIdx.x;
    if (p >= HW) return;
    float n[3] = {0.f, 0.f, 0.f};
    if (a.m[p] != 0) {
        const int4 l0 = *reinterpret_cast<const int4*>(nbr + (size_t)p * IN_KMAX), l1 = *reinterpret_cast<const int4*>(nbr + (size_t)p * IN_KMAX + 4);
        const int idx[IN_KMAX] = {l0.x, l0.y, l0.z, l0.w, l1.x, l1.y, l1.z, l1.w};
        float pt[3 * IN_KMAX];
        int cnt = 0;
#pragma unroll
        for (int i = 0; i < IN_KMAX; i++) {
            pt[3 * i] = 0.f; pt[3 * i + 1] = 0.f; pt[3 * i + 2] = 0.f;
            if ((unsigned)idx[i] < (unsigned)HW && cnt == i) {  // the list is a prefix; anything else ends it
                in_pixel_point(a, (size_t)idx[i], pt[3 * i], pt[3 * i + 1], pt[3 * i + 2]);
                cnt = i + 1;
            }
        }
        double nd[3] = {0.0, 0.0, 1.0};
        if (cnt >= 3) {
            double c[6];
            in_covariance(pt, cnt, c);
            in_smallest_eigenvector(c, nd, nullptr);
        }
        n[0] = (float)nd[0]; n[1] = (float)nd[1]; n[2] = (float)nd[2];
        float self[3];
        in_pixel_point(a, (size_t)p, self[0], self[1], self[2]);
        const float o[3] = {a.o[3 * (size_t)p], a.o[3 * (size_t)p + 1], a.o[3 * (size_t)p + 2]};
        in_face_sensor(n, o, self);
    }
    normal[3 * (size_t)p] = n[0]; normal[3 * (size_t)p + 1] = n[1]; normal[3 * (size_t)p + 2] = n[2];
}

// ---- assignment ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_in_assign(int n, const float* __restrict__ point, const float* __restrict__ normal, const uint8_t* __restrict__ mask,
                                                  int A, const float* __restrict__ pose, const float* __restrict__ size, const uint8_t* __restrict__ present,
                                                  int* __restrict__ label, float* __restrict__ lp, float* __restrict__ ln)
{
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= n) return;
    const size_t b = 3 * (size_t)p;
    float px = point[b], py = point[b + 1], pz = point[b + 2], nx = normal[b], ny = normal[b + 1], nz = normal[b + 2];
    int lab = -1;
    if (mask[p] != 0) {
        lab = 0;
        for (int a = 0; a < A; a++) {                            // uniform: the pose table comes through scalar loads
            if (present[a] == 0) continue;
            const float* ps = pose + 7 * (size_t)a;
            float w = ps[3], x = ps[4], y = ps[5], z = ps[6];
            const float inv = 1.f / sqrtf(w * w + x * x + y * y + z * z);
            w *= inv; x *= inv; y *= inv; z *= inv;
            const float r00 = 1.f - 2.f * (y * y + z * z), r01 = 2.f * (x * y - w * z), r02 = 2.f * (x * z + w * y);
            const float r10 = 2.f * (x * y + w * z), r11 = 1.f - 2.f * (x * x + z * z), r12 = 2.f * (y * z - w * x);
            const float r20 = 2.f * (x * z - w * y), r21 = 2.f * (y * z + w * x), r22 = 1.f - 2.f * (x * x + y * y);
            const float dx = px - ps[0], dy = py - ps[1], dz = pz - ps[2];
            const float lx = r00 * dx + r10 * dy + r20 * dz, ly = r01 * dx + r11 * dy + r21 * dz, lz = r02 * dx + r12 * dy + r22 * dz;
            if (fabsf(lx) < 0.5f * size[3 * a] && fabsf(ly) < 0.5f * size[3 * a + 1] && fabsf(lz) < 0.5f * size[3 * a + 2]) {
                lab = a + 1;
                const float mx = r00 * nx + r10 * ny + r20 * nz, my = r01 * nx + r11 * ny + r21 * nz, mz = r02 * nx + r12 * ny + r22 * nz;
                px = lx; py = ly; pz = lz; nx = mx; ny = my; nz = mz;
                break;
            }
        }
    }
    label[p] = lab;
    lp[b] = px; lp[b + 1] = py; lp[b + 2] = pz;
    ln[b] = nx; ln[b + 1] = ny; ln[b + 2] = nz;
}

// ---- voxel mean ----------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_in_vx_min(int N, const float* __restrict__ pts, float* __restrict__ partial)
{
    __shared__ float s[3][NW];
    const float inf = __uint_as_float(0x7f800000u);
    float m[3] = {inf, inf, inf};
    for (int i = blockIdx.x * NT + threadIdx.x; i < N; i += gridDim.x * NT) {
        m[0] = fminf(m[0], pts[3 * (size_t)i]); m[1] = fminf(m[1], pts[3 * (size_t)i + 1]); m[2] = fminf(m[2], pts[3 * (size_t)i + 2]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m[c] = fminf(m[c], __shfl_xor(m[c], o, 64));
        if ((threadIdx.x & 63) == 0) s[c][threadIdx.x >> 6] = m[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = s[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < NW; w++) v = fminf(v, s[threadIdx.x][w]);
        partial[4 * blockIdx.x + threadIdx.x] = v;
    }
}

__global__ __launch_bounds__(NT) void k_in_vx_origin(int nblk, double voxel, const float* __restrict__ partial, double* __restrict__ origin, int* __restrict__ info)
{
    __shared__ float s[3][NW];
    const float inf = __uint_as_float(0x7f800000u);
    float m[3] = {inf, inf, inf};
    for (int i = threadIdx.x; i < nblk; i += NT) { m[0] = fminf(m[0], partial[4 * i]); m[1] = fminf(m[1], partial[4 * i + 1]); m[2] = fminf(m[2], partial[4 * i + 2]); }
#pragma unroll
    for (int c = 0; c < 3; c++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m[c] = fminf(m[c], __shfl_xor(m[c], o, 64));
        if ((threadIdx.x & 63) == 0) s[c][threadIdx.x >> 6] = m[c];
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        float v = s[threadIdx.x][0];
#pragma unroll
        for (int w = 1; w < NW; w++) v = fminf(v, s[threadIdx.x][w]);
        origin[threadIdx.x] = (double)v - 0.5 * voxel;
    }
    if (threadIdx.x == 3) info[1] = 0;
}

__global__ __launch_bounds__(NT) void k_in_vx_keys(int N, double voxel, const float* __restrict__ pts, const double* __restrict__ origin,
                                                   long long* __restrict__ keys, int* __restrict__ info)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    long long key = 0;
    bool bad = false;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double f = floor(((double)pts[3 * (size_t)i + c] - origin[c]) / voxel);
        const bool ok = f >= 0.0 && f < (double)(1 << KEY_BITS);  // false for NaN too
        bad = bad || !ok;
        key = (key << KEY_BITS) | (ok ? (long long)f : 0LL);
    }
    keys[i] = key;
    if (bad) atomicOr(&info[1], LRT_INIT_KEY_RANGE);            // an integer flag: the same bits whatever the arrival order
}

__global__ __launch_bounds__(NT) void k_in_vx_heads(int N, const long long* __restrict__ keys, int* __restrict__ flag)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i < N) flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1 : 0;
}

__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int& total)       // NT threads; s_w: NW ints of LDS
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    __syncthreads();
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    int base = 0; total = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) { if (w < wv) base += s_w[w]; total += s_w[w]; }
    return base + inc - v;
}

__global__ __launch_bounds__(NT) void k_in_scan_blk(int n, const int* __restrict__ cnt, int* __restrict__ off, int* __restrict__ blksum)
{
    __shared__ int s_w[NW];
    const int base = blockIdx.x * SCAN_BLK + threadIdx.x * SCAN_ITEMS;
    int v[SCAN_ITEMS], s = 0;
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { v[k] = base + k < n ? cnt[base + k] : 0; s += v[k]; }
    int total;
    int ex = block_excl_scan(s, s_w, total);
#pragma unroll
    for (int k = 0; k < SCAN_ITEMS; k++) { if (base + k < n) off[base + k] = ex; ex += v[k]; }
    if (threadIdx.x == 0) blksum[blockIdx.x] = total;
}

__global__ __launch_bounds__(NT) void k_in_scan_top(int nblk, const int* __restrict__ blksum, int* __restrict__ blkoff, int* __restrict__ info)
{
    __shared__ int s_w[NW];
    int carry = 0;
    for (int c0 = 0; c0 < nblk; c0 += NT) {
        const int i = c0 + threadIdx.x;
        const int v = i < nblk ? blksum[i] : 0;
        int total;
        const int ex = block_excl_scan(v, s_w, total);
        if (i < nblk) blkoff[i] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) info[0] = carry;                      // M: the number of occupied voxels
}

__global__ __launch_bounds__(NT) void k_in_vx_starts(int N, const int* __restrict__ flag, const int* __restrict__ off, const int* __restrict__ blkoff,
                                                     int* __restrict__ start)
{
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= N) return;
    const int seg = off[i] + blkoff[i / SCAN_BLK];               // exclusive: the row of a head, row + 1 of the others
    if (flag[i]) start[seg] = i;
    if (i == N - 1) start[seg + flag[i]] = N;                    // start[M]: seg + flag <= N, and start holds N + 1 entries
}

__global__ __launch_bounds__(NT) void k_in_vx_mean(int N, const int* __restrict__ start, const int* __restrict__ perm, const float* __restrict__ pts,
                                                   const float* __restrict__ inten, const float* __restrict__ nrm, const int* __restrict__ info,
                                                   float* __restrict__ o_pts, float* __restrict__ o_int, float* __restrict__ o_nrm, int* __restrict__ count)
{
    const int s = blockIdx.x * NT + threadIdx.x;
    if (s >= N) return;
    double a[7] = {0, 0, 0, 0, 0, 0, 0};
    int c = 0;
    if (s < info[0]) {
        const int j0 = start[s], j1 = start[s + 1];
        for (int j = j0; j < j1; j++) {                          // sorted position = ascending input index inside a voxel (the sort is stable)
            const int src = perm[j];
            if ((unsigned)src >= (unsigned)N) continue;          // not a permutation of this cloud: skipped, never read
            const size_t b = 3 * (size_t)src;
            a[0] += (double)pts[b]; a[1] += (double)pts[b + 1]; a[2] += (double)pts[b + 2];
            a[3] += (double)inten[src];
            a[4] += (double)nrm[b]; a[5] += (double)nrm[b + 1]; a[6] += (double)nrm[b + 2];
            c++;
        }
        const double inv = c > 0 ? 1.0 / (double)c : 0.0;
#pragma unroll
        for (int i = 0; i < 7; i++) a[i] *= inv;
    }
    const size_t b = 3 * (size_t)s;
    o_pts[b] = (float)a[0]; o_pts[b + 1] = (float)a[1]; o_pts[b + 2] = (float)a[2];
    o_int[s] = (float)a[3];
    o_nrm[b] = (float)a[4]; o_nrm[b + 1] = (float)a[5]; o_nrm[b + 2] = (float)a[6];
    count[s] = c;
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define IN_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline bool size_ok(int H, int W) { return H > 0 && W > 0 && W <= (1 << 20) && (size_t)H * W <= ((size_t)1 << 27); }
static inline bool count_ok(long long N) { return N > 0 && N <= (1LL << 27); }
static inline size_t up16(size_t n) { return (n + 15) / 16 * 16; }

struct NLayout { int ntx, nT; size_t pts, boxes, total; };

static NLayout nlayout(int H, int W)
{
    NLayout L;
    L.ntx = (W + TW - 1) / TW; L.nT = L.ntx * ((H + TH - 1) / TH);
    size_t o = 0;
    L.pts = o; o += (size_t)L.nT * TP * sizeof(float4);
    L.boxes = o; o += up16((size_t)L.nT * 8 * sizeof(float));
    L.total = o;
    return L;
}

struct VLayout { int nblk, nmin; size_t partial, origin, flag, off, blksum, blkoff, start, total; };

static VLayout vlayout(long long N)
{
    VLayout L;
    L.nblk = (int)((N + SCAN_BLK - 1) / SCAN_BLK);
    const long long want = (N + NT - 1) / NT;
    L.nmin = (int)(want < MIN_BLOCKS ? want : MIN_BLOCKS);
    size_t o = 0;
    L.partial = o; o += up16((size_t)MIN_BLOCKS * 4 * sizeof(float));
    L.origin = o; o += up16(4 * sizeof(double));
    L.flag = o; o += up16((size_t)N * sizeof(int));
    L.off = o; o += up16((size_t)N * sizeof(int));
    L.blksum = o; o += up16((size_t)L.nblk * sizeof(int));
    L.blkoff = o; o += up16((size_t)L.nblk * sizeof(int));
    L.start = o; o += up16(((size_t)N + 1) * sizeof(int));
    L.total = o;
    return L;
}

static int dev_check(const char* fn, int device)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) IN_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, n);
    return LRT_OK;
}

static int work_check(const char* fn, const void* work, size_t work_bytes, size_t need)
{
    if (!work || work_bytes < need) IN_FAIL(LRT_ERR_ARG, "%s: workspace of %zu bytes, need %zu", fn, work_bytes, need);
    if (((uintptr_t)work & 15) != 0) IN_FAIL(LRT_ERR_ARG, "%s: the workspace must be 16-byte aligned", fn);
    return LRT_OK;
}

static int launch_check(const char* fn)
{
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) IN_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

extern "C" {

int lrt_init_abi_version(void) { return LRT_INIT_ABI_VERSION; }

const char* lrt_init_last_error(void) { return g_err; }

size_t lrt_init_normals_work_bytes(int H, int W) { return size_ok(H, W) ? nlayout(H, W).total : 0; }

size_t lrt_init_voxel_work_bytes(long long N) { return count_ok(N) ? vlayout(N).total : 0; }

int lrt_init_normals(int device, int H, int W, const float* rays_o, const float* rays_d, const float* range, const uint8_t* mask, int k,
                     int32_t* nbr, float* normal, void* work, size_t work_bytes, void* stream_)
{
    const char* fn = "lrt_init_normals";
    if (int rc = dev_check(fn, device)) return rc;
    if (!size_ok(H, W)) IN_FAIL(LRT_ERR_ARG, "%s: unsupported image size %d x %d", fn, H, W);
    if (k < 3 || k > IN_KMAX) IN_FAIL(LRT_ERR_ARG, "%s: k = %d, need 3 <= k <= %d", fn, k, IN_KMAX);
    if (!rays_o || !rays_d || !range || !mask || !nbr || !normal) IN_FAIL(LRT_ERR_ARG, "%s: null pointer", fn);
    if (((uintptr_t)nbr & 15) != 0) IN_FAIL(LRT_ERR_ARG, "%s: nbr must be 16-byte aligned", fn);
    if (int rc = work_check(fn, work, work_bytes, lrt_init_normals_work_bytes(H, W))) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) IN_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const NLayout L = nlayout(H, W);
    InFrame a;
    a.H = H; a.W = W; a.ntx = L.ntx; a.nT = L.nT; a.o = rays_o; a.d = rays_d; a.r = range; a.m = mask;
    float4* pts = (float4*)((char*)work + L.pts); float* boxes = (float*)((char*)work + L.boxes);
    hipLaunchKernelGGL(k_in_points, dim3(L.nT), dim3(NT), 0, stream, a, pts, boxes);
    hipLaunchKernelGGL(k_in_knn, dim3(L.nT), dim3(NT), 0, stream, H, W, L.ntx, L.nT, k, (const float4*)pts, (const float*)boxes, nbr);
    hipLaunchKernelGGL(k_in_normal, dim3((H * W + NT - 1) / NT), dim3(NT), 0, stream, a, (const int*)nbr, normal);
    return launch_check(fn);
}

int lrt_init_assign(int device, long long n, const float* point, const float* normal, const uint8_t* mask, int A, const float* pose,
                    const float* size, const uint8_t* present, int32_t* label, float* local_point, float* local_normal, void* stream_)
{
    const char* fn = "lrt_init_assign";
    if (int rc = dev_check(fn, device)) return rc;
    if (!count_ok(n)) IN_FAIL(LRT_ERR_ARG, "%s: unsupported pixel count %lld", fn, n);
    if (A < 0 || A > (1 << 16)) IN_FAIL(LRT_ERR_ARG, "%s: unsupported actor count %d", fn, A);
    if (!point || !normal || !mask || !label || !local_point || !local_normal) IN_FAIL(LRT_ERR_ARG, "%s: null pointer", fn);
    if (A > 0 && (!pose || !size || !present)) IN_FAIL(LRT_ERR_ARG, "%s: null pose / size / present table with %d actors", fn, A);
    LrtDeviceGuard guard(device);
    if (!guard.ok) IN_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipLaunchKernelGGL(k_in_assign, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream_, (int)n, point, normal, mask, A, pose, size, present,
                       label, local_point, local_normal);
    return launch_check(fn);
}

int lrt_init_voxel_keys(int device, long long N, const float* points, double voxel_size, int64_t* keys, int32_t* info, void* work,
                        size_t work_bytes, void* stream_)
{
    const char* fn = "lrt_init_voxel_keys";
    if (int rc = dev_check(fn, device)) return rc;
    if (!count_ok(N)) IN_FAIL(LRT_ERR_ARG, "%s: unsupported point count %lld", fn, N);
    if (!(voxel_size > 0.0) || !(voxel_size < 1e300)) IN_FAIL(LRT_ERR_ARG, "%s: voxel_size must be positive and finite", fn);
    if (!points || !keys || !info) IN_FAIL(LRT_ERR_ARG, "%s: null pointer", fn);
    if (int rc = work_check(fn, work, work_bytes, lrt_init_voxel_work_bytes(N))) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) IN_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const VLayout L = vlayout(N);
    char* w = (char*)work;
    float* partial = (float*)(w + L.partial); double* origin = (double*)(w + L.origin);
    hipLaunchKernelGGL(k_in_vx_min, dim3(L.nmin), dim3(NT), 0, stream, (int)N, points, partial);
    hipLaunchKernelGGL(k_in_vx_origin, dim3(1), dim3(NT), 0, stream, L.nmin, voxel_size, (const float*)partial, origin, (int*)info);
    hipLaunchKernelGGL(k_in_vx_keys, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, stream, (int)N, voxel_size, points, (const double*)origin,
                       (long long*)keys, (int*)info);
    return launch_check(fn);
}

int lrt_init_voxel_mean(int device, long long N, const int64_t* sorted_keys, const int32_t* perm, const float* points, const float* intensity,
                        const float* normals, float* out_points, float* out_intensity, float* out_normals, int32_t* count, int32_t* info,
                        void* work, size_t work_bytes, void* stream_)
{
    const char* fn = "lrt_init_voxel_mean";
    if (int rc = dev_check(fn, device)) return rc;
    if (!count_ok(N)) IN_FAIL(LRT_ERR_ARG, "%s: unsupported point count %lld", fn, N);
    if (!sorted_keys || !perm || !points || !intensity || !normals || !out_points || !out_intensity || !out_normals || !count || !info)
        IN_FAIL(LRT_ERR_ARG, "%s: null pointer", fn);
    if (int rc = work_check(fn, work, work_bytes, lrt_init_voxel_work_bytes(N))) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) IN_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const VLayout L = vlayout(N);
    char* w = (char*)work;
    int *flag = (int*)(w + L.flag), *off = (int*)(w + L.off), *blksum = (int*)(w + L.blksum), *blkoff = (int*)(w + L.blkoff), *start = (int*)(w + L.start);
    const unsigned gpx = (unsigned)((N + NT - 1) / NT);
    hipLaunchKernelGGL(k_in_vx_heads, dim3(gpx), dim3(NT), 0, stream, (int)N, (const long long*)sorted_keys, flag);
    hipLaunchKernelGGL(k_in_scan_blk, dim3(L.nblk), dim3(NT), 0, stream, (int)N, (const int*)flag, off, blksum);
    hipLaunchKernelGGL(k_in_scan_top, dim3(1), dim3(NT), 0, stream, L.nblk, (const int*)blksum, blkoff, (int*)info);
    hipLaunchKernelGGL(k_in_vx_starts, dim3(gpx), dim3(NT), 0, stream, (int)N, (const int*)flag, (const int*)off, (const int*)blkoff, start);
    hipLaunchKernelGGL(k_in_vx_mean, dim3(gpx), dim3(NT), 0, stream, (int)N, (const int*)start, (const int*)perm, points, intensity, normals,
                       (const int*)info, out_points, out_intensity, out_normals, (int*)count);
    return launch_check(fn);
}

}  // extern "C"
