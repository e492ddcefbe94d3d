// lrt_gridcd.hip -- the Chamfer term on the range-image grid (include/lrt_gridcd.h), gfx950.  Compiled into liblrt_gridcd.so, a library of its own.
//
// Forward, three launches:
//   k_gc_points  one workgroup per 8 x 32 tile of the image: both clouds' points of the tile (lrt_gridcd_math.h: gc_point) as float4
//                (x, y, z, linear pixel index) in tile-major order, each cloud's AABB over the tile's valid points and their count.  A pixel that
//                is masked out or outside the image is a padding point at GC_EMPTY; a tile without valid points gets an inverted box.
//   k_gc_search  one workgroup per (tile, direction), one WAVEFRONT per 64 queries of the tile.  The wave first scans the tile it lies in (the
//                counterpart pixels are there: a tight first best), then every other tile whose bound (gc_bound on the tile's box) is <= best
//                for ANY of its lanes (__ballot); the tiles are pre-screened 64 at a time against the wave's query box (gc_bound_box).
//                The visit is wave-uniform, so candidates come through uniform (scalar) loads, in the idiom of kc_query_pk / kc_brute of
//                lrt_chamfer.hip.  best is a u64 (distance bits << 32 | pixel index): its minimum does not depend on the visiting order
//                and ties go to the lower pixel index.  Visiting more tiles than a lane needs only adds candidates a brute-force scan
//                would also see.  The tile's distances are added up in float64 in a fixed order.
//   k_gc_fin     one workgroup adds the tiles' partial sums in a fixed order and forms the means and the loss.
//
// Backward, six launches and one memset, no float atomics:
//   k_gc_bwd_count  per target pixel the length of its inverse neighbour list (integer atomics), and n_a, n_b
//   k_gc_scan_blk / k_gc_scan_top   exclusive scan of the lengths
//   k_gc_bwd_fill   the lists, through integer cursors (their order is arbitrary: the consumer does not depend on it)
//   k_gc_bwd_grad   one thread per pixel: own term + the list in ascending source index (repeated minimum selection, lists of <= GC_SHORT), float64
//   k_gc_bwd_long   pixels with a longer list (a collapsed prediction attracts thousands of points): one wavefront per pixel scans ALL source pixels
//                   in ascending order and tests nn(j) == i, lanes reduced in a fixed order: O(H W) per long list, no O(L^2) cliff
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_gridcd_math.h"
#include "../../include/lrt_gridcd.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int TH = 8, TW = 32, TP = TH * TW, NT = 256, NW = NT / 64;
constexpr int GC_NOIDX = 0x7fffffff;
constexpr int GC_SHORT = 64;               // lists up to this length are summed by their target's thread
constexpr int SCAN_ITEMS = 4, SCAN_BLK = NT * SCAN_ITEMS;
constexpr int LONG_BLOCKS = 128;

struct GcIn {
    int H, W, ntx, nT;
    const float* o; const float* d;
    const float* ra; const uint8_t* ma;
    const float* rb; const uint8_t* mb;
};

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ void gc_pixel_point(const GcIn& a, size_t p, float r, float& x, float& y, float& z)
{
    x = gc_point(a.o[3 * p], a.d[3 * p], r); y = gc_point(a.o[3 * p + 1], a.d[3 * p + 1], r); z = gc_point(a.o[3 * p + 2], a.d[3 * p + 2], r);
}

// ---- forward ---------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_gc_points(GcIn a, float4* __restrict__ pts, float* __restrict__ boxes, int* __restrict__ tcnt)
{
    __shared__ float s_lo[2][3][NW], s_hi[2][3][NW];
    __shared__ int s_n[2][NW];
    const int tile = blockIdx.x, tid = threadIdx.x, ty = tile / a.ntx, tx = tile - ty * a.ntx;
    const int y = ty * TH + tid / TW, x = tx * TW + (tid & (TW - 1));
    const bool in = y < a.H && x < a.W;
    const size_t p = in ? (size_t)y * a.W + x : 0;
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const bool v = in && (c ? a.mb : a.ma)[p] != 0;
        float4 q = make_float4(GC_EMPTY, GC_EMPTY, GC_EMPTY, __int_as_float(GC_NOIDX));
        float lo[3] = {GC_EMPTY, GC_EMPTY, GC_EMPTY}, hi[3] = {-GC_EMPTY, -GC_EMPTY, -GC_EMPTY};
        if (v) {
            gc_pixel_point(a, p, (c ? a.rb : a.ra)[p], q.x, q.y, q.z);
            q.w = __int_as_float((int)p);
            lo[0] = hi[0] = q.x; lo[1] = hi[1] = q.y; lo[2] = hi[2] = q.z;
        }
        pts[((size_t)c * a.nT + tile) * TP + tid] = q;
        const int n = __popcll(__ballot(v));
#pragma unroll
        for (int i = 0; i < 3; i++) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { lo[i] = fminf(lo[i], __shfl_xor(lo[i], o, 64)); hi[i] = fmaxf(hi[i], __shfl_xor(hi[i], o, 64)); }
            if ((tid & 63) == 0) { s_lo[c][i][tid >> 6] = lo[i]; s_hi[c][i][tid >> 6] = hi[i]; }
        }
        if ((tid & 63) == 0) s_n[c][tid >> 6] = n;
    }
    __syncthreads();
    if (tid < 6) {
        const int c = tid / 3, i = tid - 3 * c;
        float lo = s_lo[c][i][0], hi = s_hi[c][i][0];
#pragma unroll
        for (int w = 1; w < NW; w++) { lo = fminf(lo, s_lo[c][i][w]); hi = fmaxf(hi, s_hi[c][i][w]); }
        float* b = boxes + ((size_t)c * a.nT + tile) * 8;
        b[i] = lo; b[4 + i] = hi;                              // an empty tile keeps lo = +GC_EMPTY, hi = -GC_EMPTY: the inverted box
        if (i == 0) {
            int n = 0;
#pragma unroll
            for (int w = 0; w < NW; w++) n += s_n[c][w];
            tcnt[c * a.nT + tile] = n;
            b[3] = 0.f; b[7] = 0.f;
        }
    }
}

__device__ __forceinline__ float gc_wave_max(float v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

__device__ __forceinline__ void gc_scan_tile(const float4* __restrict__ pp, float qx, float qy, float qz, unsigned long long& bk)
{
#pragma unroll 8
    for (int e = 0; e < TP; e++) {
        const float4 v = pp[e];                                // uniform address: scalar load
        const float d = gc_d2(gc_sub(v.x, qx), gc_sub(v.y, qy), gc_sub(v.z, qz));
        const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | (unsigned)__float_as_int(v.w);   // d >= +0: bit order = value order
        bk = key < bk ? key : bk;                              // a padding point's distance is +inf: above the initial best
    }
}

__global__ __launch_bounds__(NT) void k_gc_search(int H, int W, int ntx, int nT, const float4* __restrict__ pts, const float* __restrict__ boxes,
                                                  float* __restrict__ dist_a, float* __restrict__ dist_b, int* __restrict__ idx_a,
                                                  int* __restrict__ idx_b, double* __restrict__ partials)
{
    __shared__ double red[NW];
    const int tile = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y = ty * TH + tid / TW, x = tx * TW + (tid & (TW - 1));
    const bool in = y < H && x < W;
    const float4 q = pts[((size_t)dir * nT + tile) * TP + tid];
    const bool valid = __float_as_int(q.w) != GC_NOIDX;
    const float4* __restrict__ cp = pts + (size_t)(1 - dir) * nT * TP;
    const float* __restrict__ cb = boxes + (size_t)(1 - dir) * nT * 8;
    unsigned long long bk = ((unsigned long long)__float_as_uint(GC_BIG) << 32) | (unsigned)GC_NOIDX;
    if (__ballot(valid) != 0) {                                // wave-uniform from here on
        const int lane = tid & 63;
        // the wave's query box: a tile whose box-to-box bound is above every lane's best is needed by no lane (gc_bound_box), so the tiles are
        // tested 64 at a time, one per lane, and only the survivors get the exact per-lane test
        float ql[3] = {valid ? q.x : GC_EMPTY, valid ? q.y : GC_EMPTY, valid ? q.z : GC_EMPTY};
        float qh[3] = {valid ? q.x : -GC_EMPTY, valid ? q.y : -GC_EMPTY, valid ? q.z : -GC_EMPTY};
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { ql[i] = fminf(ql[i], __shfl_xor(ql[i], o, 64)); qh[i] = fmaxf(qh[i], __shfl_xor(qh[i], o, 64)); }
        gc_scan_tile(cp + (size_t)tile * TP, q.x, q.y, q.z, bk);
        float wmax = gc_wave_max(valid ? __uint_as_float((unsigned)(bk >> 32)) : 0.f);
        for (int c0 = 0; c0 < nT; c0 += 64) {
            const int tl = c0 + lane;
            float bb = __uint_as_float(0x7f800000u);
            if (tl < nT && tl != tile) {
                const float4 blo = *reinterpret_cast<const float4*>(cb + (size_t)tl * 8), bhi = *reinterpret_cast<const float4*>(cb + (size_t)tl * 8 + 4);
                bb = gc_bound_box(blo.x, blo.y, blo.z, bhi.x, bhi.y, bhi.z, ql[0], ql[1], ql[2], qh[0], qh[1], qh[2]);
            }
            unsigned long long m = __ballot(bb <= wmax);       // wmax only falls while the chunk is worked off: a stale value visits more, never less
            while (m != 0) {
                const int t = __builtin_amdgcn_readfirstlane(c0 + (int)__ffsll((long long)m) - 1);
                m &= m - 1;
                const float* __restrict__ b = cb + (size_t)t * 8;
                const float lb = gc_bound(b[0], b[1], b[2], b[4], b[5], b[6], q.x, q.y, q.z);
                // <=, not <: a tile at exactly the best distance may hold a tie with a lower pixel index
                if (__ballot(valid && lb <= __uint_as_float((unsigned)(bk >> 32))) == 0) continue;
                gc_scan_tile(cp + (size_t)t * TP, q.x, q.y, q.z, bk);
                wmax = gc_wave_max(valid ? __uint_as_float((unsigned)(bk >> 32)) : 0.f);
            }
        }
    }
    float best = __uint_as_float((unsigned)(bk >> 32));
    int bi = (int)(unsigned)bk;
    if (!valid || bi == GC_NOIDX) { best = 0.f; bi = -1; }     // a masked pixel, or an empty other cloud
    if (in) {
        const size_t p = (size_t)y * W + x;
        (dir ? dist_b : dist_a)[p] = best;
        (dir ? idx_b : idx_a)[p] = bi;
    }
    // fixed order: lanes by the shuffle tree, then the waves by index
    const double s = wave_sum((double)best);
    if ((tid & 63) == 0) red[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        double t = red[0];
#pragma unroll
        for (int w = 1; w < NW; w++) t += red[w];
        partials[(size_t)dir * nT + tile] = t;
    }
}

__global__ __launch_bounds__(NT) void k_gc_fin(int nT, double weight, const double* __restrict__ partials, const int* __restrict__ tcnt, float* __restrict__ out)
{
    __shared__ double sh[2][NT];
    __shared__ long long sn[2][NT];
    const int tid = threadIdx.x;
    double s[2] = {0, 0}; long long n[2] = {0, 0};
    for (int r = tid; r < nT; r += NT) { s[0] += partials[r]; s[1] += partials[(size_t)nT + r]; n[0] += tcnt[r]; n[1] += tcnt[nT + r]; }
    sh[0][tid] = s[0]; sh[1][tid] = s[1]; sn[0][tid] = n[0]; sn[1][tid] = n[1];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o) { sh[0][tid] += sh[0][tid + o]; sh[1][tid] += sh[1][tid + o]; sn[0][tid] += sn[0][tid + o]; sn[1][tid] += sn[1][tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        const bool some = sn[0][0] > 0 && sn[1][0] > 0;
        const double ma = some ? sh[0][0] / (double)sn[0][0] : 0.0, mb = some ? sh[1][0] / (double)sn[1][0] : 0.0;
        out[0] = some ? (float)(weight * 0.5 * (ma + mb)) : 0.f; out[1] = (float)ma; out[2] = (float)mb; out[3] = (float)sn[0][0];
    }
}

// ---- backward --------------------------------------------------------------------------------------------------------------------------------
// Zeroed header of the backward's workspace
struct GcHdr { int n_a, n_b, nlong, pad; };

// Direction 0: the targets are A's pixels, the sources B's (nn_b(j) = i); direction 1 the other way round.  cnt / cur / off are indexed by
// dir * HW + target pixel.
template <bool FILL>
__global__ __launch_bounds__(NT) void k_gc_bwd_count(GcIn a, int ndir, const int* __restrict__ idx_a, const int* __restrict__ idx_b, GcHdr* hdr,
                                                     int* cnt, const int* __restrict__ off, const int* __restrict__ blkoff, int* __restrict__ list)
{
    const int HW = a.H * a.W, j = blockIdx.x * NT + threadIdx.x;
    const bool in = j < HW;
    const bool va = in && a.ma[j] != 0, vb = in && a.mb[j] != 0;
    if (!FILL) {
        const int na = __popcll(__ballot(va)), nb = __popcll(__ballot(vb));
        if ((threadIdx.x & 63) == 0) { if (na) atomicAdd(&hdr->n_a, na); if (nb) atomicAdd(&hdr->n_b, nb); }
    }
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {
        if (dir >= ndir) break;
        if (!(dir ? va : vb)) continue;
        const int t = (dir ? idx_a : idx_b)[j];
        if ((unsigned)t >= (unsigned)HW) continue;             // -1 (no neighbour), or not an index of this image
        const int g = dir * HW + t;
        const int pos = atomicAdd(&cnt[g], 1);
        if (FILL) list[off[g] + blkoff[g / SCAN_BLK] + pos] = j;
    }
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

__global__ __launch_bounds__(NT) void k_gc_scan_blk(int n, const int* __restrict__ cnt, int* __restrict__ off, int* __restrict__ blksum)
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

__global__ __launch_bounds__(NT) void k_gc_scan_top(int nblk, const int* __restrict__ blksum, int* __restrict__ blkoff)
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
}

struct GcBwd {
    double weight;
    const int* idx_a; const int* idx_b;
    const float* d_loss;
    const GcHdr* hdr;
    const int* cnt; const int* off; const int* blkoff; const int* list;
    float* d_range_a; float* d_o; float* d_d;
};

// The finished pixel: d_range_a = grad_a . d, and the rays' gradients from both clouds.
__device__ __forceinline__ void gc_write_grad(const GcIn& a, const GcBwd& b, size_t p, const double* GA, const double* GB)
{
    const float dx = a.d[3 * p], dy = a.d[3 * p + 1], dz = a.d[3 * p + 2];
    b.d_range_a[p] = (float)(GA[0] * (double)dx + GA[1] * (double)dy + GA[2] * (double)dz);
    if (b.d_o) {
        const double ra = (double)a.ra[p], rb = (double)a.rb[p];
#pragma unroll
        for (int i = 0; i < 3; i++) {
            b.d_o[3 * p + i] = (float)(GA[i] + GB[i]);
            // a cloud without this pixel has no gradient here, whatever its range map holds (0 * inf would be NaN)
            b.d_d[3 * p + i] = (float)((GA[i] != 0.0 ? ra * GA[i] : 0.0) + (GB[i] != 0.0 ? rb * GB[i] : 0.0));
        }
    }
}

__device__ __forceinline__ void gc_scales(const GcBwd& b, double& ga, double& gb)
{
    const int na = b.hdr->n_a, nb = b.hdr->n_b;
    const double up = (double)b.d_loss[0] * b.weight * 0.5;
    const bool some = na > 0 && nb > 0;
    ga = some ? 2.0 * up / (double)na : 0.0; gb = some ? 2.0 * up / (double)nb : 0.0;
}

__global__ __launch_bounds__(NT) void k_gc_bwd_grad(GcIn a, GcBwd b, GcHdr* hdr_w, int* __restrict__ longq)
{
    const int HW = a.H * a.W, p = blockIdx.x * NT + threadIdx.x;
    if (p >= HW) return;
    double ga, gb;
    gc_scales(b, ga, gb);
    const bool rays = b.d_o != nullptr;
    double G[2][3] = {{0, 0, 0}, {0, 0, 0}};
    bool is_long = false;
#pragma unroll
    for (int dir = 0; dir < 2; dir++) {                          // dir 0: this pixel as a point of A (sources in B); dir 1: as a point of B
        if (dir == 1 && !rays) break;
        if ((dir ? a.mb : a.ma)[p] == 0) continue;
        const float* rs = dir ? a.rb : a.ra; const float* ro = dir ? a.ra : a.rb;
        const double g_own = dir ? gb : ga, g_lst = dir ? ga : gb;
        float sx, sy, sz;
        gc_pixel_point(a, p, rs[p], sx, sy, sz);
        const int nn = (dir ? b.idx_b : b.idx_a)[p];
        if ((unsigned)nn < (unsigned)HW) {
            float ox, oy, oz;
            gc_pixel_point(a, nn, ro[nn], ox, oy, oz);
            G[dir][0] = g_own * ((double)sx - (double)ox); G[dir][1] = g_own * ((double)sy - (double)oy); G[dir][2] = g_own * ((double)sz - (double)oz);
        }
        const int g = dir * HW + p, L = b.cnt[g];
        if (L > GC_SHORT) { is_long = true; continue; }
        const int* lst = b.list + b.off[g] + b.blkoff[g / SCAN_BLK];
        double S[3] = {0, 0, 0};
        int prev = -1;
        for (int k = 0; k < L; k++) {                            // ascending source index, whatever order the cursors left
            int m = GC_NOIDX;
            for (int e = 0; e < L; e++) { const int v = lst[e]; if (v > prev && v < m) m = v; }
            prev = m;
            float ox, oy, oz;
            gc_pixel_point(a, m, ro[m], ox, oy, oz);
            S[0] += (double)sx - (double)ox; S[1] += (double)sy - (double)oy; S[2] += (double)sz - (double)oz;
        }
        G[dir][0] += g_lst * S[0]; G[dir][1] += g_lst * S[1]; G[dir][2] += g_lst * S[2];
    }
    if (is_long) { longq[atomicAdd(&hdr_w->nlong, 1)] = p; return; }       // k_gc_bwd_long writes this pixel
    gc_write_grad(a, b, p, G[0], G[1]);
}

__global__ __launch_bounds__(NT) void k_gc_bwd_long(GcIn a, GcBwd b, const int* __restrict__ longq)
{
    const int HW = a.H * a.W, lane = threadIdx.x & 63;
    const int nlong = b.hdr->nlong, nwaves = gridDim.x * NW;
    double ga, gb;
    gc_scales(b, ga, gb);
    const bool rays = b.d_o != nullptr;
    for (int q = blockIdx.x * NW + (threadIdx.x >> 6); q < nlong; q += nwaves) {
        const int p = longq[q];
        double G[2][3] = {{0, 0, 0}, {0, 0, 0}};
        for (int dir = 0; dir < 2; dir++) {
            if (dir == 1 && !rays) break;
            if ((dir ? a.mb : a.ma)[p] == 0) continue;
            const float* rs = dir ? a.rb : a.ra; const float* ro = dir ? a.ra : a.rb;
            const uint8_t* mo = dir ? a.ma : a.mb; const int* io = dir ? b.idx_a : b.idx_b;
            const double g_own = dir ? gb : ga, g_lst = dir ? ga : gb;
            float sx, sy, sz;
            gc_pixel_point(a, p, rs[p], sx, sy, sz);
            double S[3] = {0, 0, 0};
            for (int j = lane; j < HW; j += 64) {              // every lane in ascending j
                if (mo[j] == 0 || io[j] != p) continue;
                float ox, oy, oz;
                gc_pixel_point(a, j, ro[j], ox, oy, oz);
                S[0] += (double)sx - (double)ox; S[1] += (double)sy - (double)oy; S[2] += (double)sz - (double)oz;
            }
#pragma unroll
            for (int i = 0; i < 3; i++) S[i] = wave_sum(S[i]);   // fixed lane order
            const int nn = (dir ? b.idx_b : b.idx_a)[p];
            if ((unsigned)nn < (unsigned)HW) {
                float ox, oy, oz;
                gc_pixel_point(a, nn, ro[nn], ox, oy, oz);
                G[dir][0] = g_own * ((double)sx - (double)ox); G[dir][1] = g_own * ((double)sy - (double)oy); G[dir][2] = g_own * ((double)sz - (double)oz);
            }
            G[dir][0] += g_lst * S[0]; G[dir][1] += g_lst * S[1]; G[dir][2] += g_lst * S[2];
        }
        if (lane == 0) gc_write_grad(a, b, p, G[0], G[1]);
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define GC_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline bool size_ok(int H, int W) { return H > 0 && W > 0 && W <= (1 << 20) && (size_t)H * W <= ((size_t)1 << 27); }
static inline size_t up16(size_t n) { return (n + 15) / 16 * 16; }

struct Layout {
    int ntx, nT, HW, nblk;
    size_t pts, boxes, tcnt, partials;                       // forward
    size_t hdr, cnt, cur, off, blksum, blkoff, list, longq;   // backward (hdr, cnt, cur contiguous: one memset)
    size_t zero_bytes, total;
};

static Layout layout(int H, int W)
{
    Layout L;
    L.ntx = (W + TW - 1) / TW; L.nT = L.ntx * ((H + TH - 1) / TH); L.HW = H * W;
    const size_t n2 = 2 * (size_t)L.HW;
    L.nblk = (int)((n2 + SCAN_BLK - 1) / SCAN_BLK);
    size_t o = 0;
    L.pts = o; o += 2 * (size_t)L.nT * TP * sizeof(float4);
    L.boxes = o; o += up16(2 * (size_t)L.nT * 8 * sizeof(float));
    L.tcnt = o; o += up16(2 * (size_t)L.nT * sizeof(int));
    L.partials = o; o += up16(2 * (size_t)L.nT * sizeof(double));
    L.hdr = o; o += up16(sizeof(GcHdr));
    L.cnt = o; o += up16(n2 * sizeof(int));
    L.cur = o; o += up16(n2 * sizeof(int));
    L.zero_bytes = o - L.hdr;
    L.off = o; o += up16(n2 * sizeof(int));
    L.blksum = o; o += up16((size_t)L.nblk * sizeof(int));
    L.blkoff = o; o += up16((size_t)L.nblk * sizeof(int));
    L.list = o; o += up16(n2 * sizeof(int));
    L.longq = o; o += up16((size_t)L.HW * sizeof(int));
    L.total = o;
    return L;
}

static int gc_check(const char* fn, int device, int H, int W, const void* o, const void* d, const void* ra, const void* ma, const void* rb,
                    const void* mb, double weight, const void* work, size_t work_bytes)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) GC_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, n);
    if (!size_ok(H, W)) GC_FAIL(LRT_ERR_ARG, "%s: unsupported image size %d x %d", fn, H, W);
    if (!o || !d || !ra || !ma || !rb || !mb) GC_FAIL(LRT_ERR_ARG, "%s: null ray / range / mask pointer", fn);
    if (!(weight == weight)) GC_FAIL(LRT_ERR_ARG, "%s: the weight is NaN", fn);
    if (!work || work_bytes < lrt_gridcd_work_bytes(H, W)) GC_FAIL(LRT_ERR_ARG, "%s: workspace of %zu bytes, need %zu", fn, work_bytes, lrt_gridcd_work_bytes(H, W));
    if (((uintptr_t)work & 15) != 0) GC_FAIL(LRT_ERR_ARG, "%s: the workspace must be 16-byte aligned", fn);
    return LRT_OK;
}

static GcIn make_in(const Layout& L, int H, int W, const float* o, const float* d, const float* ra, const uint8_t* ma, const float* rb, const uint8_t* mb)
{
    GcIn a;
    a.H = H; a.W = W; a.ntx = L.ntx; a.nT = L.nT; a.o = o; a.d = d; a.ra = ra; a.ma = ma; a.rb = rb; a.mb = mb;
    return a;
}

extern "C" {

int lrt_gridcd_abi_version(void) { return LRT_GRIDCD_ABI_VERSION; }

const char* lrt_gridcd_last_error(void) { return g_err; }

size_t lrt_gridcd_work_bytes(int H, int W)
{
    if (!size_ok(H, W)) return 0;
    return layout(H, W).total;
}

int lrt_gridcd_forward(int device, int H, int W, const float* rays_o, const float* rays_d, const float* range_a, const uint8_t* mask_a,
                       const float* range_b, const uint8_t* mask_b, double weight, float* out, float* dist_a, float* dist_b,
                       int32_t* idx_a, int32_t* idx_b, void* work, size_t work_bytes, void* stream_)
{
    const char* fn = "lrt_gridcd_forward";
    if (int rc = gc_check(fn, device, H, W, rays_o, rays_d, range_a, mask_a, range_b, mask_b, weight, work, work_bytes)) return rc;
    if (!out || !dist_a || !dist_b || !idx_a || !idx_b) GC_FAIL(LRT_ERR_ARG, "%s: null output pointer", fn);
    LrtDeviceGuard guard(device);
    if (!guard.ok) GC_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const Layout L = layout(H, W);
    const GcIn a = make_in(L, H, W, rays_o, rays_d, range_a, mask_a, range_b, mask_b);
    char* w = (char*)work;
    float4* pts = (float4*)(w + L.pts); float* boxes = (float*)(w + L.boxes); int* tcnt = (int*)(w + L.tcnt); double* partials = (double*)(w + L.partials);
    hipLaunchKernelGGL(k_gc_points, dim3(L.nT), dim3(NT), 0, stream, a, pts, boxes, tcnt);
    hipLaunchKernelGGL(k_gc_search, dim3(L.nT, 2), dim3(NT), 0, stream, H, W, L.ntx, L.nT, (const float4*)pts, (const float*)boxes, dist_a, dist_b,
                       idx_a, idx_b, partials);
    hipLaunchKernelGGL(k_gc_fin, dim3(1), dim3(NT), 0, stream, L.nT, weight, (const double*)partials, (const int*)tcnt, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) GC_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_gridcd_backward(int device, int H, int W, const float* rays_o, const float* rays_d, const float* range_a, const uint8_t* mask_a,
                        const float* range_b, const uint8_t* mask_b, double weight, const int32_t* idx_a, const int32_t* idx_b,
                        const float* d_loss, float* d_range_a, float* d_rays_o, float* d_rays_d, void* work, size_t work_bytes,
                        void* stream_)
{
    const char* fn = "lrt_gridcd_backward";
    if (int rc = gc_check(fn, device, H, W, rays_o, rays_d, range_a, mask_a, range_b, mask_b, weight, work, work_bytes)) return rc;
    if (!idx_a || !idx_b || !d_loss || !d_range_a) GC_FAIL(LRT_ERR_ARG, "%s: null index / gradient pointer", fn);
    if ((d_rays_o == nullptr) != (d_rays_d == nullptr)) GC_FAIL(LRT_ERR_ARG, "%s: d_rays_o and d_rays_d go together (both or neither)", fn);
    LrtDeviceGuard guard(device);
    if (!guard.ok) GC_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const Layout L = layout(H, W);
    const GcIn a = make_in(L, H, W, rays_o, rays_d, range_a, mask_a, range_b, mask_b);
    char* w = (char*)work;
    GcHdr* hdr = (GcHdr*)(w + L.hdr);
    int *cnt = (int*)(w + L.cnt), *cur = (int*)(w + L.cur), *off = (int*)(w + L.off), *blksum = (int*)(w + L.blksum), *blkoff = (int*)(w + L.blkoff);
    int *list = (int*)(w + L.list), *longq = (int*)(w + L.longq);
    const int ndir = d_rays_o ? 2 : 1, n = ndir * L.HW, nblk = (n + SCAN_BLK - 1) / SCAN_BLK, gpx = (L.HW + NT - 1) / NT;
    if (hipMemsetAsync(w + L.hdr, 0, L.zero_bytes, stream) != hipSuccess) GC_FAIL(LRT_ERR_HIP, "%s: hipMemsetAsync failed", fn);
    hipLaunchKernelGGL(k_gc_bwd_count<false>, dim3(gpx), dim3(NT), 0, stream, a, ndir, idx_a, idx_b, hdr, cnt, (const int*)nullptr, (const int*)nullptr, (int*)nullptr);
    hipLaunchKernelGGL(k_gc_scan_blk, dim3(nblk), dim3(NT), 0, stream, n, (const int*)cnt, off, blksum);
    hipLaunchKernelGGL(k_gc_scan_top, dim3(1), dim3(NT), 0, stream, nblk, (const int*)blksum, blkoff);
    hipLaunchKernelGGL(k_gc_bwd_count<true>, dim3(gpx), dim3(NT), 0, stream, a, ndir, idx_a, idx_b, hdr, cur, (const int*)off, (const int*)blkoff, list);
    GcBwd b;
    b.weight = weight; b.idx_a = idx_a; b.idx_b = idx_b; b.d_loss = d_loss; b.hdr = hdr; b.cnt = cnt; b.off = off; b.blkoff = blkoff; b.list = list;
    b.d_range_a = d_range_a; b.d_o = d_rays_o; b.d_d = d_rays_d;
    hipLaunchKernelGGL(k_gc_bwd_grad, dim3(gpx), dim3(NT), 0, stream, a, b, hdr, longq);
    hipLaunchKernelGGL(k_gc_bwd_long, dim3(LONG_BLOCKS), dim3(NT), 0, stream, a, b, (const int*)longq);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) GC_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
