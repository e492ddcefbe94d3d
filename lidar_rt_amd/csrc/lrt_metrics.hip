// lrt_metrics.hip -- the fused evaluation metrics of one frame (include/lrt_metrics.h), gfx950.  Compiled into liblrt_metrics.so, a library of its own.
//
// One memset (the histograms) and ten launches, no float atomics, no host wait:
//   k_mt_pass1    one workgroup per 512 pixels: the clamped pairs and e = y - x of both images (lrt_metrics_math.h), the keys |e| into the
//                 workspace, per-workgroup float64 sums of e^2 and |e|, min / max of y, the exact tp / fp / fn / eq / n_pred / n_gt counts, and
//                 the level-1 histograms of the keys: in LDS first, the non-empty bins then by integer atomics into the workspace.
//   k_mt_reduce1  one workgroup adds the partials in a fixed order: rmse, mae, psnr, the ray-drop figures, the counts; R = max y - min y for SSIM.
//   k_mt_scan<L>  one workgroup scans a level's histograms and finds, for BOTH middle ranks of both images, the bin and the rank inside it
//                 (mt_find_bin).  The two ranks may fall into different bins at any level; from then on each follows its own prefix.
//   k_mt_hist<L>  levels 2 and 3: the keys that carry a rank's prefix, counted by their next digit (LDS, then integer atomics).
//                 After level 3 both keys are known to the bit: medae = 0.5f * (lo + hi).
//   k_mt_ssim     one workgroup per 16 x 32 tile of the SSIM interior: the tile with its 3-pixel halo in LDS, the five 7-tap row sums of every
//                 row into LDS (float64), then per output pixel the 7 rows added in registers and the window term; the tile's sum in a fixed order.
//   k_mt_points   per-workgroup sums of dist_a / dist_b over the two clouds and the counts below the F-score threshold.
//   k_mt_fin      one workgroup adds the tile and point partials in a fixed order: ssim, chamfer_dist, fscore.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_metrics_math.h"
#include "../../include/lrt_metrics.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = 256, NW = NT / 64;
constexpr int PXB = 512;                       // pixels per workgroup of the pixel passes (2 per thread)
constexpr int STY = 16, STX = 32;              // SSIM: output tile; the input tile has 3 pixels more on every side
constexpr int SIY = STY + MT_WIN - 1, SIX = STX + MT_WIN - 1;

struct MtSel { uint32_t prefix[2], rank[2]; };                    // per image: the two middle ranks on their way down
struct MtHdr { MtSel sel[4][2]; double R[2]; double pad[2]; };    // sel[level][image] = what level `level` starts from (sel[3]: the final keys)

struct MtIn {
    int H, W, HW, use_gt;
    const float* pd; const float* pi; const float* pr;
    const float* gd; const float* gi; const uint8_t* gm;
    float ratio, max_depth;
};

__device__ __forceinline__ bool mt_pred_hit(const MtIn& a, int p) { return a.pr[p] < a.ratio; }

// The clamped pair of image c at pixel p: x the prediction, y the ground truth.
__device__ __forceinline__ void mt_pair(const MtIn& a, int c, int p, float& x, float& y)
{
    const bool m = a.use_gt ? a.gm[p] != 0 : mt_pred_hit(a, p);
    if (c == 0) { y = mt_depth_gt(a.gd[p], a.max_depth); x = mt_depth_pred(a.pd[p], m, a.max_depth); }
    else { y = mt_intensity_gt(a.gi[p]); x = mt_intensity_pred(a.pi[p], m); }
}

// ---- fixed-order workgroup reductions: lanes by the shuffle tree, then the waves by index; the result is valid in thread 0 ---------------------------
__device__ __forceinline__ double block_sum(double v, double* s_red)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = s_red[0];
#pragma unroll
    for (int w = 1; w < NW; w++) t += s_red[w];
    return t;
}

__device__ __forceinline__ int block_count(bool pred0, bool pred1, int* s_red)
{
    const int c = __popcll(__ballot(pred0)) + __popcll(__ballot(pred1));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = c;
    __syncthreads();
    int t = s_red[0];
#pragma unroll
    for (int w = 1; w < NW; w++) t += s_red[w];
    return t;
}

__device__ __forceinline__ void block_minmax(float lo, float hi, float* s_lo, float* s_hi, float& out_lo, float& out_hi)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { lo = fminf(lo, __shfl_xor(lo, o, 64)); hi = fmaxf(hi, __shfl_xor(hi, o, 64)); }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    out_lo = s_lo[0]; out_hi = s_hi[0];
#pragma unroll
    for (int w = 1; w < NW; w++) { out_lo = fminf(out_lo, s_lo[w]); out_hi = fmaxf(out_hi, s_hi[w]); }
}

// ---- pass 1 --------------------------------------------------------------------------------------------------------------------------------------
// partials per workgroup: pd[blk][4] = sum e^2 (depth, intensity), sum |e| (depth, intensity); pf[blk][4] = min y, max y (depth), min y, max y (intensity);
// pn[blk][6] = tp, fp, fn, eq, n_pred, n_gt
__global__ __launch_bounds__(NT) void k_mt_pass1(MtIn a, uint32_t* __restrict__ keys, uint32_t* __restrict__ hist1, double* __restrict__ pd,
                                                 float* __restrict__ pf, int* __restrict__ pn)
{
    __shared__ uint32_t s_h[2][MT_L1_BINS];
    __shared__ double s_d[NW];
    __shared__ float s_lo[NW], s_hi[NW];
    __shared__ int s_n[NW];
    const int tid = threadIdx.x, blk = blockIdx.x;
    for (int i = tid; i < 2 * MT_L1_BINS; i += NT) (&s_h[0][0])[i] = 0u;
    __syncthreads();
    double sq[2] = {0, 0}, ab[2] = {0, 0};
    float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    bool in[2], gdrop[2], pdrop[2], msk[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int p = blk * PXB + k * NT + tid;
        in[k] = p < a.HW;
        gdrop[k] = pdrop[k] = msk[k] = false;
        if (!in[k]) continue;
        const bool ghit = a.gm[p] != 0, phit = mt_pred_hit(a, p);
        gdrop[k] = !ghit; pdrop[k] = !phit; msk[k] = a.use_gt ? ghit : phit;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            float x, y;
            mt_pair(a, c, p, x, y);
            const float e = y - x;
            const uint32_t key = mt_abs_key(e);
            keys[(size_t)c * a.HW + p] = key;
            atomicAdd(&s_h[c][mt_digit(key, 1)], 1u);
            const double ed = (double)e;
            sq[c] += ed * ed; ab[c] += fabs(ed);
            lo[c] = fminf(lo[c], y); hi[c] = fmaxf(hi[c], y);
        }
    }
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const double tsq = block_sum(sq[c], s_d), tab = block_sum(ab[c], s_d);
        float blo, bhi;
        block_minmax(lo[c], hi[c], s_lo, s_hi, blo, bhi);
        if (tid == 0) { pd[blk * 4 + c] = tsq; pd[blk * 4 + 2 + c] = tab; pf[blk * 4 + 2 * c] = blo; pf[blk * 4 + 2 * c + 1] = bhi; }
    }
    const int tp = block_count(in[0] && gdrop[0] && pdrop[0], in[1] && gdrop[1] && pdrop[1], s_n);
    const int fp = block_count(in[0] && !gdrop[0] && pdrop[0], in[1] && !gdrop[1] && pdrop[1], s_n);
    const int fn = block_count(in[0] && gdrop[0] && !pdrop[0], in[1] && gdrop[1] && !pdrop[1], s_n);
    const int eq = block_count(in[0] && gdrop[0] == pdrop[0], in[1] && gdrop[1] == pdrop[1], s_n);
    const int np = block_count(in[0] && msk[0], in[1] && msk[1], s_n);
    const int ng = block_count(in[0] && !gdrop[0], in[1] && !gdrop[1], s_n);
    if (tid == 0) { int* q = pn + blk * 6; q[0] = tp; q[1] = fp; q[2] = fn; q[3] = eq; q[4] = np; q[5] = ng; }
    __syncthreads();                                                   // the LDS histograms are complete (block_count's barriers came after the last atomic)
    for (int i = tid; i < 2 * MT_L1_BINS; i += NT) {
        const uint32_t v = (&s_h[0][0])[i];
        if (v) atomicAdd(&hist1[i], v);
    }
}

__global__ __launch_bounds__(NT) void k_mt_reduce1(int nblk, int HW, double max_depth, const double* __restrict__ pd, const float* __restrict__ pf,
                                                   const int* __restrict__ pn, MtHdr* __restrict__ hdr, int* __restrict__ counts, float* __restrict__ out)
{
    __shared__ double s_d[NW];
    __shared__ float s_lo[NW], s_hi[NW];
    const int tid = threadIdx.x;
    double d[4] = {0, 0, 0, 0};
    float lo[2] = {INFINITY, INFINITY}, hi[2] = {-INFINITY, -INFINITY};
    long long n[6] = {0, 0, 0, 0, 0, 0};
    for (int r = tid; r < nblk; r += NT) {
#pragma unroll
        for (int i = 0; i < 4; i++) d[i] += pd[r * 4 + i];
#pragma unroll
        for (int c = 0; c < 2; c++) { lo[c] = fminf(lo[c], pf[r * 4 + 2 * c]); hi[c] = fmaxf(hi[c], pf[r * 4 + 2 * c + 1]); }
#pragma unroll
        for (int i = 0; i < 6; i++) n[i] += pn[r * 6 + i];
    }
    double D[4], N[6];
    float LO[2], HI[2];
#pragma unroll
    for (int i = 0; i < 4; i++) D[i] = block_sum(d[i], s_d);
#pragma unroll
    for (int i = 0; i < 6; i++) N[i] = block_sum((double)n[i], s_d);   // integers below 2^27: exact in float64, any order
#pragma unroll
    for (int c = 0; c < 2; c++) block_minmax(lo[c], hi[c], s_lo, s_hi, LO[c], HI[c]);
    if (tid == 0) {
        const double nn = (double)HW;
#pragma unroll
        for (int c = 0; c < 2; c++) {
            float* o = out + (c ? LRT_METRICS_INTENSITY_RMSE : LRT_METRICS_DEPTH_RMSE);
            o[0] = (float)mt_rmse(D[c], nn);
            o[1] = (float)(D[2 + c] / nn);
            o[4] = (float)mt_psnr(D[c], nn, c ? 1.0 : max_depth);
            hdr->R[c] = (double)HI[c] - (double)LO[c];
        }
        out[LRT_METRICS_RAYDROP_RMSE] = (float)sqrt((nn - N[3]) / nn);
        out[LRT_METRICS_RAYDROP_ACC] = (float)(N[3] / nn);
        out[LRT_METRICS_RAYDROP_F1] = (float)mt_f1(N[0], N[1], N[2]);
        out[LRT_METRICS_POINTS_N_PRED] = (float)N[4];
        out[LRT_METRICS_POINTS_N_GT] = (float)N[5];
        counts[0] = (int)N[4]; counts[1] = (int)N[5];
    }
}

// ---- selection -----------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t* s_w)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const uint32_t u = __shfl_up(inc, o, 64); if (lane >= o) inc += u; }
    __syncthreads();
    if (lane == 63) s_w[wv] = inc;
    __syncthreads();
    uint32_t base = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) if (w < wv) base += s_w[w];
    return base + inc - v;
}

// Level 1: one histogram per image, the two ranks (n - 1) / 2 and n / 2.  Levels 2, 3: one histogram per (image, rank), the rank inside the bin
// the level above selected.  hist: [image][MT_L1_BINS] or [image][rank][bins].
template <int LEVEL>
__global__ __launch_bounds__(NT) void k_mt_scan(int HW, const uint32_t* __restrict__ hist, MtHdr* __restrict__ hdr, float* __restrict__ out)
{
    constexpr int NB = LEVEL == 1 ? MT_L1_BINS : LEVEL == 2 ? MT_L2_BINS : MT_L3_BINS, PER = NB / NT;
    __shared__ uint32_t s_w[NW];
    const int tid = threadIdx.x;
    for (int j = 0; j < 4; j++) {
        const int c = j >> 1, s = j & 1;
        const uint32_t* h = hist + (size_t)(LEVEL == 1 ? c : j) * NB + tid * PER;
        const uint32_t k = LEVEL == 1 ? (s ? mt_rank_hi((uint32_t)HW) : mt_rank_lo((uint32_t)HW)) : hdr->sel[LEVEL - 1][c].rank[s];
        const uint32_t prefix = LEVEL == 1 ? 0u : hdr->sel[LEVEL - 1][c].prefix[s];
        uint32_t mine[PER], sum = 0;
#pragma unroll
        for (int i = 0; i < PER; i++) { mine[i] = h[i]; sum += mine[i]; }
        const uint32_t before = block_excl_scan(sum, s_w);
        uint32_t r;
        const int b = mt_find_bin(mine, PER, before, k, &r);
        if (b >= 0) {                                                  // exactly one thread holds rank k
            hdr->sel[LEVEL][c].prefix[s] = mt_extend(prefix, (uint32_t)(tid * PER + b), LEVEL);
            hdr->sel[LEVEL][c].rank[s] = r;
        }
    }
    if (LEVEL == 3) {
        __threadfence_block();
        __syncthreads();
        if (tid < 2) {
            const MtSel f = hdr->sel[3][tid];
            out[tid ? LRT_METRICS_INTENSITY_MEDAE : LRT_METRICS_DEPTH_MEDAE] = mt_median(f.prefix[0], f.prefix[1]);
        }
    }
}

template <int LEVEL>
__global__ __launch_bounds__(NT) void k_mt_hist(int HW, const uint32_t* __restrict__ keys, const MtHdr* __restrict__ hdr, uint32_t* __restrict__ hist)
{
    constexpr int NB = LEVEL == 2 ? MT_L2_BINS : MT_L3_BINS;
    __shared__ uint32_t s_h[4 * NB];
    const int tid = threadIdx.x;
    for (int i = tid; i < 4 * NB; i += NT) s_h[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const uint32_t p0 = hdr->sel[LEVEL - 1][c].prefix[0], p1 = hdr->sel[LEVEL - 1][c].prefix[1];
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int p = blockIdx.x * PXB + k * NT + tid;
            if (p >= HW) continue;
            const uint32_t key = keys[(size_t)c * HW + p], pre = mt_prefix(key, LEVEL), dg = mt_digit(key, LEVEL);
            if (pre == p0) atomicAdd(&s_h[(2 * c) * NB + dg], 1u);
            if (pre == p1) atomicAdd(&s_h[(2 * c + 1) * NB + dg], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i < 4 * NB; i += NT) {
        const uint32_t v = s_h[i];
        if (v) atomicAdd(&hist[i], v);
    }
}

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(NT) void k_mt_ssim(MtIn a, int ntx, int nT, const MtHdr* __restrict__ hdr, double* __restrict__ partials)
{
    __shared__ float s_x[SIY][SIX], s_y[SIY][SIX];
    __shared__ double s_row[5][SIY][STX];
    __shared__ double s_d[NW];
    const int tid = threadIdx.x, tile = blockIdx.x, ty = tile / ntx, tx = tile - ty * ntx;
    const int y0 = ty * STY, x0 = tx * STX;                          // the tile's first output pixel = its first input pixel (the window starts there)
    const int OH = a.H - (MT_WIN - 1), OW = a.W - (MT_WIN - 1);
    for (int c = 0; c < 2; c++) {
        __syncthreads();                                               // the previous image's row sums are read out
        for (int i = tid; i < SIY * SIX; i += NT) {
            const int r = i / SIX, q = i - r * SIX, yy = y0 + r, xx = x0 + q;
            float x = 0.f, y = 0.f;
            if (yy < a.H && xx < a.W) mt_pair(a, c, yy * a.W + xx, x, y);
            s_x[r][q] = x; s_y[r][q] = y;
        }
        __syncthreads();
        for (int i = tid; i < SIY * STX; i += NT) {                    // the five 7-tap row sums, left to right
            const int r = i / STX, q = i - r * STX;
            double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
            for (int t = 0; t < MT_WIN; t++) {
                const double x = (double)s_x[r][q + t], y = (double)s_y[r][q + t];
                sx += x; sy += y; sxx += x * x; syy += y * y; sxy += x * y;
            }
            s_row[0][r][q] = sx; s_row[1][r][q] = sy; s_row[2][r][q] = sxx; s_row[3][r][q] = syy; s_row[4][r][q] = sxy;
        }
        __syncthreads();
        const double R = hdr->R[c];
        double acc = 0;
        for (int i = tid; i < STY * STX; i += NT) {                    // the 7 rows, top to bottom, in registers
            const int r = i / STX, q = i - r * STX;
            if (y0 + r >= OH || x0 + q >= OW) continue;
            double s[5];
#pragma unroll
            for (int m = 0; m < 5; m++) {
                double v = 0;
#pragma unroll
                for (int t = 0; t < MT_WIN; t++) v += s_row[m][r + t][q];
                s[m] = v;
            }
            acc += mt_ssim_window(s, R);
        }
        const double t = block_sum(acc, s_d);
        if (tid == 0) partials[(size_t)c * nT + tile] = t;
    }
}

// ---- points ----------------------------------------------------------------------------------------------------------------------------------------
// pp[blk][2] = sum dist_a over gt_hit, sum dist_b over `mask`; pc[blk][2] = how many of each lie below the threshold
__global__ __launch_bounds__(NT) void k_mt_points(MtIn a, const float* __restrict__ dist_a, const float* __restrict__ dist_b, float thr,
                                                  double* __restrict__ pp, int* __restrict__ pc)
{
    __shared__ double s_d[NW];
    __shared__ int s_n[NW];
    const int tid = threadIdx.x, blk = blockIdx.x;
    double sa = 0, sb = 0;
    bool ba[2] = {false, false}, bb[2] = {false, false};
#pragma unroll
    for (int k = 0; k < 2; k++) {
        const int p = blk * PXB + k * NT + tid;
        if (p >= a.HW) continue;
        const bool ghit = a.gm[p] != 0, m = a.use_gt ? ghit : mt_pred_hit(a, p);
        if (ghit) { const float d = dist_a[p]; sa += (double)d; ba[k] = d < thr; }
        if (m) { const float d = dist_b[p]; sb += (double)d; bb[k] = d < thr; }
    }
    const double ta = block_sum(sa, s_d), tb = block_sum(sb, s_d);
    const int ca = block_count(ba[0], ba[1], s_n), cb = block_count(bb[0], bb[1], s_n);
    if (tid == 0) { pp[blk * 2] = ta; pp[blk * 2 + 1] = tb; pc[blk * 2] = ca; pc[blk * 2 + 1] = cb; }
}

__global__ __launch_bounds__(NT) void k_mt_fin(int nT, int nblk, int OH, int OW, int with_points, const MtHdr* __restrict__ hdr,
                                               const double* __restrict__ tiles, const double* __restrict__ pp, const int* __restrict__ pc,
                                               const int* __restrict__ counts, float* __restrict__ out)
{
    __shared__ double s_d[NW];
    const int tid = threadIdx.x;
    double s[2] = {0, 0};
    for (int r = tid; r < nT; r += NT) { s[0] += tiles[r]; s[1] += tiles[(size_t)nT + r]; }
    const double S0 = block_sum(s[0], s_d), S1 = block_sum(s[1], s_d);
    double d[2] = {0, 0};
    long long n[2] = {0, 0};
    if (with_points)
        for (int r = tid; r < nblk; r += NT) { d[0] += pp[r * 2]; d[1] += pp[r * 2 + 1]; n[0] += pc[r * 2]; n[1] += pc[r * 2 + 1]; }
    const double DA = block_sum(d[0], s_d), DB = block_sum(d[1], s_d), CA = block_sum((double)n[0], s_d), CB = block_sum((double)n[1], s_d);
    if (tid == 0) {
        const double nwin = (double)OH * (double)OW, nan = __longlong_as_double(0x7ff8000000000000LL);
        out[LRT_METRICS_DEPTH_SSIM] = (float)(hdr->R[0] == 0.0 ? nan : S0 / nwin);
        out[LRT_METRICS_INTENSITY_SSIM] = (float)(hdr->R[1] == 0.0 ? nan : S1 / nwin);
        const double n_pred = (double)counts[0], n_gt = (double)counts[1];
        if (!with_points) { out[LRT_METRICS_POINTS_CHAMFER_DIST] = (float)nan; out[LRT_METRICS_POINTS_FSCORE] = (float)nan; }
        else {
            out[LRT_METRICS_POINTS_CHAMFER_DIST] = (float)(n_pred > 0 && n_gt > 0 ? DA / n_gt + DB / n_pred : nan);
            out[LRT_METRICS_POINTS_FSCORE] = (float)mt_fscore(CA, n_gt, CB, n_pred);
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define MT_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline bool size_ok(int H, int W) { return H >= MT_WIN && W >= MT_WIN && W <= (1 << 20) && (size_t)H * W <= ((size_t)1 << 27); }
static inline size_t up16(size_t n) { return (n + 15) / 16 * 16; }

struct Layout {
    int HW, nblk, ntx, nT;
    size_t hist1, hist2, hist3, zero_bytes;                    // contiguous from offset 0: one memset
    size_t hdr, counts, keys, pd, pf, pn, tiles, pp, pc, total;
};

static Layout layout(int H, int W)
{
    Layout L;
    L.HW = H * W; L.nblk = (L.HW + PXB - 1) / PXB;
    L.ntx = (W - (MT_WIN - 1) + STX - 1) / STX; L.nT = L.ntx * ((H - (MT_WIN - 1) + STY - 1) / STY);
    size_t o = 0;
    L.hist1 = o; o += 2 * MT_L1_BINS * sizeof(uint32_t);
    L.hist2 = o; o += 4 * MT_L2_BINS * sizeof(uint32_t);
    L.hist3 = o; o += 4 * MT_L3_BINS * sizeof(uint32_t);
    L.zero_bytes = o;
    L.hdr = o; o += up16(sizeof(MtHdr));
    L.counts = o; o += 16;
    L.keys = o; o += up16(2 * (size_t)L.HW * sizeof(uint32_t));
    L.pd = o; o += up16((size_t)L.nblk * 4 * sizeof(double));
    L.pf = o; o += up16((size_t)L.nblk * 4 * sizeof(float));
    L.pn = o; o += up16((size_t)L.nblk * 6 * sizeof(int));
    L.tiles = o; o += up16(2 * (size_t)L.nT * sizeof(double));
    L.pp = o; o += up16((size_t)L.nblk * 2 * sizeof(double));
    L.pc = o; o += up16((size_t)L.nblk * 2 * sizeof(int));
    L.total = o;
    return L;
}

extern "C" {

int lrt_metrics_abi_version(void) { return LRT_METRICS_ABI_VERSION; }

const char* lrt_metrics_last_error(void) { return g_err; }

size_t lrt_metrics_work_bytes(int H, int W)
{
    if (!size_ok(H, W)) return 0;
    return layout(H, W).total;
}

int lrt_metrics_frame(int device, int H, int W, const float* pred_depth, const float* pred_intensity, const float* pred_raydrop,
                      const float* gt_depth, const float* gt_intensity, const uint8_t* gt_mask, const float* dist_a, const float* dist_b,
                      double raydrop_ratio, int use_gt_mask, double max_depth, double fscore_threshold, float* out, void* work,
                      size_t work_bytes, void* stream_)
{
    const char* fn = "lrt_metrics_frame";
    // the arguments first, the device after them: a bad call is refused on a machine without one, too
    if (!size_ok(H, W)) MT_FAIL(LRT_ERR_ARG, "%s: unsupported image size %d x %d (a 7 x 7 SSIM window must fit)", fn, H, W);
    if (!pred_depth || !pred_intensity || !pred_raydrop || !gt_depth || !gt_intensity || !gt_mask) MT_FAIL(LRT_ERR_ARG, "%s: null image / mask pointer", fn);
    if ((dist_a == nullptr) != (dist_b == nullptr)) MT_FAIL(LRT_ERR_ARG, "%s: dist_a and dist_b go together (both or neither)", fn);
    if (!out) MT_FAIL(LRT_ERR_ARG, "%s: null output pointer", fn);
    if (!(raydrop_ratio == raydrop_ratio) || !(max_depth == max_depth) || !(fscore_threshold == fscore_threshold))
        MT_FAIL(LRT_ERR_ARG, "%s: raydrop_ratio, max_depth or fscore_threshold is NaN", fn);
    if (!work || work_bytes < lrt_metrics_work_bytes(H, W)) MT_FAIL(LRT_ERR_ARG, "%s: workspace of %zu bytes, need %zu", fn, work_bytes, lrt_metrics_work_bytes(H, W));
    if (((uintptr_t)work & 15) != 0) MT_FAIL(LRT_ERR_ARG, "%s: the workspace must be 16-byte aligned", fn);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) MT_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) MT_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const Layout L = layout(H, W);
    MtIn a;
    a.H = H; a.W = W; a.HW = L.HW; a.use_gt = use_gt_mask ? 1 : 0;
    a.pd = pred_depth; a.pi = pred_intensity; a.pr = pred_raydrop; a.gd = gt_depth; a.gi = gt_intensity; a.gm = gt_mask;
    a.ratio = (float)raydrop_ratio; a.max_depth = (float)max_depth;
    char* w = (char*)work;
    uint32_t *hist1 = (uint32_t*)(w + L.hist1), *hist2 = (uint32_t*)(w + L.hist2), *hist3 = (uint32_t*)(w + L.hist3), *keys = (uint32_t*)(w + L.keys);
    MtHdr* hdr = (MtHdr*)(w + L.hdr);
    int *counts = (int*)(w + L.counts), *pn = (int*)(w + L.pn), *pc = (int*)(w + L.pc);
    double *pd = (double*)(w + L.pd), *tiles = (double*)(w + L.tiles), *pp = (double*)(w + L.pp);
    float* pf = (float*)(w + L.pf);
    const int with_points = dist_a != nullptr;
    if (hipMemsetAsync(w, 0, L.zero_bytes, stream) != hipSuccess) MT_FAIL(LRT_ERR_HIP, "%s: hipMemsetAsync failed", fn);
    hipLaunchKernelGGL(k_mt_pass1, dim3(L.nblk), dim3(NT), 0, stream, a, keys, hist1, pd, pf, pn);
    hipLaunchKernelGGL(k_mt_reduce1, dim3(1), dim3(NT), 0, stream, L.nblk, L.HW, max_depth, (const double*)pd, (const float*)pf, (const int*)pn, hdr, counts, out);
    hipLaunchKernelGGL(k_mt_scan<1>, dim3(1), dim3(NT), 0, stream, L.HW, (const uint32_t*)hist1, hdr, out);
    hipLaunchKernelGGL(k_mt_hist<2>, dim3(L.nblk), dim3(NT), 0, stream, L.HW, (const uint32_t*)keys, (const MtHdr*)hdr, hist2);
    hipLaunchKernelGGL(k_mt_scan<2>, dim3(1), dim3(NT), 0, stream, L.HW, (const uint32_t*)hist2, hdr, out);
    hipLaunchKernelGGL(k_mt_hist<3>, dim3(L.nblk), dim3(NT), 0, stream, L.HW, (const uint32_t*)keys, (const MtHdr*)hdr, hist3);
    hipLaunchKernelGGL(k_mt_scan<3>, dim3(1), dim3(NT), 0, stream, L.HW, (const uint32_t*)hist3, hdr, out);
    hipLaunchKernelGGL(k_mt_ssim, dim3(L.nT), dim3(NT), 0, stream, a, L.ntx, L.nT, (const MtHdr*)hdr, tiles);
    if (with_points)
        hipLaunchKernelGGL(k_mt_points, dim3(L.nblk), dim3(NT), 0, stream, a, dist_a, dist_b, (float)fscore_threshold, pp, pc);
    hipLaunchKernelGGL(k_mt_fin, dim3(1), dim3(NT), 0, stream, L.nT, L.nblk, H - (MT_WIN - 1), W - (MT_WIN - 1), with_points, (const MtHdr*)hdr,
                       (const double*)tiles, (const double*)pp, (const int*)pc, (const int*)counts, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) MT_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
