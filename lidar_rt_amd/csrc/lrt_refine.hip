// lrt_refine.hip -- inference of the ray-drop refinement network (include/lrt_refine.h), gfx950.  Compiled into liblrt_refine.so, a library of
// its own.  No allocation, no host wait, no atomics; every intermediate is channels-last (pixel, channel) float32 in the caller's workspace.
//
//   k_rf_in                   one thread per (pixel, output channel): the 1x1 convolution of the 3 or 9 input planes, read where the renderer
//                             left them (a plane is a pointer and a pixel stride; the rays are (H, W, 3)).
//   k_rf_conv<SRC, TAPS, NT, KS>  the convolutions as implicit GEMMs, pixels x C_out over K = TAPS C_in, on v_mfma_f32_32x32x2_f32 (exact float32:
//                             each output is ONE fma chain in k order).  A wave owns 32 pixels x 32 NT output channels; a workgroup is four
//                             waves on four pixel tiles (KS = 1) or, on the coarse levels, on the four quarters of one tile's K, added in wave
//                             order through LDS (KS = 4: four chains per output, one fixed order).  In a step of 8 input channels lane (r, h) gathers channels c0 + 4 h .. + 3 of pixel r
//                             with one 16-byte load and feeds them to four MFMAs (k pairs (c0 + j, c0 + 4 + j)); the weights are K-major, so a
//                             half-wave reads 128 contiguous bytes of a weight row.  The gather does the source mapping:
//                               SRC_SAME  the level's own tensor
//                               SRC_POOL  the maximum of the 2 x 2 block of the finer level
//                               SRC_UP    channel < C_skip: the skip; else the bilinear sample of the coarser level at the padded position, and
//                                         the raw value 0 where the padding of the up path lies
//                             then the folded affine and the ReLU; a tap outside the image contributes 0 AFTER them.  TAPS = 1 is the 1x1
//                             convolution of the attention block (affine without ReLU for q, k, v; none, plus the residual, for the projection).
//   k_rf_attn                 one wave per (query token, head): the scores of the query against every key into LDS, their maximum, the
//                             exponentials and their sum, then the value product, lane j summing channel j over the keys in key order.  The
//                             result goes to (head, token, d) -- and the projection reads that memory as (token, channel), as the reference does.
//   k_rf_out                  one thread per pixel: affine, ReLU, the dot with the c output weights in channel order, bias, sigmoid.
//
// Bounds: every gather is guarded by the size of the level it reads; a lane beyond the last pixel or the last output channel loads nothing
// (its operand is 0) and stores nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_refine_math.h"
#include "../../include/lrt_refine.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int RF_BLOCK = 256;
constexpr int RF_WAVES = RF_BLOCK / 64;
enum { SRC_SAME = 0, SRC_POOL = 1, SRC_UP = 2 };

struct ConvArgs {
    int H, W;                        // the grid of the output (and of the taps)
    int Cin, Cout;
    const float *a, *b;              // folded affine over Cin; a == nullptr: none
    const float* w;                  // (TAPS Cin, Cout)
    const float* src;                // SAME: (H W, Cin); POOL: the finer level (Hs Ws, Cin); UP: the skip (H W, Cskip)
    const float* src2;               // UP: the coarser level (Hs Ws, Cin - Cskip)
    const float* res;                // added to the result, (H W, Cout), or nullptr
    float* dst;                      // (H W, Cout)
    int Hs, Ws;                      // POOL: the finer level's size; UP: the coarser level's
    int Cskip, padT, padL;           // UP
    float sy, sx;                    // UP: rf_up_scale of the coarser level's height and width
    int relu;
};

__device__ inline float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ inline float4 max4(float4 x, float4 y) { return make_float4(fmaxf(x.x, y.x), fmaxf(x.y, y.y), fmaxf(x.z, y.z), fmaxf(x.w, y.w)); }
__device__ inline float4 lerp4(float4 x, float4 y, float t)
{
    const float s = 1.0f - t;
    return make_float4(s * x.x + t * y.x, s * x.y + t * y.y, s * x.z + t * y.z, s * x.w + t * y.w);
}

// Channels ci .. ci + 3 of the (virtual) input tensor at pixel (qy, qx) of the output grid, BEFORE the affine.  (qy, qx) is inside the grid.
template <int SRC>
__device__ inline float4 rf_gather(const ConvArgs& g, int qy, int qx, int ci)
{
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (SRC == SRC_SAME) {
        return ld4(g.src + ((long long)qy * g.W + qx) * g.Cin + ci);
    } else if (SRC == SRC_POOL) {
        const int y0 = 2 * qy, x0 = 2 * qx;
        if (y0 + 1 >= g.Hs || x0 + 1 >= g.Ws) return zero;              // cannot happen for H = Hs >> 1, W = Ws >> 1: the guard of the finer level
        const float* p = g.src + ((long long)y0 * g.Ws + x0) * g.Cin + ci;
        const long long row = (long long)g.Ws * g.Cin;
        return max4(max4(ld4(p), ld4(p + g.Cin)), max4(ld4(p + row), ld4(p + row + g.Cin)));
    } else {
        if (ci < g.Cskip) return ld4(g.src + ((long long)qy * g.W + qx) * g.Cskip + ci);
        const int uy = qy - g.padT, ux = qx - g.padL;
        if (uy < 0 || uy >= 2 * g.Hs || ux < 0 || ux >= 2 * g.Ws) return zero;                // the padding of the up path
        int y0, y1, x0, x1;
        float fy, fx;
        rf_up_coord(uy, g.sy, g.Hs, &y0, &y1, &fy);
        rf_up_coord(ux, g.sx, g.Ws, &x0, &x1, &fx);
        const int C2 = g.Cin - g.Cskip, cu = ci - g.Cskip;
        const float* r0 = g.src2 + (long long)y0 * g.Ws * C2 + cu;
        const float* r1 = g.src2 + (long long)y1 * g.Ws * C2 + cu;
        const float4 top = lerp4(ld4(r0 + (long long)x0 * C2), ld4(r0 + (long long)x1 * C2), fx);
        const float4 bot = lerp4(ld4(r1 + (long long)x0 * C2), ld4(r1 + (long long)x1 * C2), fx);
        return lerp4(top, bot, fy);
    }
}

// U groups of 8 input channels of one tap, from channel c0: every load of the step (the gathers, the affines, 4 U NT weights) is issued before
// its first MFMA, so a wave has U times as many bytes in flight.  The fma chain runs over the channels in ascending groups of 8 whatever U is.
template <int SRC, int NT, int U>
__device__ inline void rf_step(const ConvArgs& g, bool inside, int qy, int qx, int tap, int c0, int h, int r, int n0, const bool* col_ok, f32x16* acc)
{
    float4 v[U];
    float bv[U][4][NT];
#pragma unroll
    for (int u = 0; u < U; u++) {
        const int ci = c0 + 8 * u + 4 * h;                             // the range is a multiple of 8 channels: ci + 3 lies inside it
        v[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (inside) {
            v[u] = rf_gather<SRC>(g, qy, qx, ci);
            if (g.a) {
                const float4 a = ld4(g.a + ci), b = ld4(g.b + ci);
                v[u] = make_float4(fmaf(a.x, v[u].x, b.x), fmaf(a.y, v[u].y, b.y), fmaf(a.z, v[u].z, b.z), fmaf(a.w, v[u].w, b.w));
            }
            if (g.relu) v[u] = make_float4(fmaxf(v[u].x, 0.0f), fmaxf(v[u].y, 0.0f), fmaxf(v[u].z, 0.0f), fmaxf(v[u].w, 0.0f));
        }
        const float* wrow = g.w + ((long long)tap * g.Cin + ci) * g.Cout + n0 + r;
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int t = 0; t < NT; t++) bv[u][j][t] = col_ok[t] ? wrow[(long long)j * g.Cout + 32 * t] : 0.0f;
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
        const float av[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int t = 0; t < NT; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[u][j][t], acc[t], 0, 0, 0);
    }
}

// KS = 1: the four waves of a workgroup own four pixel tiles.  KS = 4 (the coarse levels, which have few tiles and long K): the four waves
// share ONE pixel tile, wave w sums channels [w Cin / 4, (w + 1) Cin / 4) of every tap, and wave 0 adds the four partial tiles in wave order.
template <int SRC, int TAPS, int NT, int KS>
__global__ __launch_bounds__(RF_BLOCK) void k_rf_conv(ConvArgs g)
{
    static_assert(KS == 1 || (KS == RF_WAVES && NT == 1), "the split is over the workgroup's waves");
    __shared__ float s_red[KS > 1 ? (KS - 1) * 16 * 64 : 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 31, h = lane >> 5;
    const long long n_pix = (long long)g.H * g.W;
    const long long tile = KS > 1 ? (long long)blockIdx.x : (long long)blockIdx.x * RF_WAVES + wave;
    if (tile * 32 >= n_pix) return;                                    // KS = 1: whole waves leave before any barrier; KS > 1: the whole workgroup (never: the grid is exact)
    const int n0 = blockIdx.y * (32 * NT);
    const long long p = tile * 32 + r;
    const bool live = p < n_pix;
    const int py = live ? (int)(p / g.W) : 0, px = live ? (int)(p - (long long)py * g.W) : 0;
    const int c_per = g.Cin / KS, c_begin = KS > 1 ? wave * c_per : 0, c_end = c_begin + c_per;     // KS > 1: Cin is a multiple of 8 KS

    f32x16 acc[NT];
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
        for (int i = 0; i < 16; i++) acc[t][i] = 0.0f;
    bool col_ok[NT];
#pragma unroll
    for (int t = 0; t < NT; t++) col_ok[t] = n0 + 32 * t + r < g.Cout;

    for (int tap = 0; tap < TAPS; tap++) {
        const int qy = py + (TAPS == 9 ? tap / 3 - 1 : 0), qx = px + (TAPS == 9 ? tap % 3 - 1 : 0);
        const bool inside = live && qy >= 0 && qy < g.H && qx >= 0 && qx < g.W;
        int c0 = c_begin;
        for (; c0 + 32 <= c_end; c0 += 32) rf_step<SRC, NT, 4>(g, inside, qy, qx, tap, c0, h, r, n0, col_ok, acc);
        for (; c0 < c_end; c0 += 8) rf_step<SRC, NT, 1>(g, inside, qy, qx, tap, c0, h, r, n0, col_ok, acc);
    }
    if (KS > 1) {
        if (wave > 0) {
#pragma unroll
            for (int i = 0; i < 16; i++) s_red[((wave - 1) * 16 + i) * 64 + lane] = acc[0][i];
        }
        __syncthreads();
        if (wave > 0) return;
#pragma unroll
        for (int w = 0; w < KS - 1; w++)
#pragma unroll
            for (int i = 0; i < 16; i++) acc[0][i] += s_red[(w * 16 + i) * 64 + lane];
    }
    // C/D of the 32x32 MFMA: column = lane & 31, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int t = 0; t < NT; t++) {
        if (!col_ok[t]) continue;
        const int n = n0 + 32 * t + r;
#pragma unroll
        for (int i = 0; i < 16; i++) {
            const long long q = tile * 32 + (i & 3) + 8 * (i >> 2) + 4 * h;
            if (q < n_pix) {
                float o = acc[t][i];
                if (g.res) o = g.res[q * g.Cout + n] + o;
                g.dst[q * g.Cout + n] = o;
            }
        }
    }
}

struct InArgs {
    long long n_pix;
    int Cin, C;
    const float *raydrop, *intensity, *depth, *ray_o, *ray_d;
    int sp, si, sd;
    const float *w, *bias;
    float* dst;
};

__global__ __launch_bounds__(RF_BLOCK) void k_rf_in(InArgs g)
{
    const long long e = (long long)blockIdx.x * RF_BLOCK + threadIdx.x;
    if (e >= g.n_pix * g.C) return;
    const long long p = e / g.C;
    const int co = (int)(e - p * g.C);
    float acc = g.bias[co];
    acc = fmaf(g.w[co], g.raydrop[p * g.sp], acc);
    acc = fmaf(g.w[g.C + co], g.intensity[p * g.si], acc);
    acc = fmaf(g.w[2 * g.C + co], g.depth[p * g.sd], acc);
    if (g.Cin == 9) {
#pragma unroll
        for (int i = 0; i < 3; i++) acc = fmaf(g.w[(3 + i) * g.C + co], g.ray_o[3 * p + i], acc);
#pragma unroll
        for (int i = 0; i < 3; i++) acc = fmaf(g.w[(6 + i) * g.C + co], g.ray_d[3 * p + i], acc);
    }
    g.dst[e] = acc;
}

// qkv (T, 3 C): q at channel hd d + j, k at C + hd d + j, v at 2 C + hd d + j.  hb (heads, T, d).
__global__ __launch_bounds__(64) void k_rf_attn(int T, int C, float scale, const float* __restrict__ qkv, float* __restrict__ hb)
{
    __shared__ float s_p[LRT_REFINE_MAX_TOKENS];
    const int lane = threadIdx.x, t = blockIdx.x, hd = blockIdx.y;
    const int d = C / LRT_REFINE_HEADS;                                // a multiple of 8
    const float* q = qkv + (long long)t * 3 * C + hd * d;
    float m = -INFINITY;
    for (int s = lane; s < T; s += 64) {
        const float* k = qkv + (long long)s * 3 * C + C + hd * d;
        float dot = 0.0f;
        for (int j = 0; j < d; j += 4) {
            const float4 a = ld4(q + j), b = ld4(k + j);
            dot = fmaf(a.x, b.x, dot); dot = fmaf(a.y, b.y, dot); dot = fmaf(a.z, b.z, dot); dot = fmaf(a.w, b.w, dot);
        }
        dot *= scale;
        s_p[s] = dot;
        m = fmaxf(m, dot);
    }
    for (int k = 32; k >= 1; k >>= 1) m = fmaxf(m, __shfl_xor(m, k));
    float sum = 0.0f;
    for (int s = lane; s < T; s += 64) {                                // each lane rereads what it wrote itself
        const float e = expf(s_p[s] - m);
        s_p[s] = e;
        sum += e;
    }
    for (int k = 32; k >= 1; k >>= 1) sum += __shfl_xor(sum, k);        // a butterfly: the same order on every run
    __syncthreads();
    const float inv = 1.0f / sum;
    for (int j = lane; j < d; j += 64) {
        const float* v = qkv + 2 * C + hd * d + j;
        float acc = 0.0f;
        for (int s = 0; s < T; s++) acc = fmaf(s_p[s], v[(long long)s * 3 * C], acc);
        hb[((long long)hd * T + t) * d + j] = acc * inv;
    }
}

__global__ __launch_bounds__(RF_BLOCK) void k_rf_out(long long n_pix, int C, const float* __restrict__ y, const float* __restrict__ a, const float* __restrict__ b,
                                                     const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ prob, float* __restrict__ logits)
{
    const long long p = (long long)blockIdx.x * RF_BLOCK + threadIdx.x;
    if (p >= n_pix) return;
    const float* row = y + p * C;
    float z = 0.0f;
    for (int c = 0; c < C; c += 4) {
        const float4 x = ld4(row + c), aa = ld4(a + c), bb = ld4(b + c), ww = ld4(w + c);
        z = fmaf(ww.x, fmaxf(fmaf(aa.x, x.x, bb.x), 0.0f), z);
        z = fmaf(ww.y, fmaxf(fmaf(aa.y, x.y, bb.y), 0.0f), z);
        z = fmaf(ww.z, fmaxf(fmaf(aa.z, x.z, bb.z), 0.0f), z);
        z = fmaf(ww.w, fmaxf(fmaf(aa.w, x.w, bb.w), 0.0f), z);
    }
    z += bias[0];
    if (logits) logits[p] = z;
    prob[p] = 1.0f / (1.0f + expf(-z));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define RF_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static int check_shape(const char* fn, int H, int W, int Cin, int c)
{
    if (Cin != 3 && Cin != 9) RF_FAIL(LRT_ERR_ARG, "%s: %d input channels (3 or 9)", fn, Cin);
    if (c < 8 || c > LRT_REFINE_MAX_CHANNELS || c % 8 != 0) RF_FAIL(LRT_ERR_ARG, "%s: channels %d (a multiple of 8, 8 .. %d)", fn, c, LRT_REFINE_MAX_CHANNELS);
    if (H < 16 || W < 16) RF_FAIL(LRT_ERR_ARG, "%s: a frame of %d x %d (at least 16 x 16: the coarsest level is (H >> 4) x (W >> 4))", fn, H, W);
    if ((long long)H * W > LRT_REFINE_MAX_PIXELS) RF_FAIL(LRT_ERR_ARG, "%s: a frame of %d x %d, more than %d pixels", fn, H, W, LRT_REFINE_MAX_PIXELS);
    const long long T = (long long)(H >> 4) * (W >> 4);
    if (T > LRT_REFINE_MAX_TOKENS)
        RF_FAIL(LRT_ERR_ARG, "%s: a frame of %d x %d has %lld tokens at the attention block, more than %d (nothing is truncated: the call is refused)", fn, H, W, T,
                LRT_REFINE_MAX_TOKENS);
    return LRT_OK;
}

template <int SRC, int TAPS>
static hipError_t launch_conv(const ConvArgs& g, hipStream_t stream)
{
    const long long m_tiles = ((long long)g.H * g.W + 31) / 32;
    const int n_tiles = (g.Cout + 31) / 32;
    const long long waves = m_tiles * n_tiles;                          // with one 32 x 32 tile per wave
    // tiles per level, not one shape for all: a coarse level has few tiles and a long K, so its waves split K four ways; a fine level has
    // tiles to spare, so a wave takes two column tiles and uses each gathered operand twice
    if (waves <= 2048 && g.Cin % (8 * RF_WAVES) == 0)
        hipLaunchKernelGGL((k_rf_conv<SRC, TAPS, 1, RF_WAVES>), dim3((unsigned)m_tiles, (unsigned)n_tiles), dim3(RF_BLOCK), 0, stream, g);
    else if (n_tiles % 2 == 0 && waves / 2 >= 4096)
        hipLaunchKernelGGL((k_rf_conv<SRC, TAPS, 2, 1>), dim3((unsigned)((m_tiles + RF_WAVES - 1) / RF_WAVES), (unsigned)(n_tiles / 2)), dim3(RF_BLOCK), 0, stream, g);
    else
        hipLaunchKernelGGL((k_rf_conv<SRC, TAPS, 1, 1>), dim3((unsigned)((m_tiles + RF_WAVES - 1) / RF_WAVES), (unsigned)n_tiles), dim3(RF_BLOCK), 0, stream, g);
    return hipGetLastError();
}

extern "C" {

int lrt_refine_abi_version(void) { return LRT_REFINE_ABI_VERSION; }

const char* lrt_refine_last_error(void) { return g_err; }

long long lrt_refine_param_count(int Cin, int channels)
{
    if (check_shape("lrt_refine_param_count", 16, 16, Cin, channels) != LRT_OK) return -1;
    return rf_param_count(Cin, channels);
}

long long lrt_refine_work_bytes(int H, int W, int Cin, int channels)
{
    if (check_shape("lrt_refine_work_bytes", H, W, Cin, channels) != LRT_OK) return -1;
    RfPlan pl;
    rf_plan(H, W, channels, &pl);
    return pl.off[RF_NBUF] * 4;
}

int lrt_refine_forward(int device, int H, int W, int Cin, int channels, const float* params, long long n_params,
                       const float* raydrop, const float* intensity, const float* depth, int stride_raydrop, int stride_intensity, int stride_depth,
                       const float* ray_o, const float* ray_d, float* prob, float* logits, void* workspace, long long work_bytes, void* stream_)
{
    const char* fn = "lrt_refine_forward";
    const int rc = check_shape(fn, H, W, Cin, channels);
    if (rc != LRT_OK) return rc;
    const int c = channels;
    RfPlan pl;
    rf_plan(H, W, c, &pl);
    const long long need = pl.off[RF_NBUF] * 4;
    if (!params || n_params != rf_param_count(Cin, c)) RF_FAIL(LRT_ERR_ARG, "%s: %lld parameters, a network of %d inputs and %d channels has %lld", fn, n_params, Cin, c, rf_param_count(Cin, c));
    if (((uintptr_t)params & 15)) RF_FAIL(LRT_ERR_ARG, "%s: params must be 16-byte aligned", fn);
    if (!raydrop || !intensity || !depth || !prob) RF_FAIL(LRT_ERR_ARG, "%s: null raydrop / intensity / depth / prob pointer", fn);
    if (stride_raydrop < 1 || stride_intensity < 1 || stride_depth < 1) RF_FAIL(LRT_ERR_ARG, "%s: a pixel stride below 1", fn);
    if ((Cin == 9) != (ray_o != nullptr && ray_d != nullptr) || (Cin == 3 && (ray_o || ray_d)))
        RF_FAIL(LRT_ERR_ARG, "%s: %d input channels %s ray_o and ray_d", fn, Cin, Cin == 9 ? "need" : "take no");
    if (!workspace || ((uintptr_t)workspace & 255)) RF_FAIL(LRT_ERR_ARG, "%s: the workspace must be 256-byte aligned device memory", fn);
    if (work_bytes < need) RF_FAIL(LRT_ERR_ARG, "%s: a workspace of %lld bytes, a frame of %d x %d needs %lld", fn, work_bytes, H, W, need);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) RF_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) RF_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    float* ws = (float*)workspace;
    auto buf = [&](int b) { return ws + pl.off[b]; };
    hipError_t e;

    // the input convolution
    const float* par = params;
    InArgs ia;
    ia.n_pix = pl.n[0]; ia.Cin = Cin; ia.C = c;
    ia.raydrop = raydrop; ia.intensity = intensity; ia.depth = depth; ia.ray_o = ray_o; ia.ray_d = ray_d;
    ia.sp = stride_raydrop; ia.si = stride_intensity; ia.sd = stride_depth;
    ia.w = par; ia.bias = par + (long long)Cin * c; ia.dst = buf(RF_X0);
    par += (long long)Cin * c + c;
    hipLaunchKernelGGL(k_rf_in, dim3((unsigned)((pl.n[0] * c + RF_BLOCK - 1) / RF_BLOCK)), dim3(RF_BLOCK), 0, stream, ia);
    if ((e = hipGetLastError()) != hipSuccess) RF_FAIL(LRT_ERR_HIP, "%s: launch of the input convolution failed: %s", fn, hipGetErrorString(e));

    const int mid_of[RF_PAIRS] = {RF_M1, RF_M2, RF_M3, RF_M4, RF_U3M, RF_U2M, RF_U1M, RF_U0M};
    const int out_of[RF_PAIRS] = {RF_X1, RF_X2, RF_X3, RF_X4, RF_Y3, RF_Y2, RF_Y1, RF_Y0};
    const int skip_of[RF_PAIRS] = {-1, -1, -1, -1, RF_X3, RF_X2, RF_X1, RF_X0};
    const float* prev = buf(RF_X0);                                    // what the next pair reads: the finer level going down, the coarser going up
    for (int i = 0; i < RF_PAIRS; i++) {
        if (i == 4) {
            // the attention block on x4: q, k, v; the value product in (head, token, d); the projection of that memory read as (token, channel)
            const int C8 = 8 * c, T = (int)pl.n[4];
            ConvArgs g = {};
            g.H = pl.H[4]; g.W = pl.W[4]; g.Cin = C8; g.Cout = 3 * C8; g.a = par; g.b = par + C8; g.w = par + 2 * C8;
            g.src = buf(RF_X4); g.dst = buf(RF_QKV); g.relu = 0;
            if ((e = launch_conv<SRC_SAME, 1>(g, stream)) != hipSuccess) RF_FAIL(LRT_ERR_HIP, "%s: launch of the q, k, v projection failed: %s", fn, hipGetErrorString(e));
            const int d = C8 / LRT_REFINE_HEADS;
            hipLaunchKernelGGL(k_rf_attn, dim3((unsigned)T, LRT_REFINE_HEADS), dim3(64), 0, stream, T, C8, (float)(1.0 / sqrt((double)d)), (const float*)buf(RF_QKV), buf(RF_HB));
            if ((e = hipGetLastError()) != hipSuccess) RF_FAIL(LRT_ERR_HIP, "%s: launch of the attention failed: %s", fn, hipGetErrorString(e));
            ConvArgs pj = {};
            pj.H = pl.H[4]; pj.W = pl.W[4]; pj.Cin = C8; pj.Cout = C8; pj.a = nullptr; pj.b = nullptr; pj.w = par + 2 * C8 + (long long)C8 * 3 * C8;
            pj.src = buf(RF_HB); pj.res = buf(RF_X4); pj.dst = buf(RF_X4A); pj.relu = 0;
            if ((e = launch_conv<SRC_SAME, 1>(pj, stream)) != hipSuccess) RF_FAIL(LRT_ERR_HIP, "%s: launch of the attention's projection failed: %s", fn, hipGetErrorString(e));
            par += 2 * C8 + (long long)C8 * 3 * C8 + (long long)C8 * C8;
            prev = buf(RF_X4A);
        }
        int ci, cm, co, lvl;
        rf_pair_channels(i, c, &ci, &cm, &co, &lvl);
        ConvArgs g = {};
        g.H = pl.H[lvl]; g.W = pl.W[lvl]; g.Cin = ci; g.Cout = cm; g.a = par; g.b = par + ci; g.w = par + 2 * ci;
        g.dst = buf(mid_of[i]); g.relu = 1;
        if (i < 4) {
            g.src = prev; g.Hs = pl.H[lvl - 1]; g.Ws = pl.W[lvl - 1];
            e = launch_conv<SRC_POOL, 9>(g, stream);
        } else {
            g.src = buf(skip_of[i]); g.src2 = prev; g.Cskip = ci / 2; g.Hs = pl.H[lvl + 1]; g.Ws = pl.W[lvl + 1];
            g.padT = (g.H - 2 * g.Hs) / 2; g.padL = (g.W - 2 * g.Ws) / 2;
            g.sy = rf_up_scale(g.Hs); g.sx = rf_up_scale(g.Ws);
            e = launch_conv<SRC_UP, 9>(g, stream);
        }
        if (e != hipSuccess) RF_FAIL(LRT_ERR_HIP, "%s: launch of convolution %d.1 failed: %s", fn, i, hipGetErrorString(e));
        par += 2 * ci + 9LL * ci * cm;
        ConvArgs s = {};
        s.H = g.H; s.W = g.W; s.Cin = cm; s.Cout = co; s.a = par; s.b = par + cm; s.w = par + 2 * cm;
        s.src = buf(mid_of[i]); s.dst = buf(out_of[i]); s.relu = 1;
        if ((e = launch_conv<SRC_SAME, 9>(s, stream)) != hipSuccess) RF_FAIL(LRT_ERR_HIP, "%s: launch of convolution %d.2 failed: %s", fn, i, hipGetErrorString(e));
        par += 2 * cm + 9LL * cm * co;
        prev = buf(out_of[i]);
    }
    hipLaunchKernelGGL(k_rf_out, dim3((unsigned)((pl.n[0] + RF_BLOCK - 1) / RF_BLOCK)), dim3(RF_BLOCK), 0, stream, pl.n[0], c, (const float*)buf(RF_Y0), par, par + c, par + 2 * c,
                       par + 3 * c, prob, logits);
    if ((e = hipGetLastError()) != hipSuccess) RF_FAIL(LRT_ERR_HIP, "%s: launch of the output block failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
