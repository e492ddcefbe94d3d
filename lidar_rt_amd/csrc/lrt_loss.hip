// lrt_loss.hip -- the fused range-image training loss (include/lrt_loss.h), gfx950.  Compiled into liblrt_loss.so, a library of its own.
//
//   k_loss_fwd  one workgroup per 16 x 32 tile of the image.  With a DSSIM weight: the masked intensity planes x, y of the tile and a 5-pixel
//               halo go to LDS, the five planes x, y, x^2, y^2, xy are blurred by rows into LDS and by columns into registers, and each pixel's
//               SSIM value and its three derivative maps (lrt_loss_math.h) follow; the pointwise terms (L1 depth, L1 / L2 intensity, ray-drop
//               BCE) in the same pass.  The workgroup's six partial sums are reduced in a fixed order and written to its row of a table.
//   k_loss_fin  one workgroup adds the rows of the table in a fixed order and forms n, the weighted terms and the total.
//   k_loss_bwd  the second blur (of the three derivative maps), the pointwise gradients, and each pixel's 36-byte row of d_rendered staged in
//               LDS and written once, whole and coalesced.
//
// Precision: the window sums, the SSIM arithmetic and every reduction run in float64 (the image has at most a few hundred thousand pixels:
// the op is bound by its launches, not by arithmetic), so the float32 results carry one rounding each.  The ray-drop probability, its clamp
// and the cross-entropy are float32 by contract (the clamp decides in float32 which pixels pass gradient).
// No atomics of any kind: the result does not depend on the order in which the grid executes.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_loss_math.h"
#include "../../include/lrt_loss.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int TH = 16, TW = 32, R = LRT_LOSS_HALF, IH = TH + 2 * R, IW = TW + 2 * R, NT = 256, NW = NT / 64;
constexpr int NSUM = 6;                   // depth L1, intensity L1, intensity L2, SSIM, BCE, valid count
constexpr int HDR_DOUBLES = 8;            // work[0] = n

struct LossArgs {
    int H, W, use_rayhit;
    const float* rendered; const float* gt_depth; const float* gt_int; const uint8_t* mask;
    double w_depth, w_l1, w_l2, w_dssim, w_bce;
    LrtLossWindow win;
};

__device__ inline double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__global__ __launch_bounds__(NT) void k_loss_fwd(LossArgs a, double* __restrict__ partials, float* __restrict__ maps)
{
    __shared__ float sx[IH][IW + 1], sy[IH][IW + 1];
    __shared__ double hd[5][IH][TW + 1];
    __shared__ double red[NSUM][NW];
    const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, H = a.H, W = a.W;
    const bool dssim = a.w_dssim != 0.0;
    if (dssim) {
        for (int i = tid; i < IH * IW; i += NT) {
            const int r = i / IW, c = i - r * IW, gy = y0 - R + r, gx = x0 - R + c;
            float x = 0.f, y = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t p = (size_t)gy * W + gx;
                const float m = a.mask[p] ? 1.f : 0.f;
                x = a.rendered[p * 9] * m; y = a.gt_int[p] * m;
            }
            sx[r][c] = x; sy[r][c] = y;
        }
        __syncthreads();
        for (int i = tid; i < IH * TW; i += NT) {
            const int r = i / TW, c = i - r * TW;
            double h0 = 0, h1 = 0, h2 = 0, h3 = 0, h4 = 0;
#pragma unroll
            for (int k = 0; k < LRT_LOSS_WIN; k++) {
                const double w = a.win.w[k], x = sx[r][c + k], y = sy[r][c + k];
                h0 += w * x; h1 += w * y; h2 += w * (x * x); h3 += w * (y * y); h4 += w * (x * y);
            }
            hd[0][r][c] = h0; hd[1][r][c] = h1; hd[2][r][c] = h2; hd[3][r][c] = h3; hd[4][r][c] = h4;
        }
        __syncthreads();
    }
    double acc[NSUM] = {0, 0, 0, 0, 0, 0};
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW, gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        const size_t p = (size_t)gy * W + gx;
        const float* px = a.rendered + p * 9;
        const float mf = a.mask[p] ? 1.f : 0.f;
        acc[5] += mf;
        if (a.w_depth != 0.0) acc[0] += (double)(fabsf(px[3] - a.gt_depth[p]) * mf);
        if (a.w_l1 != 0.0 || a.w_l2 != 0.0) {
            const float d = px[0] - a.gt_int[p];
            if (a.w_l1 != 0.0) acc[1] += (double)(fabsf(d) * mf);
            if (a.w_l2 != 0.0) acc[2] += (double)d * (double)d * mf;
        }
        if (a.w_bce != 0.0) {
            float dz;
            acc[4] += (double)lrt_loss_bce(lrt_loss_prob(px[1], px[2], a.use_rayhit), 1.f - mf, &dz);
        }
        if (dssim) {
            double v0 = 0, v1 = 0, v2 = 0, v3 = 0, v4 = 0;
#pragma unroll
            for (int k = 0; k < LRT_LOSS_WIN; k++) {
                const double w = a.win.w[k];
                v0 += w * hd[0][r + k][c]; v1 += w * hd[1][r + k][c]; v2 += w * hd[2][r + k][c]; v3 += w * hd[3][r + k][c]; v4 += w * hd[4][r + k][c];
            }
            double S, dmu, de11, de12;
            lrt_loss_ssim<double>(v0, v1, v2, v3, v4, &S, &dmu, &de11, &de12);
            acc[3] += S;
            const size_t np = (size_t)H * W;
            maps[p] = (float)dmu; maps[np + p] = (float)de11; maps[2 * np + p] = (float)de12;
        }
    }
    // fixed order: lanes by the shuffle tree, then the waves by index
#pragma unroll
    for (int j = 0; j < NSUM; j++) {
        const double s = wave_sum(acc[j]);
        if ((tid & 63) == 0) red[j][tid >> 6] = s;
    }
    __syncthreads();
    if (tid < NSUM) {
        double s = red[tid][0];
#pragma unroll
        for (int w = 1; w < NW; w++) s += red[tid][w];
        partials[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * NSUM + tid] = s;
    }
}

__global__ __launch_bounds__(NT) void k_loss_fin(LossArgs a, int rows, const double* __restrict__ partials, double* __restrict__ hdr, float* __restrict__ out)
{
    __shared__ double sh[NSUM][NT];
    const int tid = threadIdx.x;
    double s[NSUM] = {0, 0, 0, 0, 0, 0};
    for (int r = tid; r < rows; r += NT)
#pragma unroll
        for (int j = 0; j < NSUM; j++) s[j] += partials[(size_t)r * NSUM + j];
#pragma unroll
    for (int j = 0; j < NSUM; j++) sh[j][tid] = s[j];
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) {
        if (tid < o)
#pragma unroll
            for (int j = 0; j < NSUM; j++) sh[j][tid] += sh[j][tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const double n = sh[5][0] > 1.0 ? sh[5][0] : 1.0, N = (double)a.H * (double)a.W;
        const double depth = a.w_depth != 0.0 ? a.w_depth * sh[0][0] / n : 0.0;
        double inten = 0.0;
        if (a.w_l1 != 0.0) inten += a.w_l1 * sh[1][0] / n;
        if (a.w_l2 != 0.0) inten += a.w_l2 * sh[2][0] / n;
        if (a.w_dssim != 0.0) inten += a.w_dssim * (1.0 - sh[3][0] / N);
        const double drop = a.w_bce != 0.0 ? a.w_bce * sh[4][0] / N : 0.0;
        out[0] = (float)(depth + inten + drop); out[1] = (float)depth; out[2] = (float)inten; out[3] = (float)drop; out[4] = (float)n;
        hdr[0] = n;
    }
}

__global__ __launch_bounds__(NT) void k_loss_bwd(LossArgs a, const double* __restrict__ hdr, const float* __restrict__ maps,
                                                 const float* __restrict__ d_total, float* __restrict__ d_rendered)
{
    __shared__ float sm[3][IH][IW + 1];
    __shared__ double hd[3][IH][TW + 1];
    __shared__ float so[TH][TW * 9];
    const int tid = threadIdx.x, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH, H = a.H, W = a.W;
    const bool dssim = a.w_dssim != 0.0;
    const size_t np = (size_t)H * W;
    if (dssim) {
        for (int i = tid; i < IH * IW; i += NT) {
            const int r = i / IW, c = i - r * IW, gy = y0 - R + r, gx = x0 - R + c;
            float m0 = 0.f, m1 = 0.f, m2 = 0.f;
            if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
                const size_t p = (size_t)gy * W + gx;
                m0 = maps[p]; m1 = maps[np + p]; m2 = maps[2 * np + p];
            }
            sm[0][r][c] = m0; sm[1][r][c] = m1; sm[2][r][c] = m2;
        }
        __syncthreads();
        for (int i = tid; i < IH * TW; i += NT) {
            const int r = i / TW, c = i - r * TW;
            double h0 = 0, h1 = 0, h2 = 0;
#pragma unroll
            for (int k = 0; k < LRT_LOSS_WIN; k++) {
                const double w = a.win.w[k];
                h0 += w * sm[0][r][c + k]; h1 += w * sm[1][r][c + k]; h2 += w * sm[2][r][c + k];
            }
            hd[0][r][c] = h0; hd[1][r][c] = h1; hd[2][r][c] = h2;
        }
        __syncthreads();
    }
    const double up = (double)d_total[0], s_n = up / hdr[0], s_N = up / ((double)H * (double)W);
    for (int i = tid; i < TH * TW; i += NT) {
        const int r = i / TW, c = i - r * TW, gy = y0 + r, gx = x0 + c;
        if (gy >= H || gx >= W) continue;
        const size_t p = (size_t)gy * W + gx;
        const float* px = a.rendered + p * 9;
        const float mf = a.mask[p] ? 1.f : 0.f;
        double g0 = 0.0, g3 = 0.0;
        float g1 = 0.f, g2 = 0.f;
        if (a.w_depth != 0.0) {
            const float d = px[3] - a.gt_depth[p];
            g3 = (d > 0.f ? 1.0 : (d < 0.f ? -1.0 : (double)(d * 0.f))) * a.w_depth * s_n * mf;      // sign(0) = 0; a NaN stays one
        }
        const float r0 = px[0], gi = a.gt_int[p];
        if (a.w_l1 != 0.0 || a.w_l2 != 0.0) {
            const float d = r0 - gi;
            if (a.w_l1 != 0.0) g0 += (d > 0.f ? 1.0 : (d < 0.f ? -1.0 : (double)(d * 0.f))) * a.w_l1 * s_n;
            if (a.w_l2 != 0.0) g0 += 2.0 * (double)d * a.w_l2 * s_n;
        }
        if (dssim) {
            double v0 = 0, v1 = 0, v2 = 0;
#pragma unroll
            for (int k = 0; k < LRT_LOSS_WIN; k++) {
                const double w = a.win.w[k];
                v0 += w * hd[0][r + k][c]; v1 += w * hd[1][r + k][c]; v2 += w * hd[2][r + k][c];
            }
            g0 -= a.w_dssim * s_N * (v0 + 2.0 * (double)(r0 * mf) * v1 + (double)(gi * mf) * v2);
        }
        g0 *= mf;
        if (a.w_bce != 0.0) {
            float dz;
            (void)lrt_loss_bce(lrt_loss_prob(px[1], px[2], a.use_rayhit), 1.f - mf, &dz);
            g2 = (float)(a.w_bce * s_N * (double)dz);
            g1 = a.use_rayhit ? -g2 : 0.f;
        }
        float* o = &so[r][c * 9];
        o[0] = (float)g0; o[1] = g1; o[2] = g2; o[3] = (float)g3; o[4] = 0.f; o[5] = 0.f; o[6] = 0.f; o[7] = 0.f; o[8] = 0.f;
    }
    __syncthreads();
    // the tile's rows of d_rendered are contiguous runs of 9 * (columns inside the image) floats
    const int ncol9 = (W - x0 < TW ? W - x0 : TW) * 9;
    for (int i = tid; i < TH * TW * 9; i += NT) {
        const int r = i / (TW * 9), j = i - r * (TW * 9), gy = y0 + r;
        if (gy < H && j < ncol9) d_rendered[((size_t)gy * W + x0) * 9 + j] = so[r][j];
    }
}

static thread_local char g_err[512] = "";

#define LOSS_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static inline size_t tiles(int H, int W) { return (size_t)((H + TH - 1) / TH) * (size_t)((W + TW - 1) / TW); }
static inline bool size_ok(int H, int W) { return H > 0 && W > 0 && H <= TH * 65535 && W <= (1 << 20) && (size_t)H * W <= ((size_t)1 << 27); }   // grid.y <= 65535
static inline size_t partial_bytes(int H, int W) { return (tiles(H, W) * NSUM * sizeof(double) + 15) / 16 * 16; }

static int loss_check(const char* fn, int device, int H, int W, const void* rendered, const void* gt_depth, const void* gt_int, const void* mask,
               const double* weights, const void* work, size_t work_bytes)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) LOSS_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, n);
    if (!size_ok(H, W)) LOSS_FAIL(LRT_ERR_ARG, "%s: unsupported image size %d x %d", fn, H, W);
    if (!rendered || !gt_depth || !gt_int || !mask || !weights) LOSS_FAIL(LRT_ERR_ARG, "%s: null image / mask / weights pointer", fn);
    for (int i = 0; i < 5; i++) if (!(weights[i] == weights[i])) LOSS_FAIL(LRT_ERR_ARG, "%s: weight %d is NaN", fn, i);
    if (!work || work_bytes < lrt_loss_work_bytes(H, W)) LOSS_FAIL(LRT_ERR_ARG, "%s: workspace of %zu bytes, need %zu", fn, work_bytes, lrt_loss_work_bytes(H, W));
    if (((uintptr_t)work & 15) != 0) LOSS_FAIL(LRT_ERR_ARG, "%s: the workspace must be 16-byte aligned", fn);
    return LRT_OK;
}

static LossArgs make_args(int H, int W, const float* rendered, const float* gt_depth, const float* gt_int, const uint8_t* mask, const double* w, int use_rayhit)
{
    static const LrtLossWindow win = lrt_loss_window();
    LossArgs a;
    a.H = H; a.W = W; a.use_rayhit = use_rayhit ? 1 : 0;
    a.rendered = rendered; a.gt_depth = gt_depth; a.gt_int = gt_int; a.mask = mask;
    a.w_depth = w[0]; a.w_l1 = w[1]; a.w_l2 = w[2]; a.w_dssim = w[3]; a.w_bce = w[4];
    a.win = win;
    return a;
}

extern "C" {

int lrt_loss_abi_version(void) { return LRT_LOSS_ABI_VERSION; }

const char* lrt_loss_last_error(void) { return g_err; }

size_t lrt_loss_work_bytes(int H, int W)
{
    if (!size_ok(H, W)) return 0;
    return HDR_DOUBLES * sizeof(double) + partial_bytes(H, W) + 3 * (size_t)H * W * sizeof(float);
}

int lrt_loss_forward(int device, int H, int W, const float* rendered, const float* gt_depth, const float* gt_intensity,
                     const uint8_t* mask, const double* weights, int use_rayhit, float* out, void* work, size_t work_bytes, void* stream_)
{
    const char* fn = "lrt_loss_forward";
    if (int rc = loss_check(fn, device, H, W, rendered, gt_depth, gt_intensity, mask, weights, work, work_bytes)) return rc;
    if (!out) LOSS_FAIL(LRT_ERR_ARG, "%s: null output pointer", fn);
    LrtDeviceGuard guard(device);
    if (!guard.ok) LOSS_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const LossArgs a = make_args(H, W, rendered, gt_depth, gt_intensity, mask, weights, use_rayhit);
    double* hdr = (double*)work; double* partials = hdr + HDR_DOUBLES;
    float* maps = (float*)((char*)partials + partial_bytes(H, W));
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH);
    hipLaunchKernelGGL(k_loss_fwd, grid, dim3(NT), 0, stream, a, partials, maps);
    hipLaunchKernelGGL(k_loss_fin, dim3(1), dim3(NT), 0, stream, a, (int)tiles(H, W), (const double*)partials, hdr, out);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) LOSS_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

int lrt_loss_backward(int device, int H, int W, const float* rendered, const float* gt_depth, const float* gt_intensity,
                      const uint8_t* mask, const double* weights, int use_rayhit, const float* d_total, float* d_rendered, void* work,
                      size_t work_bytes, void* stream_)
{
    const char* fn = "lrt_loss_backward";
    if (int rc = loss_check(fn, device, H, W, rendered, gt_depth, gt_intensity, mask, weights, work, work_bytes)) return rc;
    if (!d_total || !d_rendered) LOSS_FAIL(LRT_ERR_ARG, "%s: null gradient pointer", fn);
    LrtDeviceGuard guard(device);
    if (!guard.ok) LOSS_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    hipStream_t stream = (hipStream_t)stream_;
    const LossArgs a = make_args(H, W, rendered, gt_depth, gt_intensity, mask, weights, use_rayhit);
    const double* hdr = (const double*)work;
    const float* maps = (const float*)((const char*)(hdr + HDR_DOUBLES) + partial_bytes(H, W));
    const dim3 grid((W + TW - 1) / TW, (H + TH - 1) / TH);
    hipLaunchKernelGGL(k_loss_bwd, grid, dim3(NT), 0, stream, a, hdr, maps, d_total, d_rendered);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) LOSS_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
