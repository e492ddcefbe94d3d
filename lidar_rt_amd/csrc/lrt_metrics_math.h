// lrt_metrics_math.h -- the arithmetic of the fused evaluation metrics (include/lrt_metrics.h), host/device inline: the per-pixel clamps and
// error, the per-window SSIM term, the ray-drop and points ratios, and the rank selection behind medae.  lrt_metrics.hip compiles it for gfx950,
// tests/host_check/metrics_check.cpp for the host.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define MT_HD __host__ __device__ __forceinline__
#else
#define MT_HD static inline
#endif

// ---- per pixel ---------------------------------------------------------------------------------------------------------------------------------
// torch.clamp: a NaN stays a NaN
MT_HD float mt_clamp(float x, float lo, float hi) { return x != x ? x : fminf(fmaxf(x, lo), hi); }

// depth: clamp(gt, 1e-6, max_depth) against clamp(pred * mask, 1e-6, max_depth)
MT_HD float mt_depth_gt(float gt, float max_depth) { return mt_clamp(gt, 1e-6f, max_depth); }
MT_HD float mt_depth_pred(float pred, bool m, float max_depth) { return mt_clamp(pred * (m ? 1.f : 0.f), 1e-6f, max_depth); }
// intensity: clamp(clamp(gt, 0, 1), 1e-6, 1) against clamp(clamp(pred, 0, 1) * mask, 1e-6, 1)
MT_HD float mt_intensity_gt(float gt) { return mt_clamp(mt_clamp(gt, 0.f, 1.f), 1e-6f, 1.f); }
MT_HD float mt_intensity_pred(float pred, bool m) { return mt_clamp(mt_clamp(pred, 0.f, 1.f) * (m ? 1.f : 0.f), 1e-6f, 1.f); }

MT_HD uint32_t mt_float_bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }
MT_HD float mt_bits_float(uint32_t u) { float x; memcpy(&x, &u, 4); return x; }

// The selection key of an error gt - pred (ONE float32 subtraction): the bit pattern of its absolute value.  Non-negative floats order like
// their bit patterns read as unsigned integers (NaNs above +inf: where a sort puts them).
MT_HD uint32_t mt_abs_key(float err) { return mt_float_bits(err) & 0x7fffffffu; }

// ---- rank selection ------------------------------------------------------------------------------------------------------------------------------
// Three levels over the 31 bits below the sign: 11 / 11 / 9.  A level's digit of a key, the number of bins, and the bits above the level (the
// prefix a key must carry to be counted there).
#define MT_L1_BINS 2048
#define MT_L2_BINS 2048
#define MT_L3_BINS 512
MT_HD uint32_t mt_digit(uint32_t key, int level) { return level == 1 ? key >> 20 : level == 2 ? (key >> 9) & 2047u : key & 511u; }
MT_HD uint32_t mt_prefix(uint32_t key, int level) { return level == 1 ? 0u : level == 2 ? key >> 20 : key >> 9; }
// the prefix of the next level: this level's prefix extended by the selected digit
MT_HD uint32_t mt_extend(uint32_t prefix, uint32_t digit, int level) { return level == 1 ? digit : level == 2 ? (prefix << 11) | digit : (prefix << 9) | digit; }

// Among the `nb` consecutive bins h[0 .. nb), which follow `before` smaller elements, the one that holds the element of rank k (0-based, in
// sorted order): its index, with the element's rank INSIDE the bin in *rank_in_bin; -1 if rank k lies before or after these bins.  A thread
// of the scan calls it on its own few bins with its exclusive prefix sum, the host check on a whole histogram with before = 0.
MT_HD int mt_find_bin(const uint32_t* h, int nb, uint32_t before, uint32_t k, uint32_t* rank_in_bin)
{
    if (k < before) return -1;
    uint32_t cum = before;
    for (int b = 0; b < nb; b++) {
        const uint32_t c = h[b];
        if (k - cum < c) { *rank_in_bin = k - cum; return b; }
        cum += c;
    }
    return -1;
}

// numpy's median of n float32 values from the two middle elements v[(n - 1) / 2] and v[n / 2] of the sorted array (equal for an odd n)
MT_HD uint32_t mt_rank_lo(uint32_t n) { return (n - 1) / 2; }
MT_HD uint32_t mt_rank_hi(uint32_t n) { return n / 2; }
MT_HD float mt_median(uint32_t key_lo, uint32_t key_hi) { return 0.5f * (mt_bits_float(key_lo) + mt_bits_float(key_hi)); }

// ---- SSIM ----------------------------------------------------------------------------------------------------------------------------------------
#define MT_WIN 7
#define MT_WIN_N 49
// One window of skimage's structural_similarity with its defaults: s[] = the sums of x, y, x^2, y^2, x y over the 7 x 7 window (x the
// prediction, y the ground truth), sample covariance (49 / 48), C1 = (0.01 R)^2, C2 = (0.03 R)^2.
MT_HD double mt_ssim_window(const double* s, double R)
{
    const double ux = s[0] / MT_WIN_N, uy = s[1] / MT_WIN_N, norm = (double)MT_WIN_N / (MT_WIN_N - 1.0);
    const double vx = norm * (s[2] / MT_WIN_N - ux * ux), vy = norm * (s[3] / MT_WIN_N - uy * uy), vxy = norm * (s[4] / MT_WIN_N - ux * uy);
    const double c1 = (0.01 * R) * (0.01 * R), c2 = (0.03 * R) * (0.03 * R);
    return ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
}

// ---- the scalars -----------------------------------------------------------------------------------------------------------------------------------
MT_HD double mt_rmse(double sum_sq, double n) { return sqrt(sum_sq / n); }
MT_HD double mt_psnr(double sum_sq, double n, double peak)
{
    const double mse = sum_sq / n;
    return 10.0 * log10(peak * peak / (mse < 1e-30 ? 1e-30 : mse));          // a NaN mse stays (the comparison is false)
}
// ray drop, on the (1 - hit) masks: tp = both dropped, fp = only the prediction dropped, fn = only the ground truth dropped
MT_HD double mt_f1(double tp, double fp, double fn)
{
    const double dp = tp + fp, dr = tp + fn;
    const double precision = tp / (dp < 1.0 ? 1.0 : dp), recall = tp / (dr < 1.0 ? 1.0 : dr), s = precision + recall;
    return 2 * precision * recall / (s < 1e-30 ? 1e-30 : s);
}
// points: p = count(dist < threshold) / n of each cloud, NaN -> 0; an empty cloud: 0
MT_HD double mt_fscore(double below_a, double n_a, double below_b, double n_b)
{
    if (!(n_a > 0) || !(n_b > 0)) return 0.0;
    const double p1 = below_a / n_a, p2 = below_b / n_b, f = 2 * p1 * p2 / (p1 + p2);
    return f == f ? f : 0.0;
}
