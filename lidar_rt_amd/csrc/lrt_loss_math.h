// lrt_loss_math.h -- the per-pixel arithmetic of the fused range-image loss (lrt_loss.hip), as host/device inline functions so that a plain
// host compile can check it without a GPU (tests/host_check/loss_check.cpp).
//
//   window   : the reference's 1-D Gaussian SSIM window (lib/utils/loss_utils.py gaussian(): 11 taps, sigma 1.5, normalised), in float32
//              like training._blur_matrix builds it
//   SSIM     : value and the three partial derivatives the backward blurs, from the five blurred planes of one pixel
//   ray drop : probability (sigmoid, or the two-way softmax of use_rayhit), clamp to [1e-7, 1 - 1e-7] and binary cross-entropy in float32,
//              operation for operation what torch.sigmoid / softmax / clamp / F.binary_cross_entropy and their backwards compute
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define LRT_LOSS_HD __host__ __device__ inline
#else
#define LRT_LOSS_HD inline
#endif

#define LRT_LOSS_WIN 11
#define LRT_LOSS_HALF 5

struct LrtLossWindow { float w[LRT_LOSS_WIN]; };

// exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, float32 values; the sum is the correctly rounded float32 sum of the eleven taps (what a float32 tensor
// sum returns for so few terms), taken here through a float64 accumulator
inline LrtLossWindow lrt_loss_window()
{
    LrtLossWindow g; double s = 0.0;
    for (int i = 0; i < LRT_LOSS_WIN; i++) { const float d = (float)(i - LRT_LOSS_HALF); g.w[i] = expf(-(d * d) / (2.f * 1.5f * 1.5f)); s += (double)g.w[i]; }
    const float sf = (float)s;
    for (int i = 0; i < LRT_LOSS_WIN; i++) g.w[i] /= sf;
    return g;
}

// One pixel of the SSIM map.  mu1, mu2, e11, e22, e12: the window means of x, y, x^2, y^2, xy (x = the rendered image).
// S  = (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)),  s1 = e11 - mu1^2, s2 = e22 - mu2^2, s12 = e12 - mu1 mu2.
// dmu = dS/dmu1 with e11, e12 held fixed (the sigma terms folded in), de11 = dS/ds1, de12 = dS/ds12: the gradient of sum_q S(q) w.r.t. x(p) is
// sum_q w(q - p) [dmu(q) + 2 x(p) de11(q) + y(p) de12(q)].
template <class T>
LRT_LOSS_HD void lrt_loss_ssim(T mu1, T mu2, T e11, T e22, T e12, T* S, T* dmu, T* de11, T* de12)
{
    const T C1 = (T)(0.01 * 0.01), C2 = (T)(0.03 * 0.03);
    const T s1 = e11 - mu1 * mu1, s2 = e22 - mu2 * mu2, s12 = e12 - mu1 * mu2;
    const T a1 = 2 * mu1 * mu2 + C1, a2 = 2 * s12 + C2, b1 = mu1 * mu1 + mu2 * mu2 + C1, b2 = s1 + s2 + C2;
    const T inv = 1 / (b1 * b2), s = a1 * a2 * inv;
    const T ds1 = -s / b2, ds12 = 2 * a1 * inv;
    *S = s; *de11 = ds1; *de12 = ds12;
    *dmu = 2 * mu2 * a2 * inv - 2 * mu1 * s / b1 - 2 * mu1 * ds1 - mu2 * ds12;
}

// the ray-drop probability of a pixel: sigmoid(drop logit), or softmax(hit logit, drop logit)[1] with use_rayhit
LRT_LOSS_HD float lrt_loss_prob(float hit_logit, float drop_logit, int use_rayhit)
{
    if (!use_rayhit) return 1.f / (1.f + expf(-drop_logit));
    const float mx = fmaxf(hit_logit, drop_logit), eh = expf(hit_logit - mx), ed = expf(drop_logit - mx);
    return ed / (eh + ed);
}

#define LRT_LOSS_P_LO ((float)1e-7)
#define LRT_LOSS_P_HI ((float)(1.0 - 1e-7))

// BCE(clamp(p), label) as F.binary_cross_entropy computes it (logs bounded below by -100); *dz = its derivative w.r.t. the drop logit:
// (pc - label) / max((1 - pc) pc, 1e-12), times 1 where the clamp passes (lo <= p <= hi, as torch.clamp's backward), times p (1 - p).
// The derivative w.r.t. the hit logit (use_rayhit) is -*dz.
LRT_LOSS_HD float lrt_loss_bce(float p, float label, float* dz)
{
    const float pc = fminf(fmaxf(p, LRT_LOSS_P_LO), LRT_LOSS_P_HI);
    const float v = (label - 1.f) * fmaxf(log1pf(-pc), -100.f) - label * fmaxf(logf(pc), -100.f);
    const float pass = (p >= LRT_LOSS_P_LO && p <= LRT_LOSS_P_HI) ? 1.f : 0.f;
    *dz = (pc - label) / fmaxf((1.f - pc) * pc, 1e-12f) * pass * (p * (1.f - p));
    return v;
}
