// lrt_adam_math.h -- the arithmetic of the fused Adam step (include/lrt_adam.h), host and device.  T is the type the tensors are stored in:
// float in the kernel, double in the host check's yardstick (tests/host_check/adam_check.cpp), which runs the same text.
//
// The moment lines are evaluated in double whatever T is and rounded to T once each.  torch's fused kernel does the same (its beta1 / beta2 are
// doubles, so `beta2 * exp_avg_sq + (1 - beta2) * grad * grad` is double arithmetic on float32 operands).  Float32 arithmetic there is not
// "one rounding more": (float)(1 - 0.999) alone is 0.8 ulp off, a first step's exp_avg_sq ends 2.2 ulp from the float64 value against 0.5.
// The kernel is bound by memory, the eight double operations per element do not show.
#pragma once
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LRT_ADAM_HD __host__ __device__ __forceinline__
#else
#define LRT_ADAM_HD inline
#endif

struct LrtAdamRule { double w1, b2, w2, eps; };                  // w1 = 1 - beta1, w2 = 1 - beta2: formed in double by the caller

template <typename T> struct LrtAdamStep { T step_size, bc2_sqrt; };

LRT_ADAM_HD LrtAdamRule lrt_adam_rule(double beta1, double beta2, double eps)
{
    LrtAdamRule r; r.w1 = 1.0 - beta1; r.b2 = beta2; r.w2 = 1.0 - beta2; r.eps = eps;
    return r;
}

// lr / bias_correction1: one double division, the quotient rounded to T
template <typename T> LRT_ADAM_HD LrtAdamStep<T> lrt_adam_step_of(double lr, double bias_correction1, double bias_correction2_sqrt)
{
    LrtAdamStep<T> s;
    s.step_size = (T)(lr / bias_correction1);
    s.bc2_sqrt = (T)bias_correction2_sqrt;
    return s;
}

LRT_ADAM_HD float lrt_adam_sqrt(float x) { return sqrtf(x); }
LRT_ADAM_HD double lrt_adam_sqrt(double x) { return sqrt(x); }

template <typename T> LRT_ADAM_HD void lrt_adam_update(T& p, T g, T& m, T& v, const LrtAdamRule& r, const LrtAdamStep<T>& s)
{
#if defined(__clang__)
#pragma clang fp contract(off)                                   // every operation rounds on its own, on the device as on the host
#endif
    const double gd = (double)g, md = (double)m, vd = (double)v;
    m = (T)(md + r.w1 * (gd - md));
    v = (T)(r.b2 * vd + r.w2 * gd * gd);
    const T denom = (T)((double)(lrt_adam_sqrt(v) / s.bc2_sqrt) + r.eps);
    p -= s.step_size * m / denom;
}
