// lrt_densify_math.h -- the per-row rule of the fused densify-and-prune (include/lrt_densify.h), host and device.  The kernels of
// lrt_densify.hip and the host check (tests/host_check/densify_check.cpp) run this text.
//
// The rule restates GaussianAsset.densify_and_prune (lidar_rt_amd/training.py; the reference's gaussian_model.py:311-407) with explicit noise.
// Per source row i:
//   1. g = accum / denom, one IEEE float32 division; NaN -> 0, +inf -> FLT_MAX, -inf -> -FLT_MAX (nan_to_num(0.0)).  hot = g >= grad_thr.
//      big = max_k expf(scaling_k) > big_thr.
//   2. hot & !big: CLONE -- the row stays (slot 0) and an unchanged copy is emitted (slot 1).  hot & big: SPLIT -- the row is replaced by two
//      children (slot 0: child 0, slot 1: child 1).  Anything else: KEEP (slot 0 only).
//   3. child c: xyz + R(q / |q|) (exp(scaling) * split_noise[i, c, :S]), the third component 0 when S == 2; scaling - log 1.6 (= log(exp(scaling) / 1.6)).
//      Both are evaluated in double and rounded to float32 ONCE per component: half a float32 ulp from the exact value, whatever cancels inside.
//   4. per output: low = sigmoid(opacity) < opa_thr; with size_limit huge = max_k expf(out_scaling_k) > huge_thr; with size_limit and a box
//      outside = not all of the 2 samples out_xyz + R (exp(out_scaling) * box_noise[i, slot, s]) lie within [box_min, box_max].
//      An output is marked for pruning when any of the three holds.  Whether the marks are applied is decided over the whole asset (they are
//      not when they would remove every output): lrt_densify.hip.
// The decisions (>=, >, <) are float32 comparisons of float32 values, as the torch path makes them; the geometry is double.
#pragma once
#include <float.h>
#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LRT_DENSIFY_HD __host__ __device__ __forceinline__
#else
#define LRT_DENSIFY_HD inline
#endif

#define LRT_DENSIFY_KEEP 0u
#define LRT_DENSIFY_CLONE 1u
#define LRT_DENSIFY_SPLIT 2u
// the code of a row: bits 0-1 the kind, then one bit per (flag, slot)
#define LRT_DENSIFY_KIND_MASK 3u
#define LRT_DENSIFY_PRUNE0 (1u << 2)
#define LRT_DENSIFY_PRUNE1 (1u << 3)
#define LRT_DENSIFY_LOW0 (1u << 4)
#define LRT_DENSIFY_LOW1 (1u << 5)
#define LRT_DENSIFY_HUGE0 (1u << 6)
#define LRT_DENSIFY_HUGE1 (1u << 7)
#define LRT_DENSIFY_OUT0 (1u << 8)
#define LRT_DENSIFY_OUT1 (1u << 9)

#define LRT_DENSIFY_LOG_1_6 0.47000362924573555   /* log(1.6) */

struct LrtDensifyRule {
    float grad_thr, big_thr, huge_thr, opa_thr;
    int size_limit, has_box;
    float box_min[3], box_max[3];
};

// g of step 1
LRT_DENSIFY_HD float lrt_densify_mean_grad(float accum, float denom)
{
    float g = accum / denom;
    if (g != g) g = 0.f;
    else if (g > FLT_MAX) g = FLT_MAX;
    else if (g < -FLT_MAX) g = -FLT_MAX;
    return g;
}

LRT_DENSIFY_HD float lrt_densify_max_exp(const float* s, int S)
{
    float m = expf(s[0]);
    for (int k = 1; k < S; k++) { const float e = expf(s[k]); m = e > m ? e : m; }
    return m;
}

LRT_DENSIFY_HD float lrt_densify_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// the rotation matrix of q / |q| (w, x, y, z), row-major, double
LRT_DENSIFY_HD void lrt_densify_rotation(const float* q, double* R)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double n = sqrt((double)q[0] * q[0] + (double)q[1] * q[1] + (double)q[2] * q[2] + (double)q[3] * q[3]);
    const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// c + R (sd * noise[:S]): sd = exp(scaling) in double; the result in double
LRT_DENSIFY_HD void lrt_densify_sample(const double* c, const double* R, const double* sd, int S, const float* noise, double* out)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    const double v0 = sd[0] * (double)noise[0], v1 = sd[1] * (double)noise[1], v2 = S == 3 ? sd[2] * (double)noise[2] : 0.0;
    for (int k = 0; k < 3; k++) out[k] = c[k] + ((R[3 * k] * v0 + R[3 * k + 1] * v1) + R[3 * k + 2] * v2);
}

LRT_DENSIFY_HD float lrt_densify_child_scaling(float s) { return (float)((double)s - LRT_DENSIFY_LOG_1_6); }

// Step 3 for one row: the two children's positions (float32, rounded once) from the row's xyz, scaling, rotation and split_noise (2, 3).
LRT_DENSIFY_HD void lrt_densify_children(const float* xyz, const float* scaling, int S, const float* q, const float* split_noise, float* child_xyz /* (2, 3) */)
{
    double R[9], sd[3] = {0.0, 0.0, 0.0}, c[3] = {(double)xyz[0], (double)xyz[1], (double)xyz[2]}, o[3];
    lrt_densify_rotation(q, R);
    for (int k = 0; k < S; k++) sd[k] = exp((double)scaling[k]);
    for (int ch = 0; ch < 2; ch++) {
        lrt_densify_sample(c, R, sd, S, split_noise + 3 * ch, o);
        for (int k = 0; k < 3; k++) child_xyz[3 * ch + k] = (float)o[k];
    }
}

// Steps 1, 2 and 4 for one row: its code.  box_noise (2 slots, 2 samples, 3) is read only with size_limit and a box.
LRT_DENSIFY_HD unsigned lrt_densify_row(const float* xyz, const float* scaling, int S, const float* q, float opacity, float accum, float denom,
                                        const float* split_noise, const float* box_noise, const LrtDensifyRule& r)
{
    const bool hot = lrt_densify_mean_grad(accum, denom) >= r.grad_thr;
    const bool big = lrt_densify_max_exp(scaling, S) > r.big_thr;
    const unsigned kind = hot ? (big ? LRT_DENSIFY_SPLIT : LRT_DENSIFY_CLONE) : LRT_DENSIFY_KEEP;
    unsigned code = kind;
    const bool low = lrt_densify_sigmoid(opacity) < r.opa_thr;
    if (low) code |= LRT_DENSIFY_LOW0 | (kind != LRT_DENSIFY_KEEP ? LRT_DENSIFY_LOW1 : 0u);
    if (r.size_limit) {
        float out_s[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < S; k++) out_s[k] = kind == LRT_DENSIFY_SPLIT ? lrt_densify_child_scaling(scaling[k]) : scaling[k];
        if (lrt_densify_max_exp(out_s, S) > r.huge_thr) code |= LRT_DENSIFY_HUGE0 | (kind != LRT_DENSIFY_KEEP ? LRT_DENSIFY_HUGE1 : 0u);   // both outputs of a row have one scaling
        if (r.has_box) {
            float cx[6];
            if (kind == LRT_DENSIFY_SPLIT) lrt_densify_children(xyz, scaling, S, q, split_noise, cx);
            double R[9], sd[3] = {0.0, 0.0, 0.0}, p[3];
            lrt_densify_rotation(q, R);
            for (int k = 0; k < S; k++) sd[k] = exp((double)out_s[k]);
            const int n_slots = kind == LRT_DENSIFY_KEEP ? 1 : 2;
            for (int slot = 0; slot < n_slots; slot++) {
                double c[3];
                for (int k = 0; k < 3; k++) c[k] = kind == LRT_DENSIFY_SPLIT ? (double)cx[3 * slot + k] : (double)xyz[k];
                bool inside = true;
                for (int s = 0; s < 2; s++) {
                    lrt_densify_sample(c, R, sd, S, box_noise + 3 * (2 * slot + s), p);
                    for (int k = 0; k < 3; k++) inside = inside && p[k] >= (double)r.box_min[k] && p[k] <= (double)r.box_max[k];
                }
                if (!inside) code |= slot == 0 ? LRT_DENSIFY_OUT0 : LRT_DENSIFY_OUT1;
            }
        }
    }
    if (code & (LRT_DENSIFY_LOW0 | LRT_DENSIFY_HUGE0 | LRT_DENSIFY_OUT0)) code |= LRT_DENSIFY_PRUNE0;
    if (code & (LRT_DENSIFY_LOW1 | LRT_DENSIFY_HUGE1 | LRT_DENSIFY_OUT1)) code |= LRT_DENSIFY_PRUNE1;
    return code;
}

// The statistics of one iteration for one row: accum + |g| in double, rounded to float32 once.
LRT_DENSIFY_HD float lrt_densify_accumulate(float accum, float gx, float gy, float gz)
{
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    return (float)((double)accum + sqrt(((double)gx * gx + (double)gy * gy) + (double)gz * gz));
}
