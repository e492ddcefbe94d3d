// lrt_reg_math.h -- the rule of the scan registration (include/lrt_reg.h): the one text for the device (lrt_reg.hip) and the host
// (tests/host_check/reg_check.cpp, g++ -ffp-contract=off).  The pixel rule is lrt_project_math.h's and Exp is lrt_sweep_math.h's, both unchanged.
//
//   rg_d2      a pair's squared distance in float32: d = target - query, fma(dz, dz, fma(dy, dy, dx * dx)) (the expression of lrt_gridcd_math.h)
//   rg_pixel   one source pixel: q = X p, its centre pixel, the partner of the window, the residual, the Huber weight, the Jacobian and the
//              pixel's 30 terms.  Returns the partner's linear pixel index or -1 (the terms are left as they are then: the caller zeroes them)
//   rg_solve   one pair's step from its 30 sums: the status, (A + lambda diag A + eps I) delta = -b by Cholesky, X <- X Exp(delta)
//
// Float64 with every operation rounded on its own, but for rg_d2 and the one rounding q32 = (float) q.
#ifndef LRT_REG_MATH_H_INCLUDED
#define LRT_REG_MATH_H_INCLUDED

#include <math.h>
#include "lrt_project_math.h"
#include "lrt_sweep_math.h"

#define RG_HD PJ_HD
#if defined(__clang__)
#define RG_UNROLL _Pragma("unroll")
#else
#define RG_UNROLL
#endif

#define RG_NSUM 30          /* 21 of A, 6 of b, sum w e^2, sum w, partners */
#define RG_EPS 1e-12        /* LRT_REG_EPS */
#define RG_OK 0
#define RG_FEW 1
#define RG_PIVOT 2
#define RG_CONVERGED 3

#if defined(__HIP_DEVICE_COMPILE__)
RG_HD float rg_fmaf(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
RG_HD float rg_fmaf(float a, float b, float c) { return fmaf(a, b, c); }
#endif

RG_HD float rg_d2(const float* t, const float* q)
{
#pragma clang fp contract(off)
    const float dx = t[0] - q[0], dy = t[1] - q[1], dz = t[2] - q[2];
    const float xx = dx * dx;
    return rg_fmaf(dz, dz, rg_fmaf(dy, dy, xx));
}

// X (3, 4) row-major; p: the source point; tp, tn, tm: the target's points, normals and mask (H W pixels).  max_d2 = max_dist * max_dist.
// t: RG_NSUM terms, written only when there is a partner.
RG_HD int rg_pixel(const double* X, const float* p, const PjRule& R, const double* inc, const float* tp, const float* tn, const unsigned char* tm,
                   int rh, int rw, double max_d2, double huber, double* t)
{
#pragma clang fp contract(off)
    double q[3];
    pj_transform(X, p[0], p[1], p[2], q);
    int w0, h0;
    float r32;
    if (pj_classify(q, R, inc, &w0, &h0, &r32) != PJ_KEEP) return -1;
    const float q32[3] = {(float)q[0], (float)q[1], (float)q[2]};
    int best = -1;
    float best_d2 = 0.f;
    for (int dh = -rh; dh <= rh; dh++) {
        const int h = h0 + dh;
        if (h < 0 || h >= R.H) continue;
        for (int dw = -rw; dw <= rw; dw++) {
            int w = (w0 + dw) % R.W;
            if (w < 0) w += R.W;
            const int j = h * R.W + w;
            if (!tm[j]) continue;
            const float d2 = rg_d2(tp + 3 * (long long)j, q32);
            if (!(d2 == d2)) continue;                                   // not a number: never a partner
            if (best < 0 || d2 < best_d2 || (d2 == best_d2 && j < best)) { best = j; best_d2 = d2; }
        }
    }
    if (best < 0 || !((double)best_d2 <= max_d2)) return -1;
    const double n[3] = {(double)tn[3 * (long long)best], (double)tn[3 * (long long)best + 1], (double)tn[3 * (long long)best + 2]};
    if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return -1;
    const double qt[3] = {(double)tp[3 * (long long)best], (double)tp[3 * (long long)best + 1], (double)tp[3 * (long long)best + 2]};
    const double e = n[0] * (q[0] - qt[0]) + n[1] * (q[1] - qt[1]) + n[2] * (q[2] - qt[2]);
    const double ae = fabs(e);
    const double wt = ae <= huber ? 1.0 : huber / ae;
    const double pd[3] = {(double)p[0], (double)p[1], (double)p[2]};
    double J[6];
    J[0] = X[0] * n[0] + X[4] * n[1] + X[8] * n[2];
    J[1] = X[1] * n[0] + X[5] * n[1] + X[9] * n[2];
    J[2] = X[2] * n[0] + X[6] * n[1] + X[10] * n[2];
    J[3] = pd[1] * J[2] - pd[2] * J[1];
    J[4] = pd[2] * J[0] - pd[0] * J[2];
    J[5] = pd[0] * J[1] - pd[1] * J[0];
    int k = 0;
    RG_UNROLL
    for (int i = 0; i < 6; i++) {
        const double wj = wt * J[i];
        RG_UNROLL
        for (int j = i; j < 6; j++) t[k++] = wj * J[j];
    }
    RG_UNROLL
    for (int i = 0; i < 6; i++) t[21 + i] = (wt * J[i]) * e;
    t[27] = (wt * e) * e;
    t[28] = wt;
    t[29] = 1.0;
    return best;
}

// s: a pair's RG_NSUM sums.  X (3, 4) row-major float64, replaced by X Exp(delta) when the status is RG_OK and untouched otherwise.
// norms: |rho| and |phi| of the step (0, 0 for RG_FEW and RG_PIVOT).
RG_HD int rg_solve(const double* s, double lambda, double min_pairs, double tol_t, double tol_r, double* X, double* norms)
{
#pragma clang fp contract(off)
    norms[0] = 0.0; norms[1] = 0.0;
    if (!(s[29] >= min_pairs)) return RG_FEW;
    double M[6][6], L[6][6], y[6], d[6];
    int k = 0;
    RG_UNROLL
    for (int i = 0; i < 6; i++) {
        RG_UNROLL
        for (int j = i; j < 6; j++) { M[i][j] = s[k]; M[j][i] = s[k]; k++; }
    }
    RG_UNROLL
    for (int i = 0; i < 6; i++) M[i][i] = M[i][i] + lambda * M[i][i] + RG_EPS;
    bool bad = false;
    RG_UNROLL
    for (int j = 0; j < 6; j++) {
        double v = M[j][j];
        RG_UNROLL
        for (int c = 0; c < j; c++) v = v - L[j][c] * L[j][c];
        if (!(v > 0.0)) bad = true;
        L[j][j] = sqrt(v);
        RG_UNROLL
        for (int i = j + 1; i < 6; i++) {
            double u = M[i][j];
            RG_UNROLL
            for (int c = 0; c < j; c++) u = u - L[i][c] * L[j][c];
            L[i][j] = u / L[j][j];
        }
    }
    if (bad) return RG_PIVOT;
    RG_UNROLL
    for (int i = 0; i < 6; i++) {
        double v = -s[21 + i];
        RG_UNROLL
        for (int c = 0; c < i; c++) v = v - L[i][c] * y[c];
        y[i] = v / L[i][i];
    }
    RG_UNROLL
    for (int i = 5; i >= 0; i--) {
        double v = y[i];
        RG_UNROLL
        for (int c = i + 1; c < 6; c++) v = v - L[c][i] * d[c];
        d[i] = v / L[i][i];
    }
    norms[0] = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    norms[1] = sqrt(d[3] * d[3] + d[4] * d[4] + d[5] * d[5]);
    if (!(norms[0] - norms[0] == 0.0 && norms[1] - norms[1] == 0.0)) { norms[0] = 0.0; norms[1] = 0.0; return RG_PIVOT; }     // a non-finite system
    if (norms[0] < tol_t && norms[1] < tol_r) return RG_CONVERGED;
    double Re[9], te[3], Y[12];
    sw_exp(d, Re, te);
    RG_UNROLL
    for (int i = 0; i < 3; i++) {
        RG_UNROLL
        for (int j = 0; j < 3; j++) Y[4 * i + j] = X[4 * i] * Re[j] + X[4 * i + 1] * Re[3 + j] + X[4 * i + 2] * Re[6 + j];
        Y[4 * i + 3] = X[4 * i] * te[0] + X[4 * i + 1] * te[1] + X[4 * i + 2] * te[2] + X[4 * i + 3];
    }
    RG_UNROLL
    for (int i = 0; i < 12; i++) X[i] = Y[i];
    return RG_OK;
}

#endif /* LRT_REG_MATH_H_INCLUDED */
