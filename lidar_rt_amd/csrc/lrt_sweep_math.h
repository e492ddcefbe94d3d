// lrt_sweep_math.h -- the rule of the sweep rays (include/lrt_sweep.h): the one text for the device (lrt_sweep.hip) and the host
// (tests/host_check/sweep_check.cpp).  All of it float64; the only roundings to float32 are the stores of the results.
//
//   T_f(s) = P_f Exp(s xi_f),  xi = (rho, phi) in the sensor frame (poses.se3_exp):  Exp = [I + A K + B K^2 | (I + B K + C K^2) rho],
//   K = hat(phi), u = |phi|^2, A = sin t / t, B = (1 - cos t) / t^2, C = (t - sin t) / t^3 with t = sqrt(u).
//
// Below SW_SERIES_TH2 the three coefficients and their derivatives by u come from their series, above it from the closed forms.  The threshold
// is as large as 0.25 (half a radian) on purpose: the closed derivative (B - 3 C) / (2 u) loses |log2 u| bits to cancellation, and at 0.25 the two
// branches still agree to better than 2^-45 (ten terms of the series leave less than 1e-18 there).
#ifndef LRT_SWEEP_MATH_H_INCLUDED
#define LRT_SWEEP_MATH_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SW_HD __host__ __device__ __forceinline__
#else
#define SW_HD static inline
#endif

#define SW_SERIES_TH2 0.25      /* u = |s phi|^2 below this: the series */
#define SW_SERIES_TERMS 10
#define SW_TWO_PI 6.28318530717958647692
#define SW_PI 3.14159265358979323846

// sum_k (-1)^k u^k (j + 1)! / (2 k + 1 + j)!  as  1 - u / m_0 (1 - u / m_1 (...)),  m_k = (2 k + 2 + j)(2 k + 3 + j); and its derivative by u.
SW_HD void sw_nested(double u, int j, double* val, double* der)
{
    double v = 1.0, d = 0.0;
    for (int k = SW_SERIES_TERMS - 1; k >= 0; k--) {
        const double m = (double)((2 * k + 2 + j) * (2 * k + 3 + j));
        d = -(v + u * d) / m;
        v = 1.0 - u * v / m;
    }
    *val = v; *der = d;
}

// c = (A, B, C, dA/du, dB/du, dC/du)
SW_HD void sw_coef_series(double u, double* c)
{
    sw_nested(u, 0, c + 0, c + 3);
    sw_nested(u, 1, c + 1, c + 4);
    sw_nested(u, 2, c + 2, c + 5);
    c[1] *= 0.5; c[4] *= 0.5;
    c[2] /= 6.0; c[5] /= 6.0;
}

SW_HD void sw_coef_closed(double u, double* c)
{
    const double t = sqrt(u);
    double sn, cs;
    sincos(t, &sn, &cs);
    c[0] = sn / t;
    c[1] = (1.0 - cs) / u;
    c[2] = (t - sn) / (u * t);
    c[3] = (cs - c[0]) / (2.0 * u);
    c[4] = (c[0] - 2.0 * c[1]) / (2.0 * u);
    c[5] = (c[1] - 3.0 * c[2]) / (2.0 * u);
}

SW_HD void sw_coef(double u, double* c)
{
    if (u < SW_SERIES_TH2) sw_coef_series(u, c); else sw_coef_closed(u, c);
}

// y = K x, K = hat(p)
SW_HD void sw_cross(const double* p, const double* x, double* y)
{
    y[0] = p[1] * x[2] - p[2] * x[1];
    y[1] = p[2] * x[0] - p[0] * x[2];
    y[2] = p[0] * x[1] - p[1] * x[0];
}

// K = hat(p) and K^2, row-major 3 x 3
SW_HD void sw_hat(const double* p, double* K, double* K2)
{
    K[0] = 0.0; K[1] = -p[2]; K[2] = p[1];
    K[3] = p[2]; K[4] = 0.0; K[5] = -p[0];
    K[6] = -p[1]; K[7] = p[0]; K[8] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
}

// Exp of x = (rho, phi): Re row-major 3 x 3, te 3.
SW_HD void sw_exp(const double* x, double* Re, double* te)
{
    const double* rho = x; const double* phi = x + 3;
    double c[6], K[9], K2[9];
    sw_coef(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2], c);
    sw_hat(phi, K, K2);
    for (int i = 0; i < 3; i++) {
        double t = 0.0;
        for (int j = 0; j < 3; j++) {
            const double e = (i == j) ? 1.0 : 0.0;
            Re[3 * i + j] = e + c[0] * K[3 * i + j] + c[1] * K2[3 * i + j];
            t += (e + c[1] * K[3 * i + j] + c[2] * K2[3 * i + j]) * rho[j];
        }
        te[i] = t;
    }
}

// The pose of a column: T = P Exp(s xi).  P (3, 4) row-major float32; xi float32 or null (a static sensor).  R row-major 3 x 3, t 3.
SW_HD void sw_column_pose(const float* P, const float* xi, double s, double* R, double* t)
{
    if (!xi) {
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) R[3 * i + j] = (double)P[4 * i + j];
            t[i] = (double)P[4 * i + 3];
        }
        return;
    }
    double x[6], Re[9], te[3];
    for (int k = 0; k < 6; k++) x[k] = s * (double)xi[k];
    sw_exp(x, Re, te);
    for (int i = 0; i < 3; i++) {
        const double p0 = (double)P[4 * i], p1 = (double)P[4 * i + 1], p2 = (double)P[4 * i + 2];
        for (int j = 0; j < 3; j++) R[3 * i + j] = p0 * Re[j] + p1 * Re[3 + j] + p2 * Re[6 + j];
        t[i] = p0 * te[0] + p1 * te[1] + p2 * te[2] + (double)P[4 * i + 3];
    }
}

SW_HD double sw_azimuth(int w, int W, double off, double yaw)
{
    return ((double)(W - w) - off) / (double)W * SW_TWO_PI - SW_PI - yaw;
}

// inc: two bounds (n_inc == 2) or the flipped per-beam table (row h reads inc[H - 1 - h])
SW_HD double sw_inclination(int h, int H, const float* inc, int n_inc, double off)
{
    if (n_inc == 2) return ((double)(H - h) - off) / (double)H * ((double)inc[1] - (double)inc[0]) + (double)inc[0];
    return (double)inc[H - 1 - h];
}

// The column's part of a direction: a = R (cos az, sin az, 0), c = R (0, 0, 1); a ray of row h is v = cos(inc) a + sin(inc) c, d = v / |v|.
SW_HD void sw_column_axes(const double* R, double ca, double sa, double* a, double* c)
{
    for (int i = 0; i < 3; i++) {
        a[i] = R[3 * i] * ca + R[3 * i + 1] * sa;
        c[i] = R[3 * i + 2];
    }
}

SW_HD void sw_ray(const double* a, const double* c, double ci, double si, double* d, double* n_out)
{
    const double v0 = ci * a[0] + si * c[0], v1 = ci * a[1] + si * c[1], v2 = ci * a[2] + si * c[2];
    const double n = sqrt(v0 * v0 + v1 * v1 + v2 * v2);
    d[0] = v0 / n; d[1] = v1 / n; d[2] = v2 / n;
    *n_out = n;
}

// dL/dv of d = v / |v| from dL/dd = g:  (g - d (d . g)) / n
SW_HD void sw_ray_bwd(const double* d, double n, const double* g, double* gv)
{
    const double dg = d[0] * g[0] + d[1] * g[1] + d[2] * g[2];
    for (int i = 0; i < 3; i++) gv[i] = (g[i] - d[i] * dg) / n;
}

// One column's contribution to d_pose (12, row-major 3 x 4) and d_twist (6), ADDED to them.  Ga = sum_h cos(inc) gv, Gc = sum_h sin(inc) gv,
// Gt = sum_h g_o: then dL/dR_w = [ca Ga | sa Ga | Gc] and dL/dt_w = Gt.  With R_w = Rp Re, t_w = Rp te + tp:
//   dRp = dR_w Re^T + Gt te^T, dtp = Gt, M = dRe = Rp^T dR_w, q = dte = Rp^T Gt, and through Exp at x = s xi:
//   d rho' = V^T q;  dK = A M + B q rho'^T + X K^T + K^T X with X = B M + C q rho'^T;  d phi' = vee(dK - dK^T) + 2 phi' (A' <M, K> + B' (<M, K^2> + q . K rho') + C' q . K^2 rho');
//   d xi = s d xi'.
SW_HD void sw_column_bwd(const float* P, const float* xi, double s, double ca, double sa, const double* Ga, const double* Gc, const double* Gt,
                         double* d_pose, double* d_twist)
{
    double dR[9];
    for (int i = 0; i < 3; i++) { dR[3 * i] = ca * Ga[i]; dR[3 * i + 1] = sa * Ga[i]; dR[3 * i + 2] = Gc[i]; }
    if (!xi) {
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) d_pose[4 * i + j] += dR[3 * i + j];
            d_pose[4 * i + 3] += Gt[i];
        }
        return;
    }
    double x[6], c[6], K[9], K2[9], Re[9], V[9], te[3];
    for (int k = 0; k < 6; k++) x[k] = s * (double)xi[k];
    const double* rho = x; const double* phi = x + 3;
    sw_coef(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2], c);
    sw_hat(phi, K, K2);
    for (int i = 0; i < 3; i++) {
        double t = 0.0;
        for (int j = 0; j < 3; j++) {
            const double e = (i == j) ? 1.0 : 0.0;
            Re[3 * i + j] = e + c[0] * K[3 * i + j] + c[1] * K2[3 * i + j];
            V[3 * i + j] = e + c[1] * K[3 * i + j] + c[2] * K2[3 * i + j];
            t += V[3 * i + j] * rho[j];
        }
        te[i] = t;
    }
    double M[9], q[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            d_pose[4 * i + j] += dR[3 * i] * Re[3 * j] + dR[3 * i + 1] * Re[3 * j + 1] + dR[3 * i + 2] * Re[3 * j + 2] + Gt[i] * te[j];
            M[3 * i + j] = (double)P[i] * dR[j] + (double)P[4 + i] * dR[3 + j] + (double)P[8 + i] * dR[6 + j];
        }
        d_pose[4 * i + 3] += Gt[i];
        q[i] = (double)P[i] * Gt[0] + (double)P[4 + i] * Gt[1] + (double)P[8 + i] * Gt[2];
    }
    double dx[6], Kr[3], K2r[3], X[9], dK[9];
    for (int j = 0; j < 3; j++) dx[j] = V[j] * q[0] + V[3 + j] * q[1] + V[6 + j] * q[2];
    sw_cross(phi, rho, Kr);
    sw_cross(phi, Kr, K2r);
    double mk = 0.0, mk2 = 0.0;
    for (int i = 0; i < 9; i++) { mk += M[i] * K[i]; mk2 += M[i] * K2[i]; }
    const double du = c[3] * mk + c[4] * (mk2 + q[0] * Kr[0] + q[1] * Kr[1] + q[2] * Kr[2]) + c[5] * (q[0] * K2r[0] + q[1] * K2r[1] + q[2] * K2r[2]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) X[3 * i + j] = c[1] * M[3 * i + j] + c[2] * q[i] * rho[j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = c[0] * M[3 * i + j] + c[1] * q[i] * rho[j];
            for (int k = 0; k < 3; k++) v += X[3 * i + k] * K[3 * j + k] + K[3 * k + i] * X[3 * k + j];
            dK[3 * i + j] = v;
        }
    dx[3] = dK[7] - dK[5] + 2.0 * phi[0] * du;
    dx[4] = dK[2] - dK[6] + 2.0 * phi[1] * du;
    dx[5] = dK[3] - dK[1] + 2.0 * phi[2] * du;
    for (int k = 0; k < 6; k++) d_twist[k] += s * dx[k];
}

#endif /* LRT_SWEEP_MATH_H_INCLUDED */
