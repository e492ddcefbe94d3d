// lrt_beams_math.h -- the rule of the beam rays (include/lrt_beams.h): the one text for the device (lrt_beams.hip) and the host
// (tests/host_check/beams_check.cpp).  All of it float64; the only roundings to float32 are the stores of the results.
//
// Row h of the image has two offsets (eps_h, delta_h) = beams[h] (NOT flipped, unlike the inclination table):
//   e = sw_inclination(h) + eps_h,  a = sw_azimuth(w) + delta_h,  l = (cos e cos a, cos e sin a, sin e),  ray_d = R_w l / |R_w l|,  ray_o = t_w.
//
// The elevation takes the angle sum: one sincos per row.  The azimuth takes the product form, which keeps a per-column and a per-row table:
//   cos a = ca cd - sa sd, sin a = sa cd + ca sd  with (ca, sa) of the column's nominal azimuth and (cd, sd) = (cos, sin)(delta_h), so that
//   R_w (cos a, sin a, 0) = cd A + sd B,  A = R_w (ca, sa, 0),  B = R_w (-sa, ca, 0)  -- the third axis next to sw_column_axes's two.
// A row with delta_h == 0 exactly has (cd, sd) = (1, 0) exactly and takes A itself (bm_row_axis), and cos(e + 0) is cos(e): such a row carries
// the bits of the sweep rays.  The product form's error is a few 2^-53 of a unit vector, far inside the float32 store.
//
// Backward.  With gv = dL/dv of a ray (sw_ray_bwd), v = ci a_h + si c, a_h = cd A + sd B, b_h = cd B - sd A, (ci, si) = (cos, sin)(e):
//   d eps_h   = sum_{f, w} gv . (ci c - si a_h)                    d delta_h = sum_{f, w} ci gv . b_h
//   dL/dR_w   = sum_h gv l^T = [ca Gp - sa Gq | sa Gp + ca Gq | Gc],  Gp = sum_h (ci cd) gv, Gq = sum_h (ci sd) gv, Gc = sum_h si gv
// -- three sums per column instead of the sweep rays' two; with a zero table Gp is the sweep rays' Ga bit for bit and Gq is zero.
#ifndef LRT_BEAMS_MATH_H_INCLUDED
#define LRT_BEAMS_MATH_H_INCLUDED

#include "lrt_sweep_math.h"

// One row's four numbers: r = (cos e, sin e, cos delta, sin delta), e = the nominal inclination + eps.  beams (H, 2) float32, read at row h.
SW_HD void bm_row(int h, int H, const float* inc, int n_inc, double off, const float* beams, double* r)
{
    sincos(sw_inclination(h, H, inc, n_inc, off) + (double)beams[2 * h], r + 1, r + 0);
    sincos((double)beams[2 * h + 1], r + 3, r + 2);
}

// The column's third axis: B = R (-sa, ca, 0)
SW_HD void bm_column_axis(const double* R, double ca, double sa, double* B)
{
    for (int i = 0; i < 3; i++) B[i] = R[3 * i + 1] * ca - R[3 * i] * sa;
}

// a_h = cd A + sd B; A itself for a row without an azimuth offset (the bits of the sweep rays, the sign of a zero included)
SW_HD void bm_row_axis(const double* A, const double* B, double cd, double sd, double* a)
{
    const bool plain = (cd == 1.0) && (sd == 0.0);
    for (int i = 0; i < 3; i++) a[i] = plain ? A[i] : cd * A[i] + sd * B[i];
}

// One ray's two beam terms from gv: *ge = gv . (ci c - si a_h), *gd = ci gv . b_h with b_h = cd B - sd A
SW_HD void bm_ray_beam_bwd(const double* A, const double* B, const double* c, const double* a_h, const double* r, const double* gv, double* ge, double* gd)
{
    double e = 0.0, d = 0.0;
    for (int i = 0; i < 3; i++) {
        e += gv[i] * (r[0] * c[i] - r[1] * a_h[i]);
        d += gv[i] * (r[2] * B[i] - r[3] * A[i]);
    }
    *ge = e; *gd = r[0] * d;
}

// One column's contribution to d_pose (12, row-major 3 x 4) and d_twist (6), ADDED to them, from dL/dR_w (row-major 3 x 3) and dL/dt_w = Gt:
// the chain of sw_column_bwd (its comment has the formulas) behind the point where that one forms [ca Ga | sa Ga | Gc].  The text from there on
// is sw_column_bwd's, statement for statement, so that equal dR give equal bits; lrt_sweep_math.h itself stays as it is.
SW_HD void bm_column_bwd_dR(const float* P, const float* xi, double s, const double* dR, const double* Gt, double* d_pose, double* d_twist)
{
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

// One column's contribution from its three sums (see above) and Gt = sum_h g_o.
SW_HD void bm_column_bwd(const float* P, const float* xi, double s, double ca, double sa, const double* Gp, const double* Gq, const double* Gc,
                         const double* Gt, double* d_pose, double* d_twist)
{
    double dR[9];
    for (int i = 0; i < 3; i++) { dR[3 * i] = ca * Gp[i] - sa * Gq[i]; dR[3 * i + 1] = sa * Gp[i] + ca * Gq[i]; dR[3 * i + 2] = Gc[i]; }
    bm_column_bwd_dR(P, xi, s, dR, Gt, d_pose, d_twist);
}

#endif /* LRT_BEAMS_MATH_H_INCLUDED */
