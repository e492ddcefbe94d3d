// lrt_actorsweep_math.h -- the rule of actors that move within a sweep (include/lrt_actorsweep.h), inline for host and device so that
// tests/host_check/actorsweep_check.cpp can compile it with g++ (-ffp-contract=off) and compare it with the float64 twin
// (lidar_rt_amd/actor_sweep.py).  It adds to lrt_sweepproj_math.h (sp_column_entry, sp_u, sp_column_of) and lrt_sweep_math.h (sw_exp, sw_coef)
// only what is new.  Everything is float64; the two float32 roundings are the stores of xyz_s and rot_s (and of the gradients).
//
//   as_pose         A = [Ra | ta] of a pose row (t, q, flag): the quaternion normalised as build_rotation does, in float64
//   as_table_entry  the column table: T_w = (P Exp(tau[w] xi))^-1 = sp_column_entry(xi, tau[w]) o world2sensor; an identity E_w keeps world2sensor
//   as_motion       E = Exp(s eta) = [Re | te]; false when s eta is zero in all six entries: E is EXACTLY the identity and nothing moves
//   as_search       sp_search's fixed-point iteration with a point that depends on the column: from the static column of A x at s = 0, at most
//                   AS_MAX_EVAL evaluations of "which column does column w see A Exp(tau[w] eta) x in"; always wrapped
//   as_quat         the unit quaternion of Re from phi' = s phi: (cos t, sin t / (2 t) phi'), t = |phi'| / 2; the series below SW_SERIES_TH2
//   as_place        xyz_s = float32(Re x + te), rot_s = float32(q_E (x) raw / max(|raw|, 1e-12)); the input's bits where nothing moves
//   as_place_bwd    the vector-Jacobian product of as_place at a fixed instant: d_xyz, d_rot_raw and the Gaussian's term of d_eta
//
// sw_exp has no contraction pragma of its own: the device may fuse its multiply-adds, so E can differ from the host's in its last bits.  The
// comparisons therefore rest on a margin of the inputs (every evaluated u stays away from its rounding boundary) and on a bound of 2^-40 of the
// absolute terms next to the float32 rounding.
#ifndef LRT_ACTORSWEEP_MATH_H_INCLUDED
#define LRT_ACTORSWEEP_MATH_H_INCLUDED

#include "lrt_sweepproj_math.h"

#define AS_MAX_EVAL 8           /* LRT_ACTORSWEEP_MAX_EVAL */
#define AS_TABLE 12             /* LRT_ACTORSWEEP_TABLE */
#define AS_NORM_EPS 1e-12       /* F.normalize's eps, as lrt_preprocess.hip */

#define AS_CONVERGED 0          /* how a search ended */
#define AS_UNCONVERGED 1
#define AS_INVALID 2

#define AS_HD PJ_HD

// row (8) float32 = (t, q, flag).  Returns whether the asset is posed.
AS_HD bool as_pose(const float* row, double* Ra, double* ta)
{
#pragma clang fp contract(off)
    for (int k = 0; k < 3; k++) ta[k] = (double)row[k];
    const double q0 = (double)row[3], q1 = (double)row[4], q2 = (double)row[5], q3 = (double)row[6];
    const double n = sqrt(q0 * q0 + q1 * q1 + q2 * q2 + q3 * q3);
    const double r = q0 / n, x = q1 / n, y = q2 / n, z = q3 / n;
    Ra[0] = 1.0 - 2.0 * (y * y + z * z); Ra[1] = 2.0 * (x * y - r * z);       Ra[2] = 2.0 * (x * z + r * y);
    Ra[3] = 2.0 * (x * y + r * z);       Ra[4] = 1.0 - 2.0 * (x * x + z * z); Ra[5] = 2.0 * (y * z - r * x);
    Ra[6] = 2.0 * (x * z - r * y);       Ra[7] = 2.0 * (y * z + r * x);       Ra[8] = 1.0 - 2.0 * (x * x + y * y);
    return row[7] != 0.f;
}

// y = R x + t, R row-major 3 x 3, each row summed left to right
AS_HD void as_rigid(const double* R, const double* t, const double* x, double* y)
{
#pragma clang fp contract(off)
    y[0] = R[0] * x[0] + R[1] * x[1] + R[2] * x[2] + t[0];
    y[1] = R[3] * x[0] + R[4] * x[1] + R[5] * x[2] + t[1];
    y[2] = R[6] * x[0] + R[7] * x[1] + R[8] * x[2] + t[2];
}

// q = T (y, 1), T row-major 3 x 4, each row summed left to right
AS_HD void as_apply(const double* T, const double* y, double* q)
{
#pragma clang fp contract(off)
    q[0] = T[0] * y[0] + T[1] * y[1] + T[2] * y[2] + T[3];
    q[1] = T[4] * y[0] + T[5] * y[1] + T[6] * y[2] + T[7];
    q[2] = T[8] * y[0] + T[9] * y[1] + T[10] * y[2] + T[11];
}

// T (12): world -> the sensor frame of the column whose instant is s.  w2s (12) = P^-1; xi (6) the sensor's twist or null (a static sensor).
AS_HD void as_table_entry(const double* w2s, const double* xi, double s, double* T)
{
#pragma clang fp contract(off)
    double E[SP_TABLE];
    bool moved = false;
    if (xi) {
        sp_column_entry(xi, s, E);
        moved = !sp_is_identity(E);
    }
    if (!moved) {
        for (int k = 0; k < AS_TABLE; k++) T[k] = w2s[k];
        return;
    }
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) T[4 * i + j] = E[4 * i] * w2s[j] + E[4 * i + 1] * w2s[4 + j] + E[4 * i + 2] * w2s[8 + j];
        T[4 * i + 3] = E[4 * i] * w2s[3] + E[4 * i + 1] * w2s[7] + E[4 * i + 2] * w2s[11] + E[4 * i + 3];
    }
}

// xs = s eta and, unless all of it is zero, E = Exp(xs).  Returns whether anything moves.
AS_HD bool as_motion(const double* eta, double s, double* xs, double* Re, double* te)
{
#pragma clang fp contract(off)
    bool zero = true;
    for (int k = 0; k < 6; k++) {
        xs[k] = s * eta[k];
        zero = zero && xs[k] == 0.0;
    }
    if (zero) return false;
    sw_exp(xs, Re, te);
    return true;
}

// A point the column rule can be asked about: finite and off the z axis.
AS_HD bool as_usable(const double* q)
{
    return pj_finite(q[0]) && pj_finite(q[1]) && pj_finite(q[2]) && !(q[0] == 0.0 && q[1] == 0.0);
}

// x: the centre in the actor's frame.  table: R.W entries of AS_TABLE doubles; tau: R.W instants.  Returns how the search ended; *col is the
// LAST evaluated column (-1 for AS_INVALID), *evals the evaluations used (0 when the point at s = 0 is already unusable).
AS_HD int as_search(const double* x, const double* Ra, const double* ta, const double* eta, const double* w2s, const double* table, const double* tau,
                    const PjRule& R, int* col_out, int* evals)
{
#pragma clang fp contract(off)
    double y[3], q[3], e[3], xs[6], Re[9], te[3];
    *col_out = -1; *evals = 0;
    as_rigid(Ra, ta, x, y);
    as_apply(w2s, y, q);
    if (!as_usable(q)) return AS_INVALID;
    int col = sp_column_of(rint(sp_u(q, R)), R);                   // within [0, W) whatever u holds
    int n = 0, state = AS_UNCONVERGED;
    for (;;) {
        if (as_motion(eta, tau[col], xs, Re, te)) as_rigid(Re, te, x, e);
        else { e[0] = x[0]; e[1] = x[1]; e[2] = x[2]; }
        as_rigid(Ra, ta, e, y);
        as_apply(table + AS_TABLE * (long long)col, y, q);
        n++;
        if (!as_usable(q)) { *evals = n; return AS_INVALID; }
        const int next = sp_column_of(rint(sp_u(q, R)), R);
        if (next == col) { state = AS_CONVERGED; break; }
        if (n == AS_MAX_EVAL) break;
        col = next;
    }
    *col_out = col; *evals = n;
    return state;
}

// c = (cos t, sin t / t, d cos t / du, d (sin t / t) / du) at u = t^2
AS_HD void as_half_coef(double u, double* c)
{
    if (u < SW_SERIES_TH2) {
        sw_nested(u, -1, c + 0, c + 2);
        sw_nested(u, 0, c + 1, c + 3);
    } else {
        const double t = sqrt(u);
        double sn, cs;
        sincos(t, &sn, &cs);
        c[0] = cs;
        c[1] = sn / t;
        c[2] = -0.5 * c[1];
        c[3] = (cs - c[1]) / (2.0 * u);
    }
}

// qe (4, real part first): the unit quaternion of Exp's rotation at phi; c: as_half_coef at |phi|^2 / 4
AS_HD void as_quat(const double* phi, double* qe, double* c)
{
    as_half_coef(0.25 * (phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2]), c);
    qe[0] = c[0];
    for (int k = 0; k < 3; k++) qe[1 + k] = 0.5 * c[1] * phi[k];
}

// One Gaussian at the instant s.  Returns whether it moved; otherwise the outputs are the inputs bit for bit (rot_raw NOT normalised).
AS_HD bool as_place(const double* eta, double s, const float* xf, const float* rf, float* xo, float* ro)
{
#pragma clang fp contract(off)
    double xs[6], Re[9], te[3];
    if (!as_motion(eta, s, xs, Re, te)) {
        for (int k = 0; k < 3; k++) xo[k] = xf[k];
        for (int k = 0; k < 4; k++) ro[k] = rf[k];
        return false;
    }
    const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]};
    double e[3], qe[4], c[4];
    as_rigid(Re, te, x, e);
    for (int k = 0; k < 3; k++) xo[k] = (float)e[k];
    as_quat(xs + 3, qe, c);
    const double r0 = (double)rf[0], r1 = (double)rf[1], r2 = (double)rf[2], r3 = (double)rf[3];
    const double n = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const double d = n > AS_NORM_EPS ? n : AS_NORM_EPS;
    const double bw = r0 / d, bx = r1 / d, by = r2 / d, bz = r3 / d;
    ro[0] = (float)(qe[0] * bw - qe[1] * bx - qe[2] * by - qe[3] * bz);
    ro[1] = (float)(qe[0] * bx + qe[1] * bw + qe[2] * bz - qe[3] * by);
    ro[2] = (float)(qe[0] * by - qe[1] * bz + qe[2] * bw + qe[3] * bx);
    ro[3] = (float)(qe[0] * bz + qe[1] * by - qe[2] * bx + qe[3] * bw);
    return true;
}

// The backward of as_place at the fixed instant s: g (3) = dL/dxyz_s, h (4) = dL/drot_s.  dx (3), dr (4): the gradients of xyz and rot_raw;
// deta (6): this Gaussian's term of dL/deta (zero when nothing moved: then dx = g and dr = h).
//   through Exp at xs = s eta, with M = dL/dRe = g x^T and q = dL/dte = g (the chain of sw_column_bwd):
//   d rho' = V^T q;  dK = A M + B q rho'^T + X K^T + K^T X with X = B M + C q rho'^T;
//   d phi' = vee(dK - dK^T) + 2 phi' (A' <M, K> + B' (<M, K^2> + q . K rho') + C' q . K^2 rho');
//   through the quaternion: d phi' += a dq_v / 2 + phi' (c' dq_w + a' (dq_v . phi') / 2) / 2 with dq = J^T(b) h;   d eta = s d xs.
AS_HD bool as_place_bwd(const double* eta, double s, const float* xf, const float* rf, const double* g, const double* h, double* dx, double* dr, double* deta)
{
#pragma clang fp contract(off)
    double xs[6];
    bool zero = true;
    for (int k = 0; k < 6; k++) {
        xs[k] = s * eta[k];
        zero = zero && xs[k] == 0.0;
        deta[k] = 0.0;
    }
    if (zero) {
        for (int k = 0; k < 3; k++) dx[k] = g[k];
        for (int k = 0; k < 4; k++) dr[k] = h[k];
        return false;
    }
    const double* rho = xs; const double* phi = xs + 3;
    const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]};
    double c[6], K[9], K2[9], Re[9], V[9];
    sw_coef(phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2], c);
    sw_hat(phi, K, K2);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            const double e = (i == j) ? 1.0 : 0.0;
            Re[3 * i + j] = e + c[0] * K[3 * i + j] + c[1] * K2[3 * i + j];
            V[3 * i + j] = e + c[1] * K[3 * i + j] + c[2] * K2[3 * i + j];
        }
    for (int j = 0; j < 3; j++) dx[j] = Re[j] * g[0] + Re[3 + j] * g[1] + Re[6 + j] * g[2];
    double M[9], dxs[6], Kr[3], K2r[3], X[9], dK[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) M[3 * i + j] = g[i] * x[j];
    for (int j = 0; j < 3; j++) dxs[j] = V[j] * g[0] + V[3 + j] * g[1] + V[6 + j] * g[2];
    sw_cross(phi, rho, Kr);
    sw_cross(phi, Kr, K2r);
    double mk = 0.0, mk2 = 0.0;
    for (int i = 0; i < 9; i++) { mk += M[i] * K[i]; mk2 += M[i] * K2[i]; }
    const double du = c[3] * mk + c[4] * (mk2 + g[0] * Kr[0] + g[1] * Kr[1] + g[2] * Kr[2]) + c[5] * (g[0] * K2r[0] + g[1] * K2r[1] + g[2] * K2r[2]);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) X[3 * i + j] = c[1] * M[3 * i + j] + c[2] * g[i] * rho[j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double v = c[0] * M[3 * i + j] + c[1] * g[i] * rho[j];
            for (int k = 0; k < 3; k++) v += X[3 * i + k] * K[3 * j + k] + K[3 * k + i] * X[3 * k + j];
            dK[3 * i + j] = v;
        }
    dxs[3] = dK[7] - dK[5] + 2.0 * phi[0] * du;
    dxs[4] = dK[2] - dK[6] + 2.0 * phi[1] * du;
    dxs[5] = dK[3] - dK[1] + 2.0 * phi[2] * du;
    // the rotation: out = qe (x) b, b = raw / max(|raw|, eps)
    double qe[4], hc[4];
    as_quat(phi, qe, hc);
    const double r0 = (double)rf[0], r1 = (double)rf[1], r2 = (double)rf[2], r3 = (double)rf[3];
    const double n = sqrt(r0 * r0 + r1 * r1 + r2 * r2 + r3 * r3);
    const double d = n > AS_NORM_EPS ? n : AS_NORM_EPS;
    const double bw = r0 / d, bx = r1 / d, by = r2 / d, bz = r3 / d;
    double dq[4], db[4];
    dq[0] =  bw * h[0] + bx * h[1] + by * h[2] + bz * h[3];
    dq[1] = -bx * h[0] + bw * h[1] - bz * h[2] + by * h[3];
    dq[2] = -by * h[0] + bz * h[1] + bw * h[2] - bx * h[3];
    dq[3] = -bz * h[0] - by * h[1] + bx * h[2] + bw * h[3];
    db[0] =  qe[0] * h[0] + qe[1] * h[1] + qe[2] * h[2] + qe[3] * h[3];
    db[1] = -qe[1] * h[0] + qe[0] * h[1] + qe[3] * h[2] - qe[2] * h[3];
    db[2] = -qe[2] * h[0] - qe[3] * h[1] + qe[0] * h[2] + qe[1] * h[3];
    db[3] = -qe[3] * h[0] + qe[2] * h[1] - qe[1] * h[2] + qe[0] * h[3];
    const double dqp = dq[1] * phi[0] + dq[2] * phi[1] + dq[3] * phi[2];
    const double duh = hc[2] * dq[0] + 0.5 * hc[3] * dqp;          // dL/du_h, u_h = |phi'|^2 / 4
    for (int k = 0; k < 3; k++) dxs[3 + k] += 0.5 * hc[1] * dq[1 + k] + 0.5 * phi[k] * duh;
    if (n > AS_NORM_EPS) {                                         // d(raw) = (d(b) - b (b . d(b))) / |raw|
        const double dot = bw * db[0] + bx * db[1] + by * db[2] + bz * db[3];
        dr[0] = (db[0] - bw * dot) / n; dr[1] = (db[1] - bx * dot) / n; dr[2] = (db[2] - by * dot) / n; dr[3] = (db[3] - bz * dot) / n;
    } else {
        for (int k = 0; k < 4; k++) dr[k] = db[k] / AS_NORM_EPS;
    }
    for (int k = 0; k < 6; k++) deta[k] = s * dxs[k];
    return true;
}

#endif /* LRT_ACTORSWEEP_MATH_H_INCLUDED */
