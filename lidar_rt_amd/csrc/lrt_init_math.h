// lrt_init_math.h -- the arithmetic contract of the scene-initialisation operators (include/lrt_init.h), inline for host and device so that
// tests/host_check/init_check.cpp can compile it with g++ and compare it with numpy.
//
//   point, pair distance, tile bound   those of the grid Chamfer operator (lrt_gridcd_math.h: gc_point, gc_d2, gc_bound, gc_bound_box), unchanged
//   in_smallest_eigenvector   unit eigenvector of the smallest eigenvalue of a symmetric 3 x 3 matrix, closed form, float64.  The eigenvalues
//             come from the trigonometric solution of the characteristic cubic of the matrix scaled to a largest entry of 1.  That solution is
//             accurate for the eigenvalue at the SEPARATED end of the spectrum only (the largest when det(B) >= 0, the smallest otherwise; the
//             acos loses half the digits of the close pair), so only that eigenvalue is used: its vector is the largest cross product of two rows
//             of A - l I.  If it is the smallest, that is the answer; if it is the largest, the answer is the smaller eigenvector of the 2 x 2
//             problem in its orthogonal complement, solved directly.  A flat neighbourhood (l0 << l1 ~ l2) and a needle (l0 ~ l1 << l2)
//             both keep the accuracy the conditioning allows, ~ 2^-53 l2 / (l1 - l0) in angle.  `lam` is informative (the close pair to ~1e-8 l2).
//             Returns 0 for a matrix of rank < 2 (the largest cross product of two ROWS OF A is below IN_RANK_TOL^2 for the scaled matrix:
//             l1 l2 <= ~1e-14 l2^2) or a non-finite one, and leaves the vector at (0, 0, 1): the fall-back of the normal estimation.
//   in_covariance   mean and covariance (divided by n) of n <= 8 points, float64, summed in list order
//   in_face_sensor  the sign rule: the float32-rounded normal n faces the sensor, n . (o - p) >= 0 in float64 (products of float32 values are
//             exact there); at exactly 0 the first non-zero component is positive
#ifndef LRT_INIT_MATH_H_INCLUDED
#define LRT_INIT_MATH_H_INCLUDED

#include <math.h>
#include "lrt_gridcd_math.h"

#define IN_HD GC_HD
#if defined(__clang__)
#define IN_UNROLL _Pragma("unroll")
#else
#define IN_UNROLL
#endif
#define IN_KMAX 8
#define IN_RANK_TOL 1e-14

IN_HD void in_cross(const double* a, const double* b, double* c)
{
    c[0] = a[1] * b[2] - a[2] * b[1]; c[1] = a[2] * b[0] - a[0] * b[2]; c[2] = a[0] * b[1] - a[1] * b[0];
}

IN_HD double in_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// Unit null vector of the rank-2 matrix M = A - l I (A = [a00 a01 a02; a01 a11 a12; a02 a12 a22]): the largest of the three row cross products.
// Returns its squared norm before normalisation (0: M has rank < 2, v untouched).
IN_HD double in_null_vector(double a00, double a01, double a02, double a11, double a12, double a22, double l, double* v)
{
    const double r0[3] = {a00 - l, a01, a02}, r1[3] = {a01, a11 - l, a12}, r2[3] = {a02, a12, a22 - l};
    double c01[3], c02[3], c12[3];
    in_cross(r0, r1, c01); in_cross(r0, r2, c02); in_cross(r1, r2, c12);
    const double d01 = in_dot(c01, c01), d02 = in_dot(c02, c02), d12 = in_dot(c12, c12);
    double cx = c01[0], cy = c01[1], cz = c01[2], dm = d01;
    if (d02 > dm) { cx = c02[0]; cy = c02[1]; cz = c02[2]; dm = d02; }
    if (d12 > dm) { cx = c12[0]; cy = c12[1]; cz = c12[2]; dm = d12; }
    if (!(dm > 0.0)) return 0.0;
    const double s = 1.0 / sqrt(dm);
    v[0] = cx * s; v[1] = cy * s; v[2] = cz * s;
    return dm;
}

// Two unit vectors u, v with (u, v, w) a right-handed orthonormal basis, w a unit vector.
IN_HD void in_complement(const double* w, double* u, double* v)
{
    if (fabs(w[0]) > fabs(w[1])) { const double s = 1.0 / sqrt(w[0] * w[0] + w[2] * w[2]); u[0] = -w[2] * s; u[1] = 0.0; u[2] = w[0] * s; }
    else { const double s = 1.0 / sqrt(w[1] * w[1] + w[2] * w[2]); u[0] = 0.0; u[1] = w[2] * s; u[2] = -w[1] * s; }
    in_cross(w, u, v);
}

// Unit eigenvector of the SMALLER eigenvalue of A restricted to the plane orthogonal to the unit eigenvector w (of the largest eigenvalue): the
// 2 x 2 problem [a b; b c] in a basis (u, v) of that plane, solved directly -- no eigenvalue of the close pair enters.
IN_HD void in_smallest_in_complement(double a00, double a01, double a02, double a11, double a12, double a22, const double* w, double* out)
{
    double u[3], v[3];
    in_complement(w, u, v);
    const double au[3] = {a00 * u[0] + a01 * u[1] + a02 * u[2], a01 * u[0] + a11 * u[1] + a12 * u[2], a02 * u[0] + a12 * u[1] + a22 * u[2]};
    const double av[3] = {a00 * v[0] + a01 * v[1] + a02 * v[2], a01 * v[0] + a11 * v[1] + a12 * v[2], a02 * v[0] + a12 * v[1] + a22 * v[2]};
    const double a = in_dot(u, au), b = in_dot(u, av), c = in_dot(v, av);
    const double h = 0.5 * (a - c), r = sqrt(h * h + b * b);
    // (M - l_min I) x = 0 with l_min = (a + c) / 2 - r: the row whose diagonal entry |h| + r has no cancellation
    double x = 1.0, y = 0.0;                                   // r = 0 (a double eigenvalue): any vector of the plane
    if (r > 0.0) {
        if (h >= 0.0) { x = -b; y = h + r; } else { x = r - h; y = -b; }
        const double s = 1.0 / sqrt(x * x + y * y);
        x *= s; y *= s;
    }
    out[0] = x * u[0] + y * v[0]; out[1] = x * u[1] + y * v[1]; out[2] = x * u[2] + y * v[2];
}

// c = (xx, xy, xz, yy, yz, zz).  n: the unit eigenvector of the smallest eigenvalue; lam (may be null): the three eigenvalues, ascending.
// Returns 1, or 0 with n = (0, 0, 1) for a matrix of rank < 2 or with a non-finite entry.
IN_HD int in_smallest_eigenvector(const double* c, double* n, double* lam)
{
    n[0] = 0.0; n[1] = 0.0; n[2] = 1.0;
    if (lam) { lam[0] = 0.0; lam[1] = 0.0; lam[2] = 0.0; }
    double mx = 0.0;
    bool nan = false;
    IN_UNROLL
    for (int i = 0; i < 6; i++) { const double a = fabs(c[i]); if (a > mx) mx = a; nan = nan || !(a == a); }
    if (nan) return 0;
    if (!(mx > 0.0) || !(mx < INFINITY)) return 0;
    const double inv = 1.0 / mx;
    const double a00 = c[0] * inv, a01 = c[1] * inv, a02 = c[2] * inv, a11 = c[3] * inv, a12 = c[4] * inv, a22 = c[5] * inv;
    // rank: the largest cross product of two rows of A itself (l1 l2 up to a factor of the basis)
    double tmp[3];
    if (!(in_null_vector(a00, a01, a02, a11, a12, a22, 0.0, tmp) > IN_RANK_TOL * IN_RANK_TOL)) return 0;
    const double off2 = a01 * a01 + a02 * a02 + a12 * a12;
    double l0, l1, l2, half_det = 0.0;
    if (off2 > 0.0) {
        const double q = (a00 + a11 + a22) / 3.0;
        const double b00 = a00 - q, b11 = a11 - q, b22 = a22 - q;
        const double p = sqrt((b00 * b00 + b11 * b11 + b22 * b22 + 2.0 * off2) / 6.0);
        const double ip = 1.0 / p;
        const double e00 = b00 * ip, e11 = b11 * ip, e22 = b22 * ip, e01 = a01 * ip, e02 = a02 * ip, e12 = a12 * ip;
        half_det = 0.5 * (e00 * (e11 * e22 - e12 * e12) - e01 * (e01 * e22 - e12 * e02) + e02 * (e01 * e12 - e11 * e02));
        half_det = half_det < -1.0 ? -1.0 : (half_det > 1.0 ? 1.0 : half_det);
        const double phi = acos(half_det) / 3.0;
        const double two_thirds_pi = 2.09439510239319549231;
        const double g2 = 2.0 * cos(phi), g0 = 2.0 * cos(phi + two_thirds_pi), g1 = -(g0 + g2);
        l0 = q + p * g0; l1 = q + p * g1; l2 = q + p * g2;
    } else {                                                    // diagonal: the entries, sorted
        l0 = a00; l1 = a11; l2 = a22;
        double t;
        if (l0 > l1) { t = l0; l0 = l1; l1 = t; }
        if (l1 > l2) { t = l1; l1 = l2; l2 = t; }
        if (l0 > l1) { t = l0; l0 = l1; l1 = t; }
        half_det = (l2 - l1) >= (l1 - l0) ? 1.0 : -1.0;
    }
    if (lam) { lam[0] = l0 * mx; lam[1] = l1 * mx; lam[2] = l2 * mx; }
    double v0[3] = {0.0, 0.0, 1.0}, v2[3];
    if (half_det >= 0.0) {                                      // the largest eigenvalue is the separated one (and the accurate one: d cos / d phi = 0 at phi = 0)
        if (!(in_null_vector(a00, a01, a02, a11, a12, a22, l2, v2) > 0.0)) return 0;
        in_smallest_in_complement(a00, a01, a02, a11, a12, a22, v2, v0);
    } else {                                                    // the smallest is (accurate likewise at phi = pi / 3)
        if (!(in_null_vector(a00, a01, a02, a11, a12, a22, l0, v0) > 0.0)) return 0;
    }
    const double s = 1.0 / sqrt(in_dot(v0, v0));
    n[0] = v0[0] * s; n[1] = v0[1] * s; n[2] = v0[2] * s;
    return 1;
}

// Mean and covariance (divided by n) of the first n <= IN_KMAX of IN_KMAX points given as float32 triples, float64, in list order.
// c = (xx, xy, xz, yy, yz, zz).  The loops run over all IN_KMAX slots under a predicate: constant indices, so the points stay in registers.
IN_HD void in_covariance(const float* p, int n, double* c)
{
    double m[3] = {0.0, 0.0, 0.0};
    IN_UNROLL
    for (int i = 0; i < IN_KMAX; i++) if (i < n) { m[0] += (double)p[3 * i]; m[1] += (double)p[3 * i + 1]; m[2] += (double)p[3 * i + 2]; }
    const double in = 1.0 / (double)n;
    m[0] *= in; m[1] *= in; m[2] *= in;
    IN_UNROLL
    for (int k = 0; k < 6; k++) c[k] = 0.0;
    IN_UNROLL
    for (int i = 0; i < IN_KMAX; i++) if (i < n) {
        const double x = (double)p[3 * i] - m[0], y = (double)p[3 * i + 1] - m[1], z = (double)p[3 * i + 2] - m[2];
        c[0] += x * x; c[1] += x * y; c[2] += x * z; c[3] += y * y; c[4] += y * z; c[5] += z * z;
    }
    IN_UNROLL
    for (int k = 0; k < 6; k++) c[k] *= in;
}

// The float32 normal n of the point p seen from o, turned to face the sensor.
IN_HD void in_face_sensor(float* n, const float* o, const float* p)
{
    const double s = (double)n[0] * ((double)o[0] - (double)p[0]) + (double)n[1] * ((double)o[1] - (double)p[1]) + (double)n[2] * ((double)o[2] - (double)p[2]);
    bool flip = s < 0.0;
    if (s == 0.0) { const float f = n[0] != 0.f ? n[0] : (n[1] != 0.f ? n[1] : n[2]); flip = f < 0.f; }
    if (flip) { n[0] = -n[0]; n[1] = -n[1]; n[2] = -n[2]; }
}

#endif /* LRT_INIT_MATH_H_INCLUDED */
