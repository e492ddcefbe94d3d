// lrt_mapreg_math.h -- the rule of the scan-to-map registration (include/lrt_mapreg.h): the one text for the device (lrt_mapreg.hip) and the host
// (tests/host_check/mapreg_check.cpp, g++ -ffp-contract=off).  It owns as little arithmetic as it can: the grid's cells, centres, fractions and
// lerps are lrt_raycast_math.h's, the transform is lrt_project_math.h's, the solve, the 30-sum layout and the status codes are lrt_reg_math.h's,
// all three included as they are.
//
//   mr_sample    one point of the grid frame: its cell, the trilinear value D of the cell's eight corners (the lerp order of rc_tri) and the
//                gradient g of that trilinear function; -1 outside the domain, in a cell with an unobserved corner, in free space (all eight
//                corners exactly 1.0f) and where g is exactly (0, 0, 0)
//   mr_pixel     one source pixel: q = X p, the sample, e = trunc D, n = trunc g, the Huber weight, the Jacobian and the pixel's 30 terms.
//                Returns the linear voxel index of the cell's base corner or -1 (the terms are left as they are then: the caller zeroes them)
//   mr_inverse   G = X^-1 of a rigid X (3, 4): R^T and -(R^T t), rows summed left to right
//
// Float64 with every operation rounded on its own; only + - * / and floor, so the device and the host give the same bits.
#ifndef LRT_MAPREG_MATH_H_INCLUDED
#define LRT_MAPREG_MATH_H_INCLUDED

#include <math.h>
#include "lrt_raycast_math.h"
#include "lrt_reg_math.h"
#include "lrt_project_math.h"

#define MR_HD RG_HD

// g: the grid (its origin and intensity are not read: q is in the GRID frame).  q: the point.  cell: the base corner (i, j, k).  D, grad: out.
MR_HD long long mr_sample(const RcGrid& g, const double* q, int* cell, double* D, double* grad)
{
#pragma clang fp contract(off)
    if (g.X < 2 || g.Y < 2 || g.Z < 2) return -1;                       // no domain
    const int n[3] = {g.X, g.Y, g.Z};
    double f[3], h[3];
    RG_UNROLL
    for (int a = 0; a < 3; a++) {
        if (!(q[a] - q[a] == 0.0)) return -1;                           // not finite
        const double c0 = (double)rc_centre(g.voxel, 0), c1 = (double)rc_centre(g.voxel, n[a] - 1);
        if (!(c0 <= q[a] && q[a] <= c1)) return -1;
        cell[a] = rc_cell(q[a], g.voxel, n[a]);
        const double ca = (double)rc_centre(g.voxel, cell[a]), cb = (double)rc_centre(g.voxel, cell[a] + 1);
        h[a] = cb - ca;
        f[a] = rc_clamp01((q[a] - ca) / h[a]);
    }
    float v[8];
    rc_corners(g.tsdf, g, cell, v);
    const long long b = rc_index(g, cell[0], cell[1], cell[2]), YZ = (long long)g.Y * g.Z, Z = g.Z;
    bool known = true, ones = true;
    RG_UNROLL
    for (int c = 0; c < 8; c++) {
        known = known && g.weight[b + (c & 1) * YZ + (c >> 1 & 1) * Z + (c >> 2 & 1)] >= g.min_weight;
        ones = ones && v[c] == 1.0f;
    }
    if (!known || ones) return -1;
    double d[8];
    RG_UNROLL
    for (int c = 0; c < 8; c++) d[c] = (double)v[c];
    const double c00 = rc_lerp(d[0], d[1], f[0]), c10 = rc_lerp(d[2], d[3], f[0]);
    const double c01 = rc_lerp(d[4], d[5], f[0]), c11 = rc_lerp(d[6], d[7], f[0]);
    const double c0 = rc_lerp(c00, c10, f[1]), c1 = rc_lerp(c01, c11, f[1]);
    *D = rc_lerp(c0, c1, f[2]);
    grad[0] = rc_lerp(rc_lerp(d[1] - d[0], d[3] - d[2], f[1]), rc_lerp(d[5] - d[4], d[7] - d[6], f[1]), f[2]) / h[0];
    grad[1] = rc_lerp(c10 - c00, c11 - c01, f[2]) / h[1];
    grad[2] = (c1 - c0) / h[2];
    if (grad[0] == 0.0 && grad[1] == 0.0 && grad[2] == 0.0) return -1;
    return b;
}

// X (3, 4) row-major: the source frame's pose in the grid frame; p: the source point.  t: RG_NSUM terms, written only when there is a term.
// en: null, or e and n (4 numbers) of a pixel that has a term.
MR_HD long long mr_pixel(const RcGrid& g, double trunc, const double* X, const float* p, double huber, double* t, double* en)
{
#pragma clang fp contract(off)
    double q[3], D, gr[3];
    int cell[3];
    pj_transform(X, p[0], p[1], p[2], q);
    const long long b = mr_sample(g, q, cell, &D, gr);
    if (b < 0) return -1;
    const double e = trunc * D;
    const double n[3] = {trunc * gr[0], trunc * gr[1], trunc * gr[2]};
    if (en) { en[0] = e; en[1] = n[0]; en[2] = n[1]; en[3] = n[2]; }
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
    return b;
}

MR_HD void mr_inverse(const double* X, double* G)
{
#pragma clang fp contract(off)
    RG_UNROLL
    for (int i = 0; i < 3; i++) {
        RG_UNROLL
        for (int j = 0; j < 3; j++) G[4 * i + j] = X[4 * j + i];
        G[4 * i + 3] = -(X[i] * X[3] + X[4 + i] * X[7] + X[8 + i] * X[11]);
    }
}

#endif /* LRT_MAPREG_MATH_H_INCLUDED */
