// lrt_raycast_math.h -- the rule of the ray casting of a TSDF grid (include/lrt_raycast.h), inline for host and device so that
// tests/host_check/raycast_check.cpp can compile it with g++ (-ffp-contract=off) and compare it with numpy.  Everything is float64 with
// contraction off, from + - * /, sqrt, floor and the min / max below; the twin is lidar_rt_amd.raycast.raycast_reference.
//
//   rc_centre   c = (float) (voxel (i + 0.5)): mh_centre of lrt_mesh_math.h, the same expression
//   rc_cell     i = clamp(floor(p / voxel - 0.5), 0, n - 2), clamped in float64 before the conversion
//   rc_tri      the trilinear value of a cell's eight corners: four lerps along x, two along y, one along z; lerp(a, b, f) = a + f (b - a)
//   rc_ray      one ray: its domain, its samples, its step sequence and its crossing
//
// A sample that stays in the previous sample's cell reuses that cell's corners (tsdf, known, all-ones) from registers: the same values, so no bit
// changes, and about half the gathers at the default step.
#ifndef LRT_RAYCAST_MATH_H_INCLUDED
#define LRT_RAYCAST_MATH_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RC_HD __host__ __device__ inline
#else
#define RC_HD inline
#endif

struct RcGrid {
    int X, Y, Z, min_weight;
    double voxel, ox, oy, oz;                                       // origin: the grid frame's place in the world
    const float* tsdf;
    const int* weight;
    const float* intensity;                                         // null: none
};

struct RcParams {
    double step, far_step, min_depth, max_depth;
};

struct RcOut {
    float depth, intensity;
    int samples;
    unsigned char hit;
};

RC_HD double rc_min(double a, double b) { return a < b ? a : b; }
RC_HD double rc_max(double a, double b) { return a > b ? a : b; }
RC_HD double rc_clamp01(double f) { return f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f); }
RC_HD bool rc_finite(float x) { return x - x == 0.f; }

RC_HD float rc_centre(double voxel, int i)
{
#pragma clang fp contract(off)
    return (float)(voxel * ((double)i + 0.5));
}

RC_HD int rc_cell(double p, double voxel, int n)
{
#pragma clang fp contract(off)
    const double fi = floor(p / voxel - 0.5);
    if (!(fi > 0.0)) return 0;
    if (fi > (double)(n - 2)) return n - 2;
    return (int)fi;
}

RC_HD double rc_lerp(double a, double b, double f)
{
#pragma clang fp contract(off)
    return a + f * (b - a);
}

// v[n]: corner n = (n & 1, n >> 1 & 1, n >> 2 & 1) along (x, y, z)
RC_HD double rc_tri(const float* v, const double* f)
{
#pragma clang fp contract(off)
    const double c00 = rc_lerp((double)v[0], (double)v[1], f[0]), c10 = rc_lerp((double)v[2], (double)v[3], f[0]);
    const double c01 = rc_lerp((double)v[4], (double)v[5], f[0]), c11 = rc_lerp((double)v[6], (double)v[7], f[0]);
    const double c0 = rc_lerp(c00, c10, f[1]), c1 = rc_lerp(c01, c11, f[1]);
    return rc_lerp(c0, c1, f[2]);
}

RC_HD long long rc_index(const RcGrid& g, int i, int j, int k) { return ((long long)i * g.Y + j) * g.Z + k; }

RC_HD void rc_corners(const float* a, const RcGrid& g, const int* c, float* v)
{
    const long long b = rc_index(g, c[0], c[1], c[2]), YZ = (long long)g.Y * g.Z, Z = g.Z;
    for (int n = 0; n < 8; n++) v[n] = a[b + (n & 1) * YZ + (n >> 1 & 1) * Z + (n >> 2 & 1)];
}

RC_HD RcOut rc_ray(const RcGrid& g, const RcParams& P, const float* ro, const float* rd)
{
#pragma clang fp contract(off)
    RcOut r;
    r.depth = 0.f; r.intensity = 0.f; r.samples = 0; r.hit = 0;
    if (g.X < 2 || g.Y < 2 || g.Z < 2) return r;
    if (!(rc_finite(ro[0]) && rc_finite(ro[1]) && rc_finite(ro[2]) && rc_finite(rd[0]) && rc_finite(rd[1]) && rc_finite(rd[2]))) return r;
    const double org[3] = {g.ox, g.oy, g.oz};
    double o[3], d[3], u[3];
    for (int a = 0; a < 3; a++) { o[a] = (double)ro[a] - org[a]; d[a] = (double)rd[a]; }
    const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(nrm > 0.0)) return r;
    for (int a = 0; a < 3; a++) u[a] = d[a] / nrm;
    const int n[3] = {g.X, g.Y, g.Z};
    double tin = P.min_depth, tout = P.max_depth;
    for (int a = 0; a < 3; a++) {
        const double c0 = (double)rc_centre(g.voxel, 0), c1 = (double)rc_centre(g.voxel, n[a] - 1);
        if (u[a] == 0.0) {
            if (!(c0 <= o[a] && o[a] <= c1)) return r;
            continue;
        }
        const double t1 = (c0 - o[a]) / u[a], t2 = (c1 - o[a]) / u[a];
        tin = rc_max(tin, rc_min(t1, t2));
        tout = rc_min(tout, rc_max(t1, t2));
    }
    int cell[3] = {-1, -1, -1}, prev[3] = {0, 0, 0};
    float v[8];
    bool known = false, ones = false, kp = false;
    double tp = 0.0, Dp = 0.0, fp[3] = {0.0, 0.0, 0.0};
    int ns = 0;
    for (double t = tin; t <= tout;) {
        int idx[3];
        double f[3];
        for (int a = 0; a < 3; a++) {
            const double p = o[a] + t * u[a];
            idx[a] = rc_cell(p, g.voxel, n[a]);
            const double ca = (double)rc_centre(g.voxel, idx[a]), cb = (double)rc_centre(g.voxel, idx[a] + 1);
            f[a] = rc_clamp01((p - ca) / (cb - ca));
        }
        ns++;
        if (idx[0] != cell[0] || idx[1] != cell[1] || idx[2] != cell[2]) {      // a new cell: gather its corners
            int w[8];
            rc_corners(g.tsdf, g, idx, v);
            const long long b = rc_index(g, idx[0], idx[1], idx[2]), YZ = (long long)g.Y * g.Z, Z = g.Z;
            for (int c = 0; c < 8; c++) w[c] = g.weight[b + (c & 1) * YZ + (c >> 1 & 1) * Z + (c >> 2 & 1)];
            known = true; ones = true;
            for (int c = 0; c < 8; c++) { known = known && w[c] >= g.min_weight; ones = ones && v[c] == 1.0f; }
            cell[0] = idx[0]; cell[1] = idx[1]; cell[2] = idx[2];
        }
        double s = P.step;
        if (known) {
            const double D = rc_tri(v, f);
            if (kp && Dp > 0.0 && D <= 0.0) {
                const double w = Dp / (Dp - D);
                r.depth = (float)(tp + (t - tp) * w);
                r.hit = 1;
                if (g.intensity) {
                    float ia[8], ib[8];
                    rc_corners(g.intensity, g, prev, ia);
                    rc_corners(g.intensity, g, idx, ib);
                    const double Ip = rc_tri(ia, fp), Ik = rc_tri(ib, f);
                    r.intensity = (float)(Ip + (Ik - Ip) * w);
                }
                r.samples = ns;
                return r;
            }
            if (ones) s = P.far_step;
            kp = true; tp = t; Dp = D;
            for (int a = 0; a < 3; a++) { prev[a] = idx[a]; fp[a] = f[a]; }
        } else {
            kp = false;
        }
        t = t + s;
    }
    r.samples = ns;
    return r;
}

#endif /* LRT_RAYCAST_MATH_H_INCLUDED */
