// lrt_segment_math.h -- the rules of the range-image segmentation (include/lrt_segment.h): the one text for the device (lrt_segment.hip) and the
// host (tests/host_check/segment_check.cpp, g++ -ffp-contract=off).  The pixel rule is lrt_project_math.h's, unchanged; lrt_sweep_math.h is read
// as it is for the pose conventions it states.
//
//   sg_r2, sg_d2    float32: fma(z, z, fma(y, y, x * x)) of a point, of the difference of two (the expression of lrt_gridcd_math.h)
//   sg_join         two kept 4-neighbours are one surface: d2 <= max(dabs2, cdir2 * min(r2_a, r2_b)), float32, false for a NaN
//   sg_ground_step  one pixel of the column scan: h = up . p, g = p - h up, the band test without and the slope test with a ground pixel below
//   sg_freespace    has the target frame seen through the place of X p: -1 unknown, 1 free, 0 occupied
//   sg_quant        llrint(v * 1024) of a float32 coordinate (exact product); sg_quant64 the same of a float64 value
//   sg_actor_point  a = R^T (p - t) for a (3, 4) row-major pose
//
// Float64 with every operation rounded on its own unless float32 is named.
#ifndef LRT_SEGMENT_MATH_H_INCLUDED
#define LRT_SEGMENT_MATH_H_INCLUDED

#include <math.h>
#include "lrt_project_math.h"
#include "lrt_sweep_math.h"

#define SG_HD PJ_HD

#define SG_NCOL 16          /* int64 entries per table row */
#define SG_ROOT 0
#define SG_COUNT 1
#define SG_EV 2             /* free and known of evidence image 0, then of image 1 */
#define SG_SUM 6
#define SG_MIN 9
#define SG_MAX 12
#define SG_QUANT 1024.0
#define SG_QUANT_LIMIT 9.0e15          /* |v * 1024| at or above it (or not a number) quantises to 0: far outside any max_depth */

#if defined(__HIP_DEVICE_COMPILE__)
SG_HD float sg_fmaf(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
SG_HD float sg_fmaf(float a, float b, float c) { return fmaf(a, b, c); }
#endif

SG_HD float sg_r2(const float* p)
{
#pragma clang fp contract(off)
    const float xx = p[0] * p[0];
    return sg_fmaf(p[2], p[2], sg_fmaf(p[1], p[1], xx));
}

SG_HD float sg_d2(const float* a, const float* b)
{
#pragma clang fp contract(off)
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    const float xx = dx * dx;
    return sg_fmaf(dz, dz, sg_fmaf(dy, dy, xx));
}

// dabs2 = d_abs * d_abs and cdir2 = c_dir * c_dir, each one float32 product of the float32 parameter.
SG_HD bool sg_join(const float* a, const float* b, float dabs2, float cdir2)
{
#pragma clang fp contract(off)
    const float d2 = sg_d2(a, b);
    const float ra = sg_r2(a), rb = sg_r2(b);
    const float m = ra < rb ? ra : rb;
    const float rel = cdir2 * m;
    const float bound = dabs2 > rel ? dabs2 : rel;
    return d2 <= bound;                                              // a NaN coordinate on either side makes d2 a NaN: not joined
}

struct SgGround {
    int have;                                                        // the column has a ground pixel
    double h, g[3];                                                  // the last one's height and horizontal part
};

// One valid pixel, visited in the order of ascending inclination.  Returns 1 for ground and moves the state to it.
SG_HD int sg_ground_step(const float* p, const double* up, double z_lo, double z_hi, double slope, SgGround* s)
{
#pragma clang fp contract(off)
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double h = up[0] * x + up[1] * y + up[2] * z;
    const double g[3] = {x - h * up[0], y - h * up[1], z - h * up[2]};
    bool ground;
    if (!s->have) {
        ground = h >= z_lo && h <= z_hi;
    } else {
        const double dx = g[0] - s->g[0], dy = g[1] - s->g[1], dz = g[2] - s->g[2];
        ground = fabs(h - s->h) <= slope * sqrt(dx * dx + dy * dy + dz * dz);
    }
    if (ground) { s->have = 1; s->h = h; s->g[0] = g[0]; s->g[1] = g[1]; s->g[2] = g[2]; }
    return ground ? 1 : 0;
}

// Rows in the order of ascending inclination: row h carries inc0 + (H - h - off) / H (inc1 - inc0), or the table's entry H - 1 - h.
SG_HD int sg_row_at(int k, int H, const double* inc, int n_inc) { return inc[n_inc - 1] > inc[0] ? H - 1 - k : k; }

// p: a valid source point; tr, tm: the target's ranges and mask (H W pixels).
SG_HD int sg_freespace(const double* X, const float* p, const PjRule& R, const double* inc, const float* tr, const unsigned char* tm, int rh, int rw,
                       double m_abs, double m_rel)
{
#pragma clang fp contract(off)
    double q[3];
    pj_transform(X, p[0], p[1], p[2], q);
    int w0, h0;
    float r32;
    if (pj_classify(q, R, inc, &w0, &h0, &r32) != PJ_KEEP) return -1;
    const double rq = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2]);
    const double thr = rq + m_abs + m_rel * rq;
    int n = 0, through = 1;
    for (int dh = -rh; dh <= rh; dh++) {
        const int h = h0 + dh;
        if (h < 0 || h >= R.H) continue;
        for (int dw = -rw; dw <= rw; dw++) {
            int w = (w0 + dw) % R.W;
            if (w < 0) w += R.W;
            const int j = h * R.W + w;
            if (!tm[j]) continue;
            n++;
            if (!((double)tr[j] > thr)) through = 0;
        }
    }
    return n == 0 ? -1 : through;
}

SG_HD long long sg_quant64(double a)
{
#pragma clang fp contract(off)
    const double v = a * SG_QUANT;
    if (!(fabs(v) < SG_QUANT_LIMIT)) return 0;
    return llrint(v);
}

SG_HD long long sg_quant(float p) { return sg_quant64((double)p); }

// T (3, 4) row-major: the actor in the sensor frame.
SG_HD void sg_actor_point(const double* T, const float* p, double* a)
{
#pragma clang fp contract(off)
    const double d[3] = {(double)p[0] - T[3], (double)p[1] - T[7], (double)p[2] - T[11]};
    a[0] = T[0] * d[0] + T[4] * d[1] + T[8] * d[2];
    a[1] = T[1] * d[0] + T[5] * d[1] + T[9] * d[2];
    a[2] = T[2] * d[0] + T[6] * d[1] + T[10] * d[2];
}

#endif /* LRT_SEGMENT_MATH_H_INCLUDED */
