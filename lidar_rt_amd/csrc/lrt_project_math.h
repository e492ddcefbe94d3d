// lrt_project_math.h -- the rule of the range-image projection (include/lrt_project.h), inline for host and device so that
// tests/host_check/project_check.cpp can compile it with g++ (-ffp-contract=off) and compare it with numpy.  Everything is float64; the
// one float32 value is the range r32 = (float) r that orders the returns of a pixel and becomes the depth.
//
//   pj_transform   q = T (x, y, z, 1) for a 3 x 4 row-major T, each row summed left to right; T == null: q = (x, y, z)
//   pj_column      u = (pi - (az + yaw)) W / 2 pi - off, w = rint(u); wrapped into [0, W) or refused outside it
//   pj_row_bounds  v = H - off - (el - inc0) / (inc1 - inc0) H, h = rint(v); refused outside [0, H)
//   pj_row_table   the beam of the nearest inclination of a strictly monotonic table (row h <-> inc[H - 1 - h]); ties to the lower row;
//                  further from an outermost beam than half the gap to its one neighbour is refused.  A table that is not monotonic
//                  gives some row of [0, H) or a refusal: never an index outside the table
//   pj_classify    the drop class of a point and, for a kept one, its pixel and r32
//
// It is the inverse of RangeFrames.range_rays (lidar_rt_amd/training.py): column w has azimuth (W - w - off) / W 2 pi - pi - yaw, row h the
// inclination inc0 + (H - h - off) / H (inc1 - inc0) or the table's entry H - 1 - h.
#ifndef LRT_PROJECT_MATH_H_INCLUDED
#define LRT_PROJECT_MATH_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PJ_HD __host__ __device__ inline
#else
#define PJ_HD inline
#endif

#define PJ_KEEP 0
#define PJ_INVALID 1
#define PJ_OUT_OF_RANGE 2
#define PJ_OUT_OF_VIEW 3

#define PJ_PI 3.14159265358979323846
#define PJ_TWO_PI 6.28318530717958647692

struct PjRule {
    int H, W, n_inc, wrap;
    double off, yaw, min_depth, max_depth;
};

PJ_HD bool pj_finite(double x) { return x - x == 0.0; }

PJ_HD void pj_transform(const double* T, float x, float y, float z, double* q)
{
#pragma clang fp contract(off)                                   // every operation rounds on its own, on the device as on the host
    const double p[3] = {(double)x, (double)y, (double)z};
    if (!T) { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; return; }
    q[0] = T[0] * p[0] + T[1] * p[1] + T[2] * p[2] + T[3];
    q[1] = T[4] * p[0] + T[5] * p[1] + T[6] * p[2] + T[7];
    q[2] = T[8] * p[0] + T[9] * p[1] + T[10] * p[2] + T[11];
}

// The column of azimuth az, or -1.
PJ_HD int pj_column(double az, const PjRule& R)
{
#pragma clang fp contract(off)
    const double W = (double)R.W;
    const double u = (PJ_PI - (az + R.yaw)) * W / PJ_TWO_PI - R.off;
    double w = rint(u);
    if (R.wrap) {
        const double k = floor(w / W);
        w = w - k * W;
    }
    if (!(w >= 0.0 && w < W)) return -1;
    return (int)w;
}

// The row of elevation el between the bounds inc[0], inc[1], or -1.
PJ_HD int pj_row_bounds(double el, const double* inc, const PjRule& R)
{
#pragma clang fp contract(off)
    const double H = (double)R.H;
    const double t = (el - inc[0]) / (inc[1] - inc[0]) * H;
    const double v = H - R.off - t;
    const double h = rint(v);
    if (!(h >= 0.0 && h < H)) return -1;
    return (int)h;
}

// The row of elevation el in a table of H >= 3 beams, or -1.  s(k) is the table in ascending order.
PJ_HD int pj_row_table(double el, const double* inc, int H)
{
#pragma clang fp contract(off)
    const bool asc = inc[H - 1] > inc[0];
#define PJ_S(k) (asc ? inc[(k)] : inc[H - 1 - (k)])
    int lo = 0, hi = H;                                          // the number of beams with s(k) <= el
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (PJ_S(mid) <= el) lo = mid + 1; else hi = mid;
    }
    int k;
    if (lo == 0) {
        const double d = PJ_S(0) - el, half = 0.5 * (PJ_S(1) - PJ_S(0));
        if (!(d <= half)) return -1;
        k = 0;
    } else if (lo == H) {
        const double d = el - PJ_S(H - 1), half = 0.5 * (PJ_S(H - 1) - PJ_S(H - 2));
        if (!(d <= half)) return -1;
        k = H - 1;
    } else {
        const double dl = el - PJ_S(lo - 1), dh = PJ_S(lo) - el;
        // table entry t = asc ? k : H - 1 - k, row = H - 1 - t: ascending tables put the higher beam on the lower row
        if (dl < dh) k = lo - 1;
        else if (dh < dl) k = lo;
        else k = asc ? lo : lo - 1;
    }
#undef PJ_S
    const int t = asc ? k : H - 1 - k;
    return H - 1 - t;
}

// q: the point in the sensor frame.  Returns the drop class; for PJ_KEEP, *w, *h and *r32 are the pixel and the range.  *r32 is set for every
// class but PJ_INVALID.
PJ_HD int pj_classify(const double* q, const PjRule& R, const double* inc, int* w, int* h, float* r32)
{
#pragma clang fp contract(off)
    *w = -1; *h = -1; *r32 = 0.f;
    const double x = q[0], y = q[1], z = q[2];
    if (!(pj_finite(x) && pj_finite(y) && pj_finite(z))) return PJ_INVALID;
    const double r = sqrt(x * x + y * y + z * z);
    if (r == 0.0) return PJ_INVALID;
    const float rf = (float)r;
    *r32 = rf;
    if (!((double)rf > R.min_depth && (double)rf <= R.max_depth)) return PJ_OUT_OF_RANGE;
    const double az = atan2(y, x);
    const double el = atan2(z, hypot(x, y));
    const int c = pj_column(az, R);
    if (c < 0) return PJ_OUT_OF_VIEW;
    const int row = R.n_inc == 2 ? pj_row_bounds(el, inc, R) : pj_row_table(el, inc, R.H);
    if (row < 0) return PJ_OUT_OF_VIEW;
    *w = c; *h = row;
    return PJ_KEEP;
}

#endif /* LRT_PROJECT_MATH_H_INCLUDED */
