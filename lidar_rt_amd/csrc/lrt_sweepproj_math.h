// lrt_sweepproj_math.h -- the rule of the range-image projection under the sweep model (include/lrt_sweepproj.h), inline for host and device so
// that tests/host_check/sweepproj_check.cpp can compile it with g++ (-ffp-contract=off) and compare it with numpy.  It adds to
// lrt_project_math.h (the static rule: pj_transform, the column and row arithmetic) and lrt_sweep_math.h (sw_exp) only what is new.
// Everything is float64; the one float32 value is the range r32 = (float) r that orders the returns of a pixel and becomes the depth.
//
//   sp_column_entry  the table entry of a column: the inverse of E = Exp(s xi) = [Re | te] as a row-major 3 x 4, [Re^T | -(Re^T te)]
//   sp_to_column     q = E^-1 (p, 1), each row summed left to right as pj_transform does; an entry that is EXACTLY the identity (no twist, a
//                    zero twist, s == 0) gives q = p with the sign of every zero kept -- what makes zero motion the static rule bit for bit
//   sp_u             pj_column's continuous column u = (pi - (az + yaw)) W / 2 pi - off of a point
//   sp_column_of     a rounded u as a column of [0, W) WHATEVER it holds (a NaN included): taken mod W with the wrap, clamped without
//   sp_search        the fixed-point search from the static column: at most SP_MAX_EVAL evaluations, the column and q of the LAST evaluation
//   sp_classify      the drop class of q in pj_classify's order, with the search's end between the range and the row
//   sp_point         all of it for one point
//
// sw_exp has no contraction pragma of its own: the device may fuse its multiply-adds, so a table entry can differ from the host's in its last
// bits, and with it q, u and r.  The comparisons therefore rest on two margins of the inputs (lidar_rt_amd/sweep_project.py): every evaluated
// u and the row coordinate stay away from their rounding boundaries, every kept r from a float32 rounding boundary.
#ifndef LRT_SWEEPPROJ_MATH_H_INCLUDED
#define LRT_SWEEPPROJ_MATH_H_INCLUDED

#include "lrt_project_math.h"
#include "lrt_sweep_math.h"

#define SP_UNSEEN 4             /* the drop class after PJ_KEEP .. PJ_OUT_OF_VIEW */
#define SP_MAX_EVAL 8           /* LRT_SWEEPPROJ_MAX_EVAL */
#define SP_TABLE 12             /* LRT_SWEEPPROJ_TABLE */

#define SP_CONVERGED 0          /* how a search ended */
#define SP_EDGE 1
#define SP_CYCLE 2

// E (12): the inverse of Exp(s xi), xi = (rho, phi) float64.
PJ_HD void sp_column_entry(const double* xi, double s, double* E)
{
#pragma clang fp contract(off)
    double x[6], Re[9], te[3];
    for (int k = 0; k < 6; k++) x[k] = s * xi[k];
    sw_exp(x, Re, te);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) E[4 * i + j] = Re[3 * j + i];
        E[4 * i + 3] = -(Re[i] * te[0] + Re[3 + i] * te[1] + Re[6 + i] * te[2]);
    }
}

PJ_HD bool sp_is_identity(const double* E)
{
    return E[0] == 1.0 && E[1] == 0.0 && E[2] == 0.0 && E[3] == 0.0 && E[4] == 0.0 && E[5] == 1.0 && E[6] == 0.0 && E[7] == 0.0
        && E[8] == 0.0 && E[9] == 0.0 && E[10] == 1.0 && E[11] == 0.0;
}

// q: the point p of the reference frame as the column of entry E sees it.  E == null: a static sensor.
PJ_HD void sp_to_column(const double* E, const double* p, double* q)
{
#pragma clang fp contract(off)
    if (!E || sp_is_identity(E)) { q[0] = p[0]; q[1] = p[1]; q[2] = p[2]; return; }
    q[0] = E[0] * p[0] + E[1] * p[1] + E[2] * p[2] + E[3];
    q[1] = E[4] * p[0] + E[5] * p[1] + E[6] * p[2] + E[7];
    q[2] = E[8] * p[0] + E[9] * p[1] + E[10] * p[2] + E[11];
}

PJ_HD double sp_u(const double* q, const PjRule& R)
{
#pragma clang fp contract(off)
    const double az = atan2(q[1], q[0]);
    return (PJ_PI - (az + R.yaw)) * (double)R.W / PJ_TWO_PI - R.off;
}

// c = rint(u) as a column: always within [0, W).
PJ_HD int sp_column_of(double c, const PjRule& R)
{
#pragma clang fp contract(off)
    const double W = (double)R.W;
    if (R.wrap) {
        const double k = floor(c / W);
        c = c - k * W;
        return (c >= 0.0 && c < W) ? (int)c : 0;
    }
    return c < W ? (c >= 0.0 ? (int)c : 0) : R.W - 1;              // a NaN fails the first test
}

// p: the point in the frame of the reference instant, finite.  table: W entries of SP_TABLE doubles, or null.  Returns how the search ended;
// *w is the last evaluated column, q the point as that column sees it, *evals the evaluations used (1 .. SP_MAX_EVAL).
PJ_HD int sp_search(const double* p, const double* table, const PjRule& R, double* q, int* w, int* evals)
{
#pragma clang fp contract(off)
    const double W = (double)R.W;
    int col = sp_column_of(rint(sp_u(p, R)), R);
    int n = 0, state = SP_CYCLE;
    for (;;) {
        sp_to_column(table ? table + SP_TABLE * (long long)col : nullptr, p, q);
        n++;
        const double c = rint(sp_u(q, R));
        const int next = sp_column_of(c, R);
        if (next == col) {
            state = (R.wrap || (c >= 0.0 && c < W)) ? SP_CONVERGED : SP_EDGE;
            break;
        }
        if (n == SP_MAX_EVAL) break;
        col = next;
    }
    *w = col; *evals = n;
    return state;
}

// q, state: what sp_search left.  Returns the drop class; for PJ_KEEP *h is the row.  *r32 is set for every class but PJ_INVALID.
PJ_HD int sp_classify(const double* q, int state, const PjRule& R, const double* inc, int* h, float* r32)
{
#pragma clang fp contract(off)
    *h = -1; *r32 = 0.f;
    const double x = q[0], y = q[1], z = q[2];
    if (!(pj_finite(x) && pj_finite(y) && pj_finite(z))) return PJ_INVALID;
    const double r = sqrt(x * x + y * y + z * z);
    if (r == 0.0) return PJ_INVALID;
    const float rf = (float)r;
    *r32 = rf;
    if (!((double)rf > R.min_depth && (double)rf <= R.max_depth)) return PJ_OUT_OF_RANGE;
    if (state == SP_EDGE) return PJ_OUT_OF_VIEW;
    if (state != SP_CONVERGED) return SP_UNSEEN;
    const double el = atan2(z, hypot(x, y));
    const int row = R.n_inc == 2 ? pj_row_bounds(el, inc, R) : pj_row_table(el, inc, R.H);
    if (row < 0) return PJ_OUT_OF_VIEW;
    *h = row;
    return PJ_KEEP;
}

// One point: T its frame's points2sensor or null, table its frame's column table or null.  *w, *h: the pixel of a kept point, -1 otherwise;
// *evals: 0 for a point that is not finite in the reference frame.
PJ_HD int sp_point(const double* T, float x, float y, float z, const double* table, const PjRule& R, const double* inc, int* w, int* h, float* r32, int* evals)
{
    double p[3], q[3];
    *w = -1; *h = -1; *r32 = 0.f; *evals = 0;
    pj_transform(T, x, y, z, p);
    if (!(pj_finite(p[0]) && pj_finite(p[1]) && pj_finite(p[2]))) return PJ_INVALID;
    int col;
    const int state = sp_search(p, table, R, q, &col, evals);
    const int cls = sp_classify(q, state, R, inc, h, r32);
    if (cls == PJ_KEEP) *w = col;
    return cls;
}

#endif /* LRT_SWEEPPROJ_MATH_H_INCLUDED */
