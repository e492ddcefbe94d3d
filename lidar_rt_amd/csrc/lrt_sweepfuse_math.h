// lrt_sweepfuse_math.h -- the rule of the TSDF fusion under the sweep model (include/lrt_sweepfuse.h), inline for host and device so that
// tests/host_check/sweepfuse_check.cpp can compile it with g++ (-ffp-contract=off) and compare it with numpy.  Everything is float64 with
// contraction off.  It owns no arithmetic: the centre, the frame's images and the update are lrt_mesh_math.h's (mh_centre, MhFrame, mh_fuse's
// operations in mh_fuse's order), the column search and the drop class are lrt_sweepproj_math.h's (sp_search, sp_classify), both as they are.
//
//   sf_identity   the table entry of a column of a static sensor: what sp_column_entry gives for a zero twist, exactly
//   sf_fuse       one frame's update of one voxel: the centre into the frame of the reference instant, the search for the column that sees
//                 it, the drop class and the row, the pixel, then sdf = depth - r32 with r32 measured from THAT column's origin
//
// As in lrt_sweepproj_math.h a table entry may differ between the device and the host in its last bits (sw_exp has no contraction pragma), so
// the comparisons rest on the two margins of the inputs that project_points_sweep_reference returns.
#ifndef LRT_SWEEPFUSE_MATH_H_INCLUDED
#define LRT_SWEEPFUSE_MATH_H_INCLUDED

#include "lrt_mesh_math.h"
#include "lrt_sweepproj_math.h"

PJ_HD void sf_identity(double* E)
{
    for (int k = 0; k < SP_TABLE; k++) E[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
}

// One frame's update of a voxel centred at (cx, cy, cz) in the grid frame.  T: the frame's (3, 4) grid-to-sensor transform (to the sensor frame
// of the reference instant); table: the frame's W entries of SP_TABLE doubles, or null for a static sensor.  Returns 1 when the frame takes part
// (and D, I, Wt have moved), 0 otherwise.  *cls: the drop class (PJ_KEEP also for a kept centre whose pixel is empty or lies behind the
// truncation band); *evals: the evaluations of the search, 0 for a centre that is not finite in the reference frame.
MH_HD int sf_fuse(const double* T, float cx, float cy, float cz, const double* table, const PjRule& R, const double* inc, const MhFrame& f,
                  double trunc, double* D, double* I, double* Wt, int* cls, int* evals)
{
#pragma clang fp contract(off)
    double p[3], q[3];
    *cls = PJ_INVALID; *evals = 0;
    pj_transform(T, cx, cy, cz, p);
    if (!(pj_finite(p[0]) && pj_finite(p[1]) && pj_finite(p[2]))) return 0;
    int w, h;
    float r32;
    const int state = sp_search(p, table, R, q, &w, evals);            // every column it reads the table at comes from sp_column_of: within [0, W)
    *cls = sp_classify(q, state, R, inc, &h, &r32);
    if (*cls != PJ_KEEP) return 0;
    if (w < 0 || w >= R.W || h < 0 || h >= R.H) return 0;              // never a pixel outside the image, whatever the inclination holds
    const long long px = (long long)h * R.W + w;
    if (!f.mask[px]) return 0;
    const float dep = f.depth[px];
    if (!(dep > 0.f)) return 0;
    const double sdf = (double)dep - (double)r32;
    if (sdf < -trunc) return 0;
    const double s = sdf / trunc;
    const double d = s < 1.0 ? s : 1.0;
    const double wt = *Wt;
    *D = (wt * *D + d) / (wt + 1.0);
    if (f.intensity) *I = (wt * *I + (double)f.intensity[px]) / (wt + 1.0);
    *Wt = wt + 1.0;
    return 1;
}

#endif /* LRT_SWEEPFUSE_MATH_H_INCLUDED */
