// Host build of lidar_rt_amd/csrc/lrt_gridcd_math.h for tests/test_grid_chamfer.py (g++ -ffp-contract=off): the point formation, the pair
// distance and the two box bounds, on arrays.
#include "../../lidar_rt_amd/csrc/lrt_gridcd_math.h"

extern "C" {

// out[i] = gc_point(o[i], d[i], r[i])
void gc_points(int n, const float* o, const float* d, const float* r, float* out)
{
    for (int i = 0; i < n; i++) out[i] = gc_point(o[i], d[i], r[i]);
}

// q, p: (n, 3) queries and candidates; out[i] = gc_d2(p - q)
void gc_pairs(int n, const float* q, const float* p, float* out)
{
    for (int i = 0; i < n; i++) out[i] = gc_d2(gc_sub(p[3 * i], q[3 * i]), gc_sub(p[3 * i + 1], q[3 * i + 1]), gc_sub(p[3 * i + 2], q[3 * i + 2]));
}

// lo, hi, q: (n, 3); out[i] = gc_bound(box i, query i)
void gc_bounds(int n, const float* lo, const float* hi, const float* q, float* out)
{
    for (int i = 0; i < n; i++)
        out[i] = gc_bound(lo[3 * i], lo[3 * i + 1], lo[3 * i + 2], hi[3 * i], hi[3 * i + 1], hi[3 * i + 2], q[3 * i], q[3 * i + 1], q[3 * i + 2]);
}

// lo, hi: (n, 3) candidate boxes; qlo, qhi: (n, 3) query boxes; out[i] = gc_bound_box
void gc_bounds_box(int n, const float* lo, const float* hi, const float* qlo, const float* qhi, float* out)
{
    for (int i = 0; i < n; i++)
        out[i] = gc_bound_box(lo[3 * i], lo[3 * i + 1], lo[3 * i + 2], hi[3 * i], hi[3 * i + 1], hi[3 * i + 2], qlo[3 * i], qlo[3 * i + 1], qlo[3 * i + 2],
                              qhi[3 * i], qhi[3 * i + 1], qhi[3 * i + 2]);
}

float gc_empty(void) { return GC_EMPTY; }
float gc_big(void) { return GC_BIG; }

}  // extern "C"
