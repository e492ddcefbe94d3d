// lrt_gridcd_math.h -- the float32 arithmetic contract of the grid Chamfer operator (include/lrt_gridcd.h), inline for host and device so that
// tests/host_check/gridcd_check.cpp can compile it with g++ (-ffp-contract=off) and compare it with numpy.
//
//   gc_point  a pixel's world point as torch forms it: o + d * r, a multiplication and an addition, two roundings, never one fma
//             (hipcc contracts a * b + c by default: the device side spells the roundings out)
//   gc_d2     a pair's squared distance, the expression of lrt_chamfer.h: fma(dz, dz, fma(dy, dy, dx * dx)), d = candidate - query
//   gc_bound  the same expression on the per-axis gaps max(lo - q, q - hi, 0) between a query and a box.  Float32 subtraction is monotonic and
//             odd (fl(-x) = -fl(x)), so for every point p with lo <= p <= hi the gap is <= |fl(p - q)| on each axis; multiplication and fma of
//             non-negative operands are monotonic, so gc_bound <= gc_d2 AS COMPUTED for every point in the box.  An inverted (empty) box
//             (lo = +GC_EMPTY, hi = -GC_EMPTY) has gaps of 1e30 whose squares overflow: its bound is +inf.
//   gc_bound_box  the same for a box of queries: a lower bound of gc_bound for every query inside it.
#ifndef LRT_GRIDCD_MATH_H_INCLUDED
#define LRT_GRIDCD_MATH_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__)
#define GC_HD __host__ __device__ __forceinline__
#else
#define GC_HD inline
#endif

#define GC_EMPTY 1e30f          // coordinate of a padding point / bound of an empty box: every distance to it overflows to +inf
#define GC_BIG 3.0e38f          // initial best: any finite pair distance of sane inputs is smaller, +inf is not

// One rounding per operation.  On the device __fmul_rn / __fadd_rn do not guarantee it: they are inline functions around a plain * and +
// that carry hipcc's default -ffp-contract=fast, and the compiler fuses them into one v_fma_f32 (seen in k_gc_points' code).  The pragma
// takes the `contract` flag off the operations written HERE, so they stay separate wherever these functions are inlined.
#if defined(__clang__)
#define GC_NO_CONTRACT _Pragma("clang fp contract(off)")
#else
#define GC_NO_CONTRACT
#endif
#if defined(__HIP_DEVICE_COMPILE__)
GC_HD float gc_mul(float a, float b) { GC_NO_CONTRACT return a * b; }
GC_HD float gc_add(float a, float b) { GC_NO_CONTRACT return a + b; }
GC_HD float gc_sub(float a, float b) { GC_NO_CONTRACT return a - b; }
GC_HD float gc_fma(float a, float b, float c) { return __fmaf_rn(a, b, c); }
#else
GC_HD float gc_mul(float a, float b) { GC_NO_CONTRACT volatile float r = a * b; return r; }      // volatile: whatever -ffp-contract says (g++)
GC_HD float gc_add(float a, float b) { GC_NO_CONTRACT volatile float r = a + b; return r; }
GC_HD float gc_sub(float a, float b) { GC_NO_CONTRACT volatile float r = a - b; return r; }
GC_HD float gc_fma(float a, float b, float c) { return fmaf(a, b, c); }
#endif

GC_HD float gc_point(float o, float d, float r) { return gc_add(o, gc_mul(d, r)); }

GC_HD float gc_d2(float dx, float dy, float dz) { return gc_fma(dz, dz, gc_fma(dy, dy, gc_mul(dx, dx))); }

GC_HD float gc_gap(float lo, float hi, float q) { return fmaxf(fmaxf(gc_sub(lo, q), gc_sub(q, hi)), 0.f); }

GC_HD float gc_bound(float lox, float loy, float loz, float hix, float hiy, float hiz, float qx, float qy, float qz)
{
    return gc_d2(gc_gap(lox, hix, qx), gc_gap(loy, hiy, qy), gc_gap(loz, hiz, qz));
}

// Box against box: the gaps max(lo - qhi, qlo - hi, 0).  For every query q with qlo <= q <= qhi they are <= gc_gap(lo, hi, q) (subtraction is
// monotonic in both operands), so gc_bound_box <= gc_bound of every query in the query box: a whole wavefront may skip a tile on it.
GC_HD float gc_bound_box(float lox, float loy, float loz, float hix, float hiy, float hiz, float qlx, float qly, float qlz, float qhx,
                         float qhy, float qhz)
{
    return gc_d2(fmaxf(fmaxf(gc_sub(lox, qhx), gc_sub(qlx, hix)), 0.f), fmaxf(fmaxf(gc_sub(loy, qhy), gc_sub(qly, hiy)), 0.f),
                 fmaxf(fmaxf(gc_sub(loz, qhz), gc_sub(qlz, hiz)), 0.f));
}

#endif /* LRT_GRIDCD_MATH_H_INCLUDED */
