// lrt_unproject_math.h -- the rule of the point clouds of range images (include/lrt_unproject.h), inline for host and device so that
// tests/host_check/unproject_check.cpp can compile it with g++ (-ffp-contract=off) and compare it with numpy.
//
//   up_classify   the class of a pixel: invalid, masked, out_of_range or kept -- the first that applies
//   up_point32    p = o + d r in float32: the product rounded, then the sum rounded.  What the boolean-mask expression of
//                 RangeFrames.inverse_projection_with_range (lidar_rt_amd/training.py) gives, bit for bit
//   up_point64    (x, y, z) = o + d r in float64 (the product of two float32 is exact there), q = T (x, y, z, 1) for a 3 x 4 row-major T, each row
//                 summed left to right, rounded to float32 once -- lrt_project_math.h treats points2sensor the same way
//
// Far from the origin the float32 sum o + d r loses the low bits of d r: with |o| = 1.6 km the range recomputed from the point is off by up to
// |o| / r ulps.  up_point64 with T = (sensor pose)^-1 keeps them: the point's error is the one rounding of the result.
#ifndef LRT_UNPROJECT_MATH_H_INCLUDED
#define LRT_UNPROJECT_MATH_H_INCLUDED

#if defined(__HIPCC__) || defined(__CUDACC__)
#define UP_HD __host__ __device__ inline
#else
#define UP_HD inline
#endif

#define UP_KEEP 0
#define UP_INVALID 1
#define UP_MASKED 2
#define UP_OUT_OF_RANGE 3

struct UpRule {
    int has_keep, has_drop;
    float ratio;                                                 // (float) raydrop_ratio: torch compares a float32 tensor with a number in float32
    double min_depth, max_depth;
};

UP_HD bool up_finite(float x) { return x - x == 0.f; }

// r: the depth; o, d: the ray; keep, drop: read only where the rule has them.
UP_HD int up_classify(float r, const float* o, const float* d, unsigned char keep, float drop, const UpRule& R)
{
    if (!(up_finite(r) && up_finite(o[0]) && up_finite(o[1]) && up_finite(o[2]) && up_finite(d[0]) && up_finite(d[1]) && up_finite(d[2]))) return UP_INVALID;
    if (R.has_keep && keep == 0) return UP_MASKED;
    if (R.has_drop && !(drop < R.ratio)) return UP_MASKED;
    if (!((double)r > R.min_depth && (double)r <= R.max_depth)) return UP_OUT_OF_RANGE;
    return UP_KEEP;
}

UP_HD void up_point32(float r, const float* o, const float* d, float* p)
{
#pragma clang fp contract(off)                                   // every operation rounds on its own, on the device as on the host
    const float m0 = d[0] * r, m1 = d[1] * r, m2 = d[2] * r;
    p[0] = o[0] + m0;
    p[1] = o[1] + m1;
    p[2] = o[2] + m2;
}

UP_HD void up_point64(float r, const float* o, const float* d, const double* T, float* p)
{
#pragma clang fp contract(off)
    const double rr = (double)r;
    const double m0 = (double)d[0] * rr, m1 = (double)d[1] * rr, m2 = (double)d[2] * rr;
    const double x = (double)o[0] + m0, y = (double)o[1] + m1, z = (double)o[2] + m2;
    const double q0 = T[0] * x + T[1] * y + T[2] * z + T[3];
    const double q1 = T[4] * x + T[5] * y + T[6] * z + T[7];
    const double q2 = T[8] * x + T[9] * y + T[10] * z + T[11];
    p[0] = (float)q0;
    p[1] = (float)q1;
    p[2] = (float)q2;
}

#endif /* LRT_UNPROJECT_MATH_H_INCLUDED */
