// lrt_place_math.h -- the rules of the place matcher (include/lrt_place.h): the one text for the device (lrt_place.hip) and the host
// (tests/host_check/place_check.cpp, g++ -ffp-contract=off).
//
//   pl_cell      one valid pixel: is it kept, its ring and its cell value (the sector is integer arithmetic on the column: pl_sector)
//   pl_sector    (w * NS) / W
//   pl_padded    NR rounded up to a multiple of 4: the bytes of one sector
//   pl_sad4      the sum of the absolute differences of the four bytes of two words, added to acc
//   pl_key       D << 7 | s: the smaller key is the smaller D, and among equal D the smaller shift
//
// Float64 with every operation rounded on its own.
#ifndef LRT_PLACE_MATH_H_INCLUDED
#define LRT_PLACE_MATH_H_INCLUDED

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PL_HD __host__ __device__ inline
#else
#define PL_HD inline
#endif

#define PL_MAX_RINGS 32
#define PL_MAX_SECTORS 128
#define PL_SHIFT_BITS 7
#define PL_NO_KEY 0x7fffffff

struct PlRule {
    int NR, NS;
    double up[3], r_min, r_max, z_lo, z_step;
};

PL_HD int pl_padded(int NR) { return (NR + 3) / 4 * 4; }

PL_HD int pl_sector(int w, int NS, int W) { return (int)(((long long)w * NS) / W); }

// 1 and (*ring, *value) for a kept pixel, 0 otherwise.  A NaN coordinate makes rho or h a NaN and every comparison false.
PL_HD int pl_cell(const float* p, const PlRule& R, int* ring, int* value)
{
#pragma clang fp contract(off)
    const double x = (double)p[0], y = (double)p[1], z = (double)p[2];
    const double h = R.up[0] * x + R.up[1] * y + R.up[2] * z;
    const double gx = x - h * R.up[0], gy = y - h * R.up[1], gz = z - h * R.up[2];
    const double rho = sqrt(gx * gx + gy * gy + gz * gz);
    if (!(rho >= R.r_min && rho < R.r_max && h >= R.z_lo)) return 0;
    const double fr = floor((rho - R.r_min) * (double)R.NR / (R.r_max - R.r_min));
    *ring = fr >= (double)(R.NR - 1) ? R.NR - 1 : (int)fr;
    const double fv = floor((h - R.z_lo) / R.z_step);
    *value = fv >= 254.0 ? 255 : 1 + (int)fv;
    return 1;
}

PL_HD unsigned pl_sad4(unsigned a, unsigned b, unsigned acc)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int k = 0; k < 4; k++) {
        const int x = (int)((a >> (8 * k)) & 255u), y = (int)((b >> (8 * k)) & 255u);
        acc += (unsigned)(x > y ? x - y : y - x);
    }
    return acc;
#endif
}

PL_HD int pl_key(unsigned D, int s) { return (int)((D << PL_SHIFT_BITS) | (unsigned)s); }

#endif /* LRT_PLACE_MATH_H_INCLUDED */
