// lrt_refine_math.h -- the small rules of the ray-drop refinement network that the host and the device share (include/lrt_refine.h states the
// network): the level sizes, the channel counts of the eight convolution pairs, the parameter and workspace layouts, the bilinear source
// coordinate.  Float32 as the reference's network; the order of every operation is fixed here.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define RF_HD __host__ __device__ inline
#else
#define RF_HD inline
#endif

constexpr int RF_LEVELS = 5;
constexpr int RF_PAIRS = 8;                                          // down1 .. down4, up1 .. up4

// Channel counts (in, mid, out) of pair i in units of c, and the level it writes.
inline void rf_pair_channels(int i, int c, int* ci, int* cm, int* co, int* level)
{
    const int in_[RF_PAIRS] = {1, 2, 4, 8, 16, 8, 4, 2}, out_[RF_PAIRS] = {2, 4, 8, 8, 4, 2, 1, 1}, lvl[RF_PAIRS] = {1, 2, 3, 4, 3, 2, 1, 0};
    *ci = in_[i] * c; *co = out_[i] * c; *cm = i < 4 ? *co : *ci; *level = lvl[i];
}

// Bilinear x2 with aligned corners: the source coordinate of destination index `dst` is dst * scale, scale = (in - 1) / (2 in - 1) in float32
// (0 for a source of size 1); i0 = floor, i1 = min(i0 + 1, in - 1), the weight of i1 is the fraction.
RF_HD float rf_up_scale(int n_in) { return n_in > 1 ? (float)(n_in - 1) / (float)(2 * n_in - 1) : 0.0f; }

RF_HD void rf_up_coord(int dst, float scale, int n_in, int* i0, int* i1, float* frac)
{
    const float s = scale * (float)dst;
    int a = (int)s;
    if (a > n_in - 1) a = n_in - 1;
    *i0 = a;
    *i1 = a + 1 < n_in ? a + 1 : n_in - 1;
    *frac = s - (float)a;
}

// The workspace: every intermediate of one frame, channels-last (pixel, channel), each at a multiple of 64 floats.
enum { RF_X0 = 0, RF_M1, RF_X1, RF_M2, RF_X2, RF_M3, RF_X3, RF_M4, RF_X4, RF_QKV, RF_HB, RF_X4A, RF_U3M, RF_Y3, RF_U2M, RF_Y2, RF_U1M, RF_Y1, RF_U0M, RF_Y0, RF_NBUF };

struct RfPlan {
    int H[RF_LEVELS], W[RF_LEVELS];
    long long n[RF_LEVELS];                                          // pixels of a level
    long long off[RF_NBUF + 1];                                      // float offsets into the workspace; off[RF_NBUF] is the total
};

inline void rf_plan(int H, int W, int c, RfPlan* p)
{
    for (int l = 0; l < RF_LEVELS; l++) { p->H[l] = H >> l; p->W[l] = W >> l; p->n[l] = (long long)p->H[l] * p->W[l]; }
    const int level[RF_NBUF] = {0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 4, 4, 3, 3, 2, 2, 1, 1, 0, 0};
    const int chan[RF_NBUF] = {1, 2, 2, 4, 4, 8, 8, 8, 8, 24, 8, 8, 16, 4, 8, 2, 4, 1, 2, 1};
    long long o = 0;
    for (int b = 0; b < RF_NBUF; b++) {
        p->off[b] = o;
        o += (p->n[level[b]] * chan[b] * c + 63) / 64 * 64;
    }
    p->off[RF_NBUF] = o;
}

inline long long rf_param_count(int Cin, int c)
{
    long long n = (long long)Cin * c + c;
    for (int i = 0; i < RF_PAIRS; i++) {
        int ci, cm, co, lvl;
        rf_pair_channels(i, c, &ci, &cm, &co, &lvl);
        n += 2LL * ci + 9LL * ci * cm + 2LL * cm + 9LL * cm * co;
    }
    return n + 16LL * c + 8LL * c * 24 * c + 8LL * c * 8 * c + 2LL * c + c + 1;
}
