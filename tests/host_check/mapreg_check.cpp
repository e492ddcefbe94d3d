// mapreg_check.cpp -- lrt_mapreg_math.h (with lrt_raycast_math.h, lrt_reg_math.h and lrt_project_math.h) compiled for the host
// (g++ -ffp-contract=off): every source pixel of every frame through mr_pixel, for tests/test_map_registration.py to compare with the numpy twin
// bit for bit.
//
//   in:  8 int32   X Y Z F H W min_weight hostile
//        3 float64 voxel trunc huber
//        pose (F, 12) float64, tsdf (X Y Z) float32, weight (X Y Z) int32, points (F, H W, 3) float32, mask (F, H W) uint8
//   out: cell (F, H W) int64 (-1: no term), e and n (F, H W, 4) float64, terms (F, H W, 30) float64 -- zeros without a term --,
//        inverse (F, 12) float64: mr_inverse of every pose
//
// hostile != 0: after the pass above the rule runs over inputs made to break it -- points that are NaN, infinite or huge, points exactly on and
// one ulp outside every face of the domain, poses full of NaN, and grids of 0, 1 and 2 voxels along an axis (the arrays then hold exactly the
// voxels the dims name, so that a read past them is a read past a heap block).  Nothing is written for them; the sanitizers are the check.
// Prints "MAPREGCHECK ok".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <limits>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_mapreg_math.h"

template <typename T>
static std::vector<T> get(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "mapreg_check: short input\n"); exit(2); }
    return v;
}

static RcGrid grid_of(int X, int Y, int Z, int mw, double voxel, const float* ts, const int* wt)
{
    RcGrid g;
    g.X = X; g.Y = Y; g.Z = Z; g.min_weight = mw; g.voxel = voxel; g.ox = g.oy = g.oz = 0.0;
    g.tsdf = ts; g.weight = wt; g.intensity = nullptr;
    return g;
}

static long long hostile(double voxel, double trunc, double huber, const double* pose)
{
    const float nan = std::numeric_limits<float>::quiet_NaN(), inf = std::numeric_limits<float>::infinity();
    const double eye[12] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0};
    double bad[12];
    for (int k = 0; k < 12; k++) bad[k] = k == 5 ? (double)nan : eye[k];
    const int dims[][3] = {{0, 3, 3}, {1, 4, 5}, {3, 1, 2}, {2, 2, 1}, {2, 2, 2}, {2, 5, 3}, {4, 2, 7}, {5, 6, 2}, {6, 5, 4}};
    long long n = 0, terms = 0;
    for (const auto& d : dims) {
        const size_t N = (size_t)d[0] * d[1] * d[2];
        std::vector<float> ts(N);
        std::vector<int> wt(N);
        for (size_t v = 0; v < N; v++) { ts[v] = (float)((int)(v * 7 % 11) - 5) / 5.f; wt[v] = v % 13 == 0 ? 0 : 1; }
        const RcGrid g = grid_of(d[0], d[1], d[2], 1, voxel, ts.data(), wt.data());
        std::vector<float> vals = {nan, inf, -inf, 3.0e38f, -3.0e38f, 0.f, -0.f, 1e-30f};
        for (int a = 0; a < 3; a++) {
            const int m = d[a] > 0 ? d[a] : 1;
            for (int i : {0, m - 2, m - 1}) {
                if (i < 0) continue;
                const float c = rc_centre(voxel, i);
                vals.push_back(c); vals.push_back(nextafterf(c, inf)); vals.push_back(nextafterf(c, -inf));
            }
        }
        double t[RG_NSUM], en[4];
        for (float x : vals) for (float y : vals) for (float z : vals) {
            const float p[3] = {x, y, z};
            for (const double* X : {eye, pose, (const double*)bad}) {
                terms += mr_pixel(g, trunc, X, p, huber, t, en) >= 0;
                n++;
            }
        }
    }
    printf("hostile: %lld samples, %lld with a term\n", n, terms);
    return n;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: mapreg_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = get<int>(f, 8);
    const std::vector<double> dd = get<double>(f, 3);
    const int X = hd[0], Y = hd[1], Z = hd[2], F = hd[3], H = hd[4], W = hd[5], mw = hd[6];
    if (X < 1 || Y < 1 || Z < 1 || F < 1 || H < 1 || W < 1 || mw < 1) { fprintf(stderr, "mapreg_check: bad header\n"); return 2; }
    const size_t N = (size_t)X * Y * Z, HW = (size_t)H * W;
    const std::vector<double> pose = get<double>(f, 12 * (size_t)F);
    const std::vector<float> ts = get<float>(f, N);
    const std::vector<int> wt = get<int>(f, N);
    const std::vector<float> sp = get<float>(f, 3 * F * HW);
    const std::vector<unsigned char> sm = get<unsigned char>(f, F * HW);
    fclose(f);
    const RcGrid g = grid_of(X, Y, Z, mw, dd[0], ts.data(), wt.data());
    std::vector<long long> cell(F * HW, -1);
    std::vector<double> en(4 * F * HW, 0.0), terms((size_t)RG_NSUM * F * HW, 0.0), inv(12 * (size_t)F);
    for (int fr = 0; fr < F; fr++) {
        for (size_t i = 0; i < HW; i++) {
            const size_t k = fr * HW + i;
            if (!sm[k]) continue;
            double t[RG_NSUM], e4[4];
            const long long b = mr_pixel(g, dd[1], pose.data() + 12 * fr, sp.data() + 3 * k, dd[2], t, e4);
            if (b < 0) continue;
            cell[k] = b;
            memcpy(en.data() + 4 * k, e4, sizeof e4);
            memcpy(terms.data() + RG_NSUM * k, t, sizeof t);
        }
        mr_inverse(pose.data() + 12 * fr, inv.data() + 12 * fr);
    }
    if (hd[7]) hostile(dd[0], dd[1], dd[2], pose.data());
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(cell.data(), sizeof(long long), cell.size(), o);
    fwrite(en.data(), sizeof(double), en.size(), o);
    fwrite(terms.data(), sizeof(double), terms.size(), o);
    fwrite(inv.data(), sizeof(double), inv.size(), o);
    fclose(o);
    printf("MAPREGCHECK ok\n");
    return 0;
}
