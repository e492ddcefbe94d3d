// reg_check.cpp -- lrt_reg_math.h compiled for the host (g++ -ffp-contract=off): the rule's text evaluated on one pair read from a file.
//
//   in : int32 H, W, n_inc, rh, rw, 0, 0, 0; float64 off, yaw, min_depth, max_depth, max_dist, huber, lambda, min_pairs, tol_t, tol_r;
//        float64 inc[n_inc], X[12]; float32 src_points[H W 3]; uint8 src_mask[H W]; float32 tgt_points[H W 3], tgt_normals[H W 3]; uint8 tgt_mask[H W]
//   out: int32 assoc[H W]; float64 sums[30] (the pixels in ascending order); int32 status, 0; float64 X'[12], |rho|, |phi| of one rg_solve
//
// Prints "REGCHECK ok".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_reg_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "reg_check: short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: reg_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = rd<int>(f, 8);
    const std::vector<double> par = rd<double>(f, 10);
    const int H = hd[0], W = hd[1], n_inc = hd[2], rh = hd[3], rw = hd[4];
    if (H < 1 || W < 1 || (n_inc != 2 && n_inc != H) || rh < 0 || rh > 4 || rw < 0 || rw > 16) { fprintf(stderr, "reg_check: bad header\n"); return 2; }
    const size_t HW = (size_t)H * W;
    const std::vector<double> inc = rd<double>(f, n_inc);
    std::vector<double> X = rd<double>(f, 12);
    const std::vector<float> sp = rd<float>(f, 3 * HW);
    const std::vector<unsigned char> sm = rd<unsigned char>(f, HW);
    const std::vector<float> tp = rd<float>(f, 3 * HW), tn = rd<float>(f, 3 * HW);
    const std::vector<unsigned char> tm = rd<unsigned char>(f, HW);
    fclose(f);
    PjRule R;
    R.H = H; R.W = W; R.n_inc = n_inc; R.wrap = 1; R.off = par[0]; R.yaw = par[1]; R.min_depth = par[2]; R.max_depth = par[3];
    std::vector<int> assoc(HW, -1);
    double sums[RG_NSUM];
    for (int k = 0; k < RG_NSUM; k++) sums[k] = 0.0;
    for (size_t i = 0; i < HW; i++) {
        if (!sm[i]) continue;
        double t[RG_NSUM];
        for (int k = 0; k < RG_NSUM; k++) t[k] = 0.0;
        assoc[i] = rg_pixel(X.data(), sp.data() + 3 * i, R, inc.data(), tp.data(), tn.data(), tm.data(), rh, rw, par[4] * par[4], par[5], t);
        for (int k = 0; k < RG_NSUM; k++) sums[k] += t[k];
    }
    double norms[2];
    const int st[2] = {rg_solve(sums, par[6], par[7], par[8], par[9], X.data(), norms), 0};
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(assoc.data(), sizeof(int), HW, o);
    fwrite(sums, sizeof(double), RG_NSUM, o);
    fwrite(st, sizeof(int), 2, o);
    fwrite(X.data(), sizeof(double), 12, o);
    fwrite(norms, sizeof(double), 2, o);
    fclose(o);
    printf("REGCHECK ok\n");
    return 0;
}
