// sweep_check.cpp -- lrt_sweep_math.h compiled for the host (g++ -ffp-contract=off): the rule's text evaluated on one case read from a file.
//   in:  int32 F, H, W, n_inc, has_twist, 0, 0, 0; float64 off, yaw; float32 pose (F, 12), twist (F, 6) if has_twist, inc (n_inc), tau (W),
//        g_o (F, H, W, 3), g_d (F, H, W, 3)
//   out: float64 columns (F, W, 12) [R row-major, t]; float32 ray_o (F, H, W, 3), ray_d (F, H, W, 3), d_pose (F, 12), d_twist (F, 6)
// It also compares the series and the closed coefficients at the threshold and next to it, and prints "SWEEPCHECK ok".
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_sweep_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: sweep_check in out\n"); return 2; }
    // the two branches at the threshold
    const double us[3] = {SW_SERIES_TH2, SW_SERIES_TH2 * (1.0 - 1e-9), SW_SERIES_TH2 * (1.0 + 1e-9)};
    double worst = 0.0;
    for (double u : us) {
        double a[6], b[6];
        sw_coef_series(u, a);
        sw_coef_closed(u, b);
        for (int k = 0; k < 6; k++) worst = fmax(worst, fabs(a[k] - b[k]));
    }
    printf("SWEEPCHECK branches %.3e\n", worst);
    if (!(worst <= ldexp(1.0, -40))) { fprintf(stderr, "series and closed coefficients differ by %.3e at the threshold\n", worst); return 1; }

    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 8);
    const int F = hd[0], H = hd[1], W = hd[2], n_inc = hd[3], has_twist = hd[4];
    const std::vector<double> dd = rd<double>(f, 2);
    const double off = dd[0], yaw = dd[1];
    const std::vector<float> pose = rd<float>(f, (size_t)F * 12), twist = rd<float>(f, has_twist ? (size_t)F * 6 : 0), inc = rd<float>(f, n_inc), tau = rd<float>(f, W);
    const size_t n3 = (size_t)F * H * W * 3;
    const std::vector<float> g_o = rd<float>(f, n3), g_d = rd<float>(f, n3);
    fclose(f);

    std::vector<double> cols((size_t)F * W * 12), ci(H), si(H);
    std::vector<float> ray_o(n3), ray_d(n3), d_pose((size_t)F * 12), d_twist((size_t)F * 6);
    for (int h = 0; h < H; h++) sincos(sw_inclination(h, H, inc.data(), n_inc, off), &si[h], &ci[h]);
    for (int fr = 0; fr < F; fr++) {
        const float* P = pose.data() + 12 * fr;
        const float* xi = has_twist ? twist.data() + 6 * fr : nullptr;
        double out[18];
        for (int k = 0; k < 18; k++) out[k] = 0.0;
        for (int w = 0; w < W; w++) {
            const double s = xi ? (double)tau[w] : 0.0;
            double R[9], t[3], sa, ca, ax[3], cx[3];
            sw_column_pose(P, xi, s, R, t);
            sincos(sw_azimuth(w, W, off, yaw), &sa, &ca);
            sw_column_axes(R, ca, sa, ax, cx);
            double* c = cols.data() + 12 * ((size_t)fr * W + w);
            for (int k = 0; k < 9; k++) c[k] = R[k];
            for (int k = 0; k < 3; k++) c[9 + k] = t[k];
            double Ga[3] = {0, 0, 0}, Gc[3] = {0, 0, 0}, Gt[3] = {0, 0, 0};
            for (int h = 0; h < H; h++) {
                const size_t r = 3 * (((size_t)fr * H + h) * W + w);
                double d[3], n, gv[3];
                sw_ray(ax, cx, ci[h], si[h], d, &n);
                const double g[3] = {(double)g_d[r], (double)g_d[r + 1], (double)g_d[r + 2]};
                sw_ray_bwd(d, n, g, gv);
                for (int i = 0; i < 3; i++) {
                    ray_d[r + i] = (float)d[i];
                    ray_o[r + i] = (float)t[i];
                    Ga[i] += ci[h] * gv[i]; Gc[i] += si[h] * gv[i]; Gt[i] += (double)g_o[r + i];
                }
            }
            sw_column_bwd(P, xi, s, ca, sa, Ga, Gc, Gt, out, out + 12);
        }
        for (int k = 0; k < 12; k++) d_pose[12 * fr + k] = (float)out[k];
        for (int k = 0; k < 6; k++) d_twist[6 * fr + k] = (float)out[12 + k];
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(cols.data(), sizeof(double), cols.size(), o);
    fwrite(ray_o.data(), sizeof(float), n3, o);
    fwrite(ray_d.data(), sizeof(float), n3, o);
    fwrite(d_pose.data(), sizeof(float), d_pose.size(), o);
    fwrite(d_twist.data(), sizeof(float), d_twist.size(), o);
    fclose(o);
    printf("SWEEPCHECK ok\n");
    return 0;
}
