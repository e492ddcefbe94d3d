// beams_check.cpp -- lrt_beams_math.h compiled for the host (g++ -ffp-contract=off): the rule's text evaluated on one case read from a file.
//   in:  int32 F, H, W, n_inc, has_twist, 0, 0, 0; float64 off, yaw; float32 pose (F, 12), twist (F, 6) if has_twist, inc (n_inc), tau (W),
//        beams (H, 2), g_o (F, H, W, 3), g_d (F, H, W, 3)
//   out: float32 ray_o (F, H, W, 3), ray_d (F, H, W, 3), d_pose (F, 12), d_twist (F, 6), d_beams (H, 2)
// The sums run in the order of lrt_beams.hip up to the cross-lane steps: rows within a column, columns within a frame, frames.  Prints "BEAMSCHECK ok".
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cmath>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_beams_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: beams_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int32_t> hd = rd<int32_t>(f, 8);
    const int F = hd[0], H = hd[1], W = hd[2], n_inc = hd[3], has_twist = hd[4];
    const std::vector<double> dd = rd<double>(f, 2);
    const double off = dd[0], yaw = dd[1];
    const std::vector<float> pose = rd<float>(f, (size_t)F * 12), twist = rd<float>(f, has_twist ? (size_t)F * 6 : 0), inc = rd<float>(f, n_inc), tau = rd<float>(f, W),
                             beams = rd<float>(f, (size_t)H * 2);
    const size_t n3 = (size_t)F * H * W * 3;
    const std::vector<float> g_o = rd<float>(f, n3), g_d = rd<float>(f, n3);
    fclose(f);

    std::vector<double> row((size_t)H * 4), db((size_t)H * 2, 0.0);
    std::vector<float> ray_o(n3), ray_d(n3), d_pose((size_t)F * 12), d_twist((size_t)F * 6), d_beams((size_t)H * 2);
    for (int h = 0; h < H; h++) bm_row(h, H, inc.data(), n_inc, off, beams.data(), row.data() + 4 * h);
    for (int fr = 0; fr < F; fr++) {
        const float* P = pose.data() + 12 * fr;
        const float* xi = has_twist ? twist.data() + 6 * fr : nullptr;
        double out[18];
        for (int k = 0; k < 18; k++) out[k] = 0.0;
        for (int w = 0; w < W; w++) {
            const double s = xi ? (double)tau[w] : 0.0;
            double R[9], t[3], sa, ca, A[3], B[3], cx[3];
            sw_column_pose(P, xi, s, R, t);
            sincos(sw_azimuth(w, W, off, yaw), &sa, &ca);
            sw_column_axes(R, ca, sa, A, cx);
            bm_column_axis(R, ca, sa, B);
            double Gp[3] = {0, 0, 0}, Gq[3] = {0, 0, 0}, Gc[3] = {0, 0, 0}, Gt[3] = {0, 0, 0};
            for (int h = 0; h < H; h++) {
                const size_t r = 3 * (((size_t)fr * H + h) * W + w);
                const double* rw = row.data() + 4 * h;
                double ah[3], d[3], n, gv[3], ge, gd;
                bm_row_axis(A, B, rw[2], rw[3], ah);
                sw_ray(ah, cx, rw[0], rw[1], d, &n);
                const double g[3] = {(double)g_d[r], (double)g_d[r + 1], (double)g_d[r + 2]};
                sw_ray_bwd(d, n, g, gv);
                bm_ray_beam_bwd(A, B, cx, ah, rw, gv, &ge, &gd);
                db[2 * h] += ge; db[2 * h + 1] += gd;
                const double wp = rw[0] * rw[2], wq = rw[0] * rw[3];
                for (int i = 0; i < 3; i++) {
                    ray_d[r + i] = (float)d[i];
                    ray_o[r + i] = (float)t[i];
                    Gp[i] += wp * gv[i]; Gq[i] += wq * gv[i]; Gc[i] += rw[1] * gv[i]; Gt[i] += (double)g_o[r + i];
                }
            }
            bm_column_bwd(P, xi, s, ca, sa, Gp, Gq, Gc, Gt, out, out + 12);
        }
        for (int k = 0; k < 12; k++) d_pose[12 * fr + k] = (float)out[k];
        for (int k = 0; k < 6; k++) d_twist[6 * fr + k] = (float)out[12 + k];
    }
    for (size_t k = 0; k < db.size(); k++) d_beams[k] = (float)db[k];
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(ray_o.data(), sizeof(float), n3, o);
    fwrite(ray_d.data(), sizeof(float), n3, o);
    fwrite(d_pose.data(), sizeof(float), d_pose.size(), o);
    fwrite(d_twist.data(), sizeof(float), d_twist.size(), o);
    fwrite(d_beams.data(), sizeof(float), d_beams.size(), o);
    fclose(o);
    printf("BEAMSCHECK ok\n");
    return 0;
}
