// Host program for tests/test_actor_sweep.py: lidar_rt_amd/csrc/lrt_actorsweep_math.h, the text the kernels run, compiled for the host and run over
// the Gaussians that the test wrote; the test compares what comes back with the float64 twin (lidar_rt_amd.actor_sweep.actor_sweep_reference).
//
//   actorsweep_check IN OUT
//   IN : int32 P, A, W, has_twist; float64 off, yaw; int32 seg_start (A + 1); float32 poses (A, 8); float32 actor_twist (A, 6); float64 world2sensor (12);
//        float64 sensor_twist (6) if has_twist; float64 tau (W); float32 xyz (P, 3), rot_raw (P, 4), g_xyz (P, 3), g_rot (P, 4)
//   OUT: int32 (P, 3): column, state (3 = not searched), evaluations; float32 (P, 14): xyz_s, rot_s, d_xyz, d_rot_raw; float64 (P, 6): the Gaussian's
//        term of d_actor_twist
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_actorsweep_math.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: actorsweep_check IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t h[4];
    double d[2];
    if (!rd(f, h, sizeof h) || !rd(f, d, sizeof d)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int P = h[0], A = h[1], W = h[2];
    const bool has_twist = h[3] != 0;
    if (P < 0 || P > (1 << 24) || A < 1 || A > (1 << 16) || W < 1 || W > (1 << 20)) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int32_t> seg((size_t)A + 1);
    std::vector<float> poses((size_t)A * 8), twist((size_t)A * 6), xyz((size_t)P * 3), rot((size_t)P * 4), gx((size_t)P * 3), gr((size_t)P * 4);
    std::vector<double> w2s(12), xi(has_twist ? 6 : 0), tau((size_t)W);
    if (!rd(f, seg.data(), seg.size() * 4) || !rd(f, poses.data(), poses.size() * 4) || !rd(f, twist.data(), twist.size() * 4) || !rd(f, w2s.data(), 96)
        || !rd(f, xi.data(), xi.size() * 8) || !rd(f, tau.data(), tau.size() * 8) || !rd(f, xyz.data(), xyz.size() * 4) || !rd(f, rot.data(), rot.size() * 4)
        || !rd(f, gx.data(), gx.size() * 4) || !rd(f, gr.data(), gr.size() * 4)) {
        std::fprintf(stderr, "short input\n"); return 2;
    }
    std::fclose(f);
    std::vector<double> table((size_t)W * AS_TABLE);                 // what k_as_table writes
    for (int w = 0; w < W; w++) as_table_entry(w2s.data(), has_twist ? xi.data() : nullptr, tau[w], &table[(size_t)w * AS_TABLE]);
    PjRule R;
    R.H = 1; R.W = W; R.n_inc = 2; R.wrap = 1; R.off = d[0]; R.yaw = d[1]; R.min_depth = 0.0; R.max_depth = 0.0;
    std::vector<int32_t> oi((size_t)P * 3);
    std::vector<float> of((size_t)P * 14);
    std::vector<double> od((size_t)P * 6);
    for (int g = 0; g < P; g++) {
        int lo = 0, hi = A;                                          // as_asset of the kernels
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (seg[mid] <= g) lo = mid; else hi = mid; }
        const int a = lo;
        double eta[6];
        bool any = false;
        for (int k = 0; k < 6; k++) { eta[k] = (double)twist[(size_t)6 * a + k]; any = any || eta[k] != 0.0; }
        const bool live = any && poses[(size_t)8 * a + 7] != 0.f;
        const float* xf = &xyz[(size_t)3 * g];
        const float* rf = &rot[(size_t)4 * g];
        float* o = &of[(size_t)14 * g];
        for (int k = 0; k < 3; k++) { o[k] = xf[k]; o[7 + k] = gx[(size_t)3 * g + k]; }
        for (int k = 0; k < 4; k++) { o[3 + k] = rf[k]; o[10 + k] = gr[(size_t)4 * g + k]; }
        for (int k = 0; k < 6; k++) od[(size_t)6 * g + k] = 0.0;
        int col = -1, evals = 0, state = 3;
        if (live) {
            double Ra[9], ta[3];
            as_pose(&poses[(size_t)8 * a], Ra, ta);
            const double x[3] = {(double)xf[0], (double)xf[1], (double)xf[2]};
            state = as_search(x, Ra, ta, eta, w2s.data(), table.data(), tau.data(), R, &col, &evals);
            if (state != AS_INVALID && col >= 0 && col < W) {
                as_place(eta, tau[col], xf, rf, o, o + 3);
                const double gg[3] = {(double)o[7], (double)o[8], (double)o[9]}, hh[4] = {(double)o[10], (double)o[11], (double)o[12], (double)o[13]};
                double dx[3], dr[4];
                if (as_place_bwd(eta, tau[col], xf, rf, gg, hh, dx, dr, &od[(size_t)6 * g])) {
                    for (int k = 0; k < 3; k++) o[7 + k] = (float)dx[k];
                    for (int k = 0; k < 4; k++) o[10 + k] = (float)dr[k];
                }
            } else {
                col = -1;
            }
        }
        oi[(size_t)3 * g] = col; oi[(size_t)3 * g + 1] = state; oi[(size_t)3 * g + 2] = evals;
    }
    FILE* out = std::fopen(argv[2], "wb");
    if (!out) { std::perror(argv[2]); return 2; }
    std::fwrite(oi.data(), 4, oi.size(), out);
    std::fwrite(of.data(), 4, of.size(), out);
    std::fwrite(od.data(), 8, od.size(), out);
    std::fclose(out);
    std::printf("ACTORSWEEPCHECK ok|%d Gaussians|%d assets|%d columns|%s\n", P, A, W, has_twist ? "twist" : "static");
    return 0;
}
