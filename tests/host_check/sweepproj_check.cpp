// Host program for tests/test_sweep_project.py: lidar_rt_amd/csrc/lrt_sweepproj_math.h, the text the kernels run, compiled for the host and run
// over the points that the test wrote; the test compares what comes back with the float64 twin
// (lidar_rt_amd.sweep_project.project_points_sweep_reference).
//
//   sweepproj_check IN OUT
//   IN : int32 N, F, H, W, n_inc, wrap, has_transform, has_twist; float64 off, yaw, min_depth, max_depth; int64 offsets (F + 1); float64
//        inclination (n_inc); float64 points2sensor (F, 3, 4) if has_transform; float64 twist (F, 6) and tau (W) if has_twist; float32 points (N, 4)
//   OUT: int32 (N, 5): w, h, bits(r32), drop class, evaluations of every point (w = h = -1 for a dropped point, bits = 0 for an invalid one)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_sweepproj_math.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: sweepproj_check IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t h[8];
    double d[4];
    if (!rd(f, h, sizeof h) || !rd(f, d, sizeof d)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int N = h[0], F = h[1];
    PjRule R;
    R.H = h[2]; R.W = h[3]; R.n_inc = h[4]; R.wrap = h[5];
    R.off = d[0]; R.yaw = d[1]; R.min_depth = d[2]; R.max_depth = d[3];
    if (N < 0 || N > (1 << 24) || F < 1 || F > (1 << 16) || R.H < 1 || R.W < 1 || R.W > (1 << 16) || (R.n_inc != 2 && (R.n_inc != R.H || R.H < 3))) {
        std::fprintf(stderr, "bad header\n"); return 2;
    }
    const bool has_T = h[6] != 0, has_twist = h[7] != 0;
    std::vector<int64_t> off((size_t)F + 1);
    std::vector<double> inc((size_t)R.n_inc), T(has_T ? (size_t)F * 12 : 0), xi(has_twist ? (size_t)F * 6 : 0), tau(has_twist ? (size_t)R.W : 0);
    std::vector<float> pts((size_t)N * 4);
    if (!rd(f, off.data(), off.size() * 8) || !rd(f, inc.data(), inc.size() * 8) || !rd(f, T.data(), T.size() * 8) || !rd(f, xi.data(), xi.size() * 8)
        || !rd(f, tau.data(), tau.size() * 8) || !rd(f, pts.data(), pts.size() * 4)) {
        std::fprintf(stderr, "short input\n"); return 2;
    }
    std::fclose(f);
    if (off[0] != 0 || off[F] != N) { std::fprintf(stderr, "bad offsets\n"); return 2; }
    std::vector<double> table(has_twist ? (size_t)F * R.W * SP_TABLE : 0);           // what k_swproj_table writes
    if (has_twist)
        for (int fr = 0; fr < F; fr++)
            for (int w = 0; w < R.W; w++) sp_column_entry(&xi[(size_t)fr * 6], tau[w], &table[((size_t)fr * R.W + w) * SP_TABLE]);
    std::vector<int32_t> out((size_t)N * 5);
    for (int fr = 0; fr < F; fr++) {
        if (off[fr + 1] < off[fr]) { std::fprintf(stderr, "bad offsets\n"); return 2; }
        for (int64_t i = off[fr]; i < off[fr + 1]; i++) {
            int w, row, evals;
            float r32;
            const int cls = sp_point(has_T ? &T[(size_t)fr * 12] : nullptr, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2],
                                     has_twist ? &table[(size_t)fr * R.W * SP_TABLE] : nullptr, R, inc.data(), &w, &row, &r32, &evals);
            uint32_t bits;
            std::memcpy(&bits, &r32, 4);
            out[5 * i] = w; out[5 * i + 1] = row; out[5 * i + 2] = (int32_t)bits; out[5 * i + 3] = cls; out[5 * i + 4] = evals;
        }
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    std::fwrite(out.data(), 4, out.size(), o);
    std::fclose(o);
    std::printf("SWEEPPROJCHECK ok|%d points|%d frames|%d x %d|%s\n", N, F, R.H, R.W, has_twist ? "twist" : "static");
    return 0;
}
