// Host program for tests/test_range_image.py: lidar_rt_amd/csrc/lrt_project_math.h, the text the kernels run, compiled for the host and run over
// the points that the test wrote; the test compares what comes back with the float64 twin (lidar_rt_amd.range_image.project_points_reference).
//
//   project_check IN OUT
//   IN : int32 N, F, H, W, n_inc, wrap, has_transform, 0; float64 off, yaw, min_depth, max_depth; int64 offsets (F + 1); float64 inclination
//        (n_inc); float64 points2sensor (F, 3, 4) if has_transform; float32 points (N, 4)
//   OUT: int32 (N, 4): w, h, bits(r32), drop class of every point (w = h = -1 for a dropped point, bits = 0 for an invalid one)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_project_math.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: project_check IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t h[8];
    double d[4];
    if (!rd(f, h, sizeof h) || !rd(f, d, sizeof d)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int N = h[0], F = h[1];
    PjRule R;
    R.H = h[2]; R.W = h[3]; R.n_inc = h[4]; R.wrap = h[5];
    R.off = d[0]; R.yaw = d[1]; R.min_depth = d[2]; R.max_depth = d[3];
    if (N < 0 || N > (1 << 24) || F < 1 || F > (1 << 16) || R.H < 1 || R.W < 1 || (R.n_inc != 2 && (R.n_inc != R.H || R.H < 3))) { std::fprintf(stderr, "bad header\n"); return 2; }
    std::vector<int64_t> off((size_t)F + 1);
    std::vector<double> inc((size_t)R.n_inc), T(h[6] ? (size_t)F * 12 : 0);
    std::vector<float> pts((size_t)N * 4);
    if (!rd(f, off.data(), off.size() * 8) || !rd(f, inc.data(), inc.size() * 8) || !rd(f, T.data(), T.size() * 8) || !rd(f, pts.data(), pts.size() * 4)) {
        std::fprintf(stderr, "short input\n"); return 2;
    }
    std::fclose(f);
    if (off[0] != 0 || off[F] != N) { std::fprintf(stderr, "bad offsets\n"); return 2; }
    std::vector<int32_t> out((size_t)N * 4);
    for (int fr = 0; fr < F; fr++) {
        if (off[fr + 1] < off[fr]) { std::fprintf(stderr, "bad offsets\n"); return 2; }
        for (int64_t i = off[fr]; i < off[fr + 1]; i++) {
            double q[3];
            pj_transform(h[6] ? &T[(size_t)fr * 12] : nullptr, pts[4 * i], pts[4 * i + 1], pts[4 * i + 2], q);
            int w, row;
            float r32;
            const int cls = pj_classify(q, R, inc.data(), &w, &row, &r32);
            uint32_t bits;
            std::memcpy(&bits, &r32, 4);
            out[4 * i] = w; out[4 * i + 1] = row; out[4 * i + 2] = (int32_t)bits; out[4 * i + 3] = cls;
        }
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    std::fwrite(out.data(), 4, out.size(), o);
    std::fclose(o);
    std::printf("PROJECTCHECK ok|%d points|%d frames|%d x %d\n", N, F, R.H, R.W);
    return 0;
}
