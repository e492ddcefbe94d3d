// Stand-alone host build of lidar_rt_amd/csrc/lrt_init_math.h for tests/test_scene_init.py (g++, its own main; may be built with
// -fsanitize=address,undefined): reads from standard input an int64 count n and n symmetric 3 x 3 matrices as 6 float64 each
// (xx, xy, xz, yy, yz, zz), and writes to standard output, per matrix, 7 float64: the unit eigenvector of the smallest eigenvalue, the three
// eigenvalues in ascending order, and the routine's return value (0: rank < 2 or not finite, the vector is the (0, 0, 1) fall-back).
// With the argument "cov" the input is n lists of 8 float32 points (24 float32) and an int32 count each, and the covariance of the first
// `count` points is formed by in_covariance first.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_init_math.h"

int main(int argc, char** argv)
{
    const bool from_points = argc > 1 && std::strcmp(argv[1], "cov") == 0;
    int64_t n = 0;
    if (std::fread(&n, sizeof n, 1, stdin) != 1 || n < 0 || n > (int64_t(1) << 26)) { std::fprintf(stderr, "init_check: bad count\n"); return 2; }
    std::vector<double> out((size_t)n * 7);
    for (int64_t i = 0; i < n; i++) {
        double c[6], v[3], lam[3];
        if (from_points) {
            float p[3 * IN_KMAX]; int32_t cnt = 0;
            if (std::fread(p, sizeof(float), 3 * IN_KMAX, stdin) != 3 * IN_KMAX || std::fread(&cnt, sizeof cnt, 1, stdin) != 1 || cnt < 1 || cnt > IN_KMAX) {
                std::fprintf(stderr, "init_check: short or bad point list %lld\n", (long long)i); return 2;
            }
            in_covariance(p, cnt, c);
        } else if (std::fread(c, sizeof(double), 6, stdin) != 6) { std::fprintf(stderr, "init_check: short input at matrix %lld\n", (long long)i); return 2; }
        const int rc = in_smallest_eigenvector(c, v, lam);
        double* o = out.data() + (size_t)i * 7;
        o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = lam[0]; o[4] = lam[1]; o[5] = lam[2]; o[6] = (double)rc;
    }
    if (n > 0 && std::fwrite(out.data(), sizeof(double), out.size(), stdout) != out.size()) return 3;
    return 0;
}
