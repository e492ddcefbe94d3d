// unproject_check.cpp -- lrt_unproject_math.h on the host: the class and the point bits of every pixel of a case, for tests/test_unproject.py.
//
//   unproject_check IN OUT
//
// IN:  int32 F, H, W, has_keep, has_drop, tmode (0 none, 1 per frame, 2 per column); float64 ratio, min_depth, max_depth;
//      float32 depth[F H W], rays_o[F H W 3], rays_d[F H W 3]; uint8 keep[F H W] if has_keep; float32 raydrop[F H W] if has_drop;
//      float64 T[F 12] or T[F W 12] by tmode.
// OUT: per pixel four int32: class, bits of x, y, z (0 for a pixel that is not kept).
// Compile with -ffp-contract=off: every operation rounds on its own, as the header asks of the device compiler.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../lidar_rt_amd/csrc/lrt_unproject_math.h"

template <class T>
static bool read_n(FILE* f, std::vector<T>& v, size_t n)
{
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: unproject_check IN OUT\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    int32_t hdr[6];
    double par[3];
    if (fread(hdr, sizeof hdr, 1, f) != 1 || fread(par, sizeof par, 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int F = hdr[0], H = hdr[1], W = hdr[2], has_keep = hdr[3], has_drop = hdr[4], tmode = hdr[5];
    if (F < 1 || H < 1 || W < 1 || tmode < 0 || tmode > 2) { fprintf(stderr, "bad header\n"); return 2; }
    const size_t hw = (size_t)H * W, n = (size_t)F * hw;
    std::vector<float> depth, o, d, drop;
    std::vector<unsigned char> keep;
    std::vector<double> T;
    bool ok = read_n(f, depth, n) && read_n(f, o, 3 * n) && read_n(f, d, 3 * n);
    if (ok && has_keep) ok = read_n(f, keep, n);
    if (ok && has_drop) ok = read_n(f, drop, n);
    if (ok && tmode) ok = read_n(f, T, (tmode == 1 ? (size_t)F : (size_t)F * W) * 12);
    fclose(f);
    if (!ok) { fprintf(stderr, "short input\n"); return 2; }
    UpRule R;
    R.has_keep = has_keep; R.has_drop = has_drop; R.ratio = (float)par[0]; R.min_depth = par[1]; R.max_depth = par[2];
    std::vector<int32_t> out(4 * n, 0);
    for (size_t i = 0; i < n; i++) {
        const size_t fr = i / hw, w = (i % hw) % W;
        const int cls = up_classify(depth[i], &o[3 * i], &d[3 * i], has_keep ? keep[i] : (unsigned char)1, has_drop ? drop[i] : 0.f, R);
        out[4 * i] = cls;
        if (cls != UP_KEEP) continue;
        float p[3];
        if (tmode == 0) up_point32(depth[i], &o[3 * i], &d[3 * i], p);
        else up_point64(depth[i], &o[3 * i], &d[3 * i], &T[12 * (tmode == 1 ? fr : fr * W + w)], p);
        memcpy(&out[4 * i + 1], p, 12);
    }
    FILE* g = fopen(argv[2], "wb");
    if (!g || fwrite(out.data(), sizeof(int32_t), out.size(), g) != out.size()) { perror(argv[2]); return 2; }
    fclose(g);
    printf("UNPROJECTCHECK ok %zu pixels\n", n);
    return 0;
}
