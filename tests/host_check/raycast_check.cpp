// raycast_check.cpp -- lrt_raycast_math.h compiled for the host (g++ -ffp-contract=off): the rule rc_ray on sampled rays of a grid, from a file.
//
//   in : int32 X, Y, Z, min_weight, N, has_intensity, 0, 0; float64 voxel, origin x, y, z, step, far_step, min_depth, max_depth;
//        float32 tsdf[X Y Z]; int32 weight[X Y Z]; float32 intensity[X Y Z] (has_intensity); float32 ray_o[N 3]; float32 ray_d[N 3]
//   out: float32 depth[N]; uint8 hit[N]; float32 intensity[N]; int32 samples[N]
//
// Prints "RAYCHECK ok".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_raycast_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "raycast_check: short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: raycast_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = rd<int>(f, 8);
    const std::vector<double> par = rd<double>(f, 8);
    const int X = hd[0], Y = hd[1], Z = hd[2], N = hd[4], has_int = hd[5];
    if (X < 1 || Y < 1 || Z < 1 || N < 0) { fprintf(stderr, "raycast_check: bad header\n"); return 2; }
    const size_t V = (size_t)X * Y * Z;
    const std::vector<float> tsdf = rd<float>(f, V);
    const std::vector<int> weight = rd<int>(f, V);
    const std::vector<float> inten = rd<float>(f, has_int ? V : 0);
    const std::vector<float> ro = rd<float>(f, 3 * (size_t)N), rdir = rd<float>(f, 3 * (size_t)N);
    fclose(f);
    RcGrid g;
    g.X = X; g.Y = Y; g.Z = Z; g.min_weight = hd[3]; g.voxel = par[0]; g.ox = par[1]; g.oy = par[2]; g.oz = par[3];
    g.tsdf = tsdf.data(); g.weight = weight.data(); g.intensity = has_int ? inten.data() : nullptr;
    RcParams P;
    P.step = par[4]; P.far_step = par[5]; P.min_depth = par[6]; P.max_depth = par[7];
    std::vector<float> depth(N), oi(N);
    std::vector<unsigned char> hit(N);
    std::vector<int> ns(N);
    for (int q = 0; q < N; q++) {
        const RcOut r = rc_ray(g, P, ro.data() + 3 * (size_t)q, rdir.data() + 3 * (size_t)q);
        depth[q] = r.depth; hit[q] = r.hit; oi[q] = r.intensity; ns[q] = r.samples;
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(depth.data(), sizeof(float), N, o); fwrite(hit.data(), 1, N, o); fwrite(oi.data(), sizeof(float), N, o); fwrite(ns.data(), sizeof(int), N, o);
    fclose(o);
    printf("RAYCHECK ok\n");
    return 0;
}
