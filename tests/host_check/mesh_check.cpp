// mesh_check.cpp -- lrt_mesh_math.h (with lrt_project_math.h) compiled for the host (g++ -ffp-contract=off): the fusion rule evaluated on sampled
// voxels and the vertex rule on sampled edges, from a file.
//
//   in : int32 X, Y, Z, F, H, W, n_inc, n_vox, n_edge, has_intensity, 0, 0; float64 voxel, trunc, off, yaw, min_depth, max_depth, 0, 0;
//        float64 T[F 12]; float64 inc[n_inc]; float32 depth[F H W]; uint8 mask[F H W]; float32 frame_intensity[F H W] (has_intensity);
//        float32 tsdf[N]; int32 weight[N]; float32 intensity[N]; int32 voxels[n_vox]; int32 edges[n_edge 2] (v, axis)
//   out: float32 tsdf[n_vox]; int32 weight[n_vox]; float32 intensity[n_vox] (after one call over the F frames);
//        float32 vertices[n_edge 3]; float32 vertex_intensity[n_edge] (of the input state)
//
// Prints "MESHCHECK ok".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_mesh_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "mesh_check: short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: mesh_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = rd<int>(f, 12);
    const std::vector<double> par = rd<double>(f, 8);
    const int X = hd[0], Y = hd[1], Z = hd[2], F = hd[3], H = hd[4], W = hd[5], n_inc = hd[6], n_vox = hd[7], n_edge = hd[8], has_int = hd[9];
    if (X < 1 || Y < 1 || Z < 1 || F < 0 || H < 1 || W < 1 || !(n_inc == 2 || n_inc == H) || n_vox < 0 || n_edge < 0) { fprintf(stderr, "mesh_check: bad header\n"); return 2; }
    const size_t N = (size_t)X * Y * Z, HW = (size_t)H * W;
    const std::vector<double> T = rd<double>(f, 12 * (size_t)F), inc = rd<double>(f, n_inc);
    const std::vector<float> depth = rd<float>(f, F * HW);
    const std::vector<unsigned char> mask = rd<unsigned char>(f, F * HW);
    const std::vector<float> fint = rd<float>(f, has_int ? F * HW : 0);
    const std::vector<float> tsdf = rd<float>(f, N);
    const std::vector<int> weight = rd<int>(f, N);
    const std::vector<float> inten = rd<float>(f, N);
    const std::vector<int> vox = rd<int>(f, n_vox), edges = rd<int>(f, 2 * (size_t)n_edge);
    fclose(f);
    PjRule R;
    R.H = H; R.W = W; R.n_inc = n_inc; R.wrap = 1; R.off = par[2]; R.yaw = par[3]; R.min_depth = par[4]; R.max_depth = par[5];
    const double voxel = par[0], trunc = par[1];
    std::vector<float> o_tsdf(n_vox), o_int(n_vox), o_vert(3 * (size_t)n_edge), o_vint(n_edge);
    std::vector<int> o_w(n_vox);
    for (int s = 0; s < n_vox; s++) {
        const int v = vox[s], i = v / (Y * Z), j = (v / Z) % Y, k = v % Z;
        double D = tsdf[v], Wt = weight[v], I = inten[v];
        int seen = 0;
        for (int fr = 0; fr < F; fr++) {
            MhFrame m;
            m.depth = depth.data() + fr * HW; m.mask = mask.data() + fr * HW; m.intensity = has_int ? fint.data() + fr * HW : nullptr;
            seen |= mh_fuse(T.data() + 12 * fr, mh_centre(voxel, i), mh_centre(voxel, j), mh_centre(voxel, k), R, inc.data(), m, trunc, &D, &I, &Wt);
        }
        o_tsdf[s] = seen ? (float)D : tsdf[v];
        o_w[s] = seen ? (int)Wt : weight[v];
        o_int[s] = seen && has_int ? (float)I : inten[v];
    }
    for (int s = 0; s < n_edge; s++) {
        const int v = edges[2 * s], ax = edges[2 * s + 1];
        const int idx[3] = {v / (Y * Z), (v / Z) % Y, v % Z}, dv[3] = {Y * Z, Z, 1};
        const int u = v + dv[ax];
        const double t = mh_t(tsdf[v], tsdf[u]);
        for (int q = 0; q < 3; q++) o_vert[3 * s + q] = mh_lerp(mh_centre(voxel, idx[q]), mh_centre(voxel, idx[q] + (q == ax)), t);
        o_vint[s] = mh_lerp(inten[v], inten[u], t);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(o_tsdf.data(), sizeof(float), n_vox, o); fwrite(o_w.data(), sizeof(int), n_vox, o); fwrite(o_int.data(), sizeof(float), n_vox, o);
    fwrite(o_vert.data(), sizeof(float), o_vert.size(), o); fwrite(o_vint.data(), sizeof(float), n_edge, o);
    fclose(o);
    printf("MESHCHECK ok\n");
    return 0;
}
