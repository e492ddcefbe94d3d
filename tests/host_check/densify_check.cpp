// Host program for tests/test_fused_densify.py: lidar_rt_amd/csrc/lrt_densify_math.h, the text the kernels run, compiled for the host and run over
// the rows of one asset that the test wrote; the test compares what comes back with the float64 twin (lidar_rt_amd.densify.densify_reference).
//
//   densify_check IN OUT
//   IN : int32 P, S, size_limit, has_box; float32 grad_thr, big_thr, huge_thr, opa_thr, box_min[3], box_max[3]; then float32 arrays
//        xyz (P, 3), scaling (P, S), rotation (P, 4), opacity (P), accum (P), denom (P), split_noise (P, 2, 3), box_noise (P, 2, 2, 3),
//        mean_grads (P, 3), weights (P)
//   OUT: uint32 code (P); float32 child_xyz (P, 2, 3), child_scaling (P, S), accum + |mean_grad| (P), denom + (weight > 0) (P)
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_densify_math.h"

static bool rd(FILE* f, void* p, size_t n) { return n == 0 || std::fread(p, 1, n, f) == n; }

int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: densify_check IN OUT\n"); return 2; }
    FILE* f = std::fopen(argv[1], "rb");
    if (!f) { std::perror(argv[1]); return 2; }
    int32_t h[4];
    float t[10];
    if (!rd(f, h, sizeof h) || !rd(f, t, sizeof t)) { std::fprintf(stderr, "short header\n"); return 2; }
    const int P = h[0], S = h[1];
    if (P < 0 || P > (1 << 24) || (S != 2 && S != 3)) { std::fprintf(stderr, "bad header\n"); return 2; }
    LrtDensifyRule r;
    r.grad_thr = t[0]; r.big_thr = t[1]; r.huge_thr = t[2]; r.opa_thr = t[3]; r.size_limit = h[2]; r.has_box = h[3];
    for (int k = 0; k < 3; k++) { r.box_min[k] = t[4 + k]; r.box_max[k] = t[7 + k]; }
    const size_t n = (size_t)P;
    std::vector<float> xyz(3 * n), sc((size_t)S * n), q(4 * n), op(n), acc(n), den(n), sn(6 * n), bn(12 * n), mg(3 * n), w(n);
    std::vector<float>* arrs[] = {&xyz, &sc, &q, &op, &acc, &den, &sn, &bn, &mg, &w};
    for (auto* a : arrs) if (!rd(f, a->data(), a->size() * 4)) { std::fprintf(stderr, "short input\n"); return 2; }
    std::fclose(f);
    std::vector<uint32_t> code(n);
    std::vector<float> cx(6 * n), cs((size_t)S * n), acc2(n), den2(n);
    for (size_t i = 0; i < n; i++) {
        code[i] = lrt_densify_row(&xyz[3 * i], &sc[S * i], S, &q[4 * i], op[i], acc[i], den[i], &sn[6 * i], &bn[12 * i], r);
        lrt_densify_children(&xyz[3 * i], &sc[S * i], S, &q[4 * i], &sn[6 * i], &cx[6 * i]);
        for (int k = 0; k < S; k++) cs[S * i + k] = lrt_densify_child_scaling(sc[S * i + k]);
        acc2[i] = lrt_densify_accumulate(acc[i], mg[3 * i], mg[3 * i + 1], mg[3 * i + 2]);
        den2[i] = den[i] + (w[i] > 0.f ? 1.f : 0.f);
    }
    FILE* o = std::fopen(argv[2], "wb");
    if (!o) { std::perror(argv[2]); return 2; }
    std::fwrite(code.data(), 4, n, o); std::fwrite(cx.data(), 4, cx.size(), o); std::fwrite(cs.data(), 4, cs.size(), o);
    std::fwrite(acc2.data(), 4, n, o); std::fwrite(den2.data(), 4, n, o);
    std::fclose(o);
    std::printf("DENSIFYCHECK ok|%d rows|S %d\n", P, S);
    return 0;
}
