// Host build of the ray-gradient half of lrt_math.h (lrt_hit_ray_backward, lrt_sh_basis_vjp) for tests/test_ray_grad_host.py:
// single hits, single basis vectors, and a brute-force per-ray loop that sums the per-hit terms the way the kernels do.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../lidar_rt_amd/csrc/lrt_math.h"

extern "C" void rg_hit(const float* o, const float* d, float t, const float* mu, const float* sc, const float* q, float mod,
                       float dL_dG, float dL_dD_gs, float* out6 /* dL/do, dL/dd */)
{
    LrtHitGeom hg; lrt_hit_geom(o, d, t, mu, sc, q, mod, &hg);
    for (int i = 0; i < 6; i++) out6[i] = 0.f;
    lrt_hit_ray_backward(&hg, d, t, dL_dG, dL_dD_gs, out6, out6 + 3);
}

extern "C" void rg_sh_vjp(int deg, const float* d, const float* dL_db, float* out3)
{
    for (int i = 0; i < 3; i++) out3[i] = 0.f;
    lrt_sh_basis_vjp(deg, d, dL_db, out3);
}

// Per ray: the forward (sorted brute-force hits, 16-hit chunks), then the backward's per-hit dL/dalpha as tests/host_check/host_check.cpp
// forms it, and the ray gradient summed over the composited hits plus the colour term once per ray.
extern "C" int rg_trace(int P, const float* means, const float* scales, const float* rots, const float* opac, float mod, int n_rays,
                        const float* ray_o, const float* ray_d, int M, int deg, const float* shs, const float* bg, const float* dL_dout,
                        float* out9, float* d_ray_o, float* d_ray_d)
{
    std::vector<float> rec((size_t)P * LRT_REC_FLOATS);
    for (int g = 0; g < P; g++) {
        LrtSplatAux aux;
        lrt_make_splat(means + 3 * g, scales + 2 * g, rots + 4 * g, opac[g], mod, g, rec.data() + (size_t)g * LRT_REC_FLOATS, &aux);
    }
    const int nsh = (deg + 1) * (deg + 1);
    struct Hit { float t, ao; int g; };
    for (int r = 0; r < n_rays; r++) {
        const float* o = ray_o + 3 * r; const float* d = ray_d + 3 * r;
        std::vector<Hit> hits;
        for (int g = 0; g < P; g++) {
            float t, ao;
            if (lrt_splat_hit(rec.data() + (size_t)g * LRT_REC_FLOATS, o, d, &t, &ao) && t >= LRT_T_NEAR) hits.push_back({t, ao, g});
        }
        std::sort(hits.begin(), hits.end(), [](const Hit& a, const Hit& b) { return a.t < b.t; });
        // the composited hits, in order, with their weights and colours (forward)
        struct Comp { Hit h; float T, alpha, w, c[3]; bool cl0; };
        std::vector<Comp> comp;
        float b[16] = {0};
        lrt_sh_basis(deg, d, b);
        {
            float T = 1.f, base = -1.f; size_t pos = 0; bool stop = false;
            while (!stop) {
                while (pos < hits.size() && !(hits[pos].t > base)) pos++;
                const size_t n = std::min<size_t>(16, hits.size() - pos), beyond = hits.size() - pos;
                float last_t = base;
                for (size_t i = 0; i < n && !stop; i++) {
                    const Hit& h = hits[pos + i];
                    last_t = h.t;
                    const float alpha = fminf(LRT_ALPHA_MAX, h.ao);
                    if (!(alpha >= LRT_ALPHA_MIN)) continue;
                    const float testT = T * (1.f - alpha);
                    if (testT < LRT_T_STOP) { stop = true; break; }
                    Comp c; c.h = h; c.T = T; c.alpha = alpha; c.w = alpha * T;
                    const float* sh = shs + (size_t)h.g * M * 3;
                    for (int ch = 0; ch < 3; ch++) { c.c[ch] = 0.5f; for (int k = 0; k < nsh; k++) c.c[ch] += b[k] * sh[3 * k + ch]; }
                    c.cl0 = c.c[0] < 0.f; c.c[0] = fmaxf(c.c[0], 0.f);
                    comp.push_back(c);
                    T = testT;
                }
                if (stop || beyond < 16) break;
                pos += n;
                base = last_t + LRT_STEP_EPS;
            }
            float* op_ = out9 + 9 * r;
            float C[3] = {0, 0, 0}, D = 0.f, W = 0.f;
            for (const Comp& c : comp) { for (int ch = 0; ch < 3; ch++) C[ch] += c.w * c.c[ch]; D += c.w * c.h.t; W += c.w; }
            for (int ch = 0; ch < 3; ch++) op_[ch] = C[ch] + T * bg[ch];
            op_[3] = D; op_[4] = W; op_[5] = op_[6] = op_[7] = 0.f; op_[8] = T;
        }
        // backward
        const float* dL = dL_dout + 9 * r; const float* fin = out9 + 9 * r;
        const float dL_dbg = dL[0] * bg[0] + dL[1] * bg[1] + dL[2] * bg[2];
        float C[3] = {0, 0, 0}, N[3] = {0, 0, 0}, Dd = 0.f, go[3] = {0, 0, 0}, gd[3] = {0, 0, 0}, db[16] = {0};
        for (const Comp& c : comp) {
            const int g = c.h.g;
            LrtHitGeom hg; lrt_hit_geom(o, d, c.h.t, means + 3 * g, scales + 2 * g, rots + 4 * g, mod, &hg);
            const float nrm[3] = {hg.R[2], hg.R[5], hg.R[8]};
            for (int ch = 0; ch < 3; ch++) { C[ch] += c.w * c.c[ch]; N[ch] += c.w * nrm[ch]; }
            Dd += c.w * c.h.t;
            const float i1a = 1.f / (1.f - c.alpha);
            float dLa = 0.f;
            for (int ch = 0; ch < 3; ch++) dLa += dL[ch] * (c.T * c.c[ch] - (fin[ch] - C[ch]) * i1a);
            dLa += dL_dbg * (-fin[8] * i1a);
            dLa += dL[3] * (c.T * c.h.t - (fin[3] - Dd) * i1a);
            for (int ch = 0; ch < 3; ch++) dLa += dL[5 + ch] * (c.T * nrm[ch] - (fin[5 + ch] - N[ch]) * i1a);
            dLa *= (c.h.ao > LRT_ALPHA_MAX) ? 0.f : 1.f;
            lrt_hit_ray_backward(&hg, d, c.h.t, opac[g] * dLa, dL[3] * c.w, go, gd);
            const float rr[3] = {c.cl0 ? 0.f : dL[0] * c.w, dL[1] * c.w, dL[2] * c.w};
            const float* sh = shs + (size_t)g * M * 3;
            for (int k = 0; k < nsh; k++) db[k] += rr[0] * sh[3 * k] + rr[1] * sh[3 * k + 1] + rr[2] * sh[3 * k + 2];
        }
        lrt_sh_basis_vjp(deg, d, db, gd);
        for (int i = 0; i < 3; i++) { d_ray_o[3 * r + i] = go[i]; d_ray_d[3 * r + i] = gd[i]; }
    }
    return 0;
}
