// Host program for tests/test_fused_adam.py: lidar_rt_amd/csrc/lrt_adam_math.h, the text the kernel runs, instantiated for float and compared element
// by element with the same text instantiated for double.  Seeded inputs; among them g = 0, m = v = 0, lr = 0 and the steps 1 and 1000.
//
// Bounds, from the number formats (u = 2^-24, half a float32 ulp relative):
//   exp_avg, exp_avg_sq   the float instantiation evaluates the line in double and rounds once: within half a float32 ulp of the double value
//                         (the float64 roundings of the line itself, ~1e-16 relative, are allowed for by the factor 1 + 1e-6).
//   parameter             update = step_size * m / (sqrt(v) / bc2_sqrt + eps).  Roundings to float32 on the way: the quotient lr / bc1 (1 u), m (1 u),
//                         the product (1 u), v (half of 1 u under the root), the root (1 u), bc2_sqrt and the quotient (2 u), the sum (1 u),
//                         the last quotient (1 u): below 9 u |update|; the subtraction adds 1 u |p|.
// Prints one line per case and the worst ratios; exit status 1 when a bound is missed.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../lidar_rt_amd/csrc/lrt_adam_math.h"

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static double uni()                                                  // splitmix64 -> [0, 1)
{
    uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; z ^= z >> 31;
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}
static float signed_log_uniform(double lo, double hi) { const double x = std::pow(10.0, lo + (hi - lo) * uni()); return (float)(uni() < 0.5 ? -x : x); }

static double ulp32(double x)                                        // spacing of float32 at |x| (the smallest normal's below it)
{
    int e; std::frexp(std::fabs(x) < 1.17549435e-38 ? 1.17549435e-38 : std::fabs(x), &e);
    return std::ldexp(1.0, e - 24);
}

int main()
{
    const double beta1 = 0.9, beta2 = 0.999, eps = 1e-15;
    const LrtAdamRule rule = lrt_adam_rule(beta1, beta2, eps);
    const double U = std::ldexp(1.0, -24);
    int bad = 0;
    const double steps[] = {1.0, 1000.0};
    const double lrs[] = {0.0, 1.6e-4, 2.5e-3, 5e-2};
    for (double step : steps) for (double lr : lrs) {
        const double bc1 = 1.0 - std::pow(beta1, step), bc2s = std::sqrt(1.0 - std::pow(beta2, step));
        const LrtAdamStep<float> sf = lrt_adam_step_of<float>(lr, bc1, bc2s);
        const LrtAdamStep<double> sd = lrt_adam_step_of<double>(lr, bc1, bc2s);
        double worst_m = 0, worst_v = 0, worst_p = 0;
        int kept = 0;
        const int n = 1000;
        for (int i = 0; i < n; i++) {
            const int kind = i % 5;                                  // 0: g = 0;  1: m = v = 0;  2: both;  3, 4: everything set
            const float g = (kind == 0 || kind == 2) ? 0.f : signed_log_uniform(-6, 2);
            const float m0 = (kind == 1 || kind == 2) ? 0.f : signed_log_uniform(-6, 2);
            const float v0 = (kind == 1 || kind == 2) ? 0.f : std::fabs(signed_log_uniform(-12, 4));
            const float p0 = signed_log_uniform(-3, 1);
            float pf = p0, mf = m0, vf = v0;
            double pd = p0, md = m0, vd = v0;
            lrt_adam_update<float>(pf, g, mf, vf, rule, sf);
            lrt_adam_update<double>(pd, (double)g, md, vd, rule, sd);
            const double em = std::fabs((double)mf - md) / ulp32(md), ev = std::fabs((double)vf - vd) / ulp32(vd);
            const double update = (double)p0 - pd;
            const double ep = std::fabs((double)pf - pd) / (U * (std::fabs(pd) + 9.0 * std::fabs(update)) + 1e-300);
            if (em > worst_m) worst_m = em;
            if (ev > worst_v) worst_v = ev;
            if (ep > worst_p) worst_p = ep;
            if (lr == 0.0) {                                          // the parameter's bits stay, the moments move
                uint32_t a, b; float q = p0; __builtin_memcpy(&a, &pf, 4); __builtin_memcpy(&b, &q, 4);
                if (a != b) { std::printf("lr = 0 moved a parameter: %a -> %a\n", (double)p0, (double)pf); bad++; }
                if (g != 0.f && !(mf != m0 && vf != v0)) { std::printf("lr = 0, g = %a: the moments did not move\n", (double)g); bad++; }
                kept++;
            }
            if (kind == 2 && !(mf == 0.f && vf == 0.f && pf == p0)) { std::printf("g = m = v = 0 changed something\n"); bad++; }
            if (!std::isfinite(pf) || !std::isfinite(mf) || !std::isfinite(vf)) { std::printf("non-finite result\n"); bad++; }
        }
        const double lim = 0.5 * (1.0 + 1e-6);
        const bool ok = worst_m <= lim && worst_v <= lim && worst_p <= 1.0;
        std::printf("ADAMCHECK|step %g|lr %g|%d elements|exp_avg %.4f ulp (<= 0.5)|exp_avg_sq %.4f ulp (<= 0.5)|parameter %.4f of its bound\n", step, lr, n, worst_m, worst_v, worst_p);
        if (!ok) bad++;
    }
    std::printf(bad ? "ADAMCHECK FAILED (%d)\n" : "ADAMCHECK ok\n", bad);
    return bad ? 1 : 0;
}
