// Host build of lidar_rt_amd/csrc/lrt_loss_math.h for tests/test_fused_loss.py: the window, the SSIM value with its three partials (float64 and
// float32 instantiations) and the ray-drop probability / BCE with its logit derivative, over arrays.
#include "../../lidar_rt_amd/csrc/lrt_loss_math.h"

extern "C" {

void lc_window(float* w) { const LrtLossWindow g = lrt_loss_window(); for (int i = 0; i < LRT_LOSS_WIN; i++) w[i] = g.w[i]; }

// in: n rows of (mu1, mu2, e11, e22, e12); out: n rows of (S, dS/dmu1, dS/de11, dS/de12)
void lc_ssim_f64(int n, const double* in, double* out)
{
    for (int i = 0; i < n; i++) lrt_loss_ssim<double>(in[5 * i], in[5 * i + 1], in[5 * i + 2], in[5 * i + 3], in[5 * i + 4], out + 4 * i, out + 4 * i + 1, out + 4 * i + 2, out + 4 * i + 3);
}

void lc_ssim_f32(int n, const float* in, float* out)
{
    for (int i = 0; i < n; i++) lrt_loss_ssim<float>(in[5 * i], in[5 * i + 1], in[5 * i + 2], in[5 * i + 3], in[5 * i + 4], out + 4 * i, out + 4 * i + 1, out + 4 * i + 2, out + 4 * i + 3);
}

// out: n rows of (p, BCE, dBCE/d drop logit)
void lc_bce(int n, const float* hit, const float* drop, const float* label, int use_rayhit, float* out)
{
    for (int i = 0; i < n; i++) {
        const float p = lrt_loss_prob(hit[i], drop[i], use_rayhit);
        out[3 * i] = p; out[3 * i + 1] = lrt_loss_bce(p, label[i], out + 3 * i + 2);
    }
}

}
