// Host build of lidar_rt_amd/csrc/lrt_metrics_math.h for tests/test_fused_metrics.py (g++ -ffp-contract=off): the clamped pairs, the window
// term with the kernel's order of summation (7-tap row sums, then 7 rows), and the rank selection the way the kernels drive it: per level a
// histogram of the keys that carry each rank's prefix, scanned in chunks of a thread's few bins.
#include "../../lidar_rt_amd/csrc/lrt_metrics_math.h"
#include <vector>

extern "C" {

// image 0: depth, image 1: intensity.  x[i], y[i] = the clamped prediction / ground truth, key[i] = the selection key of y - x
void mt_pairs(int n, int image, const float* pred, const float* gt, const unsigned char* mask, float max_depth, float* x, float* y, uint32_t* key)
{
    for (int i = 0; i < n; i++) {
        const bool m = mask[i] != 0;
        if (image == 0) { y[i] = mt_depth_gt(gt[i], max_depth); x[i] = mt_depth_pred(pred[i], m, max_depth); }
        else { y[i] = mt_intensity_gt(gt[i]); x[i] = mt_intensity_pred(pred[i], m); }
        key[i] = mt_abs_key(y[i] - x[i]);
    }
}

// sums: (H - 6, W - 6, 5) window sums of x, y, x^2, y^2, x y; returns the mean window term
double mt_ssim_image(int H, int W, const float* x, const float* y, double R, double* sums)
{
    const int OH = H - (MT_WIN - 1), OW = W - (MT_WIN - 1);
    std::vector<double> row((size_t)5 * H * OW);
    for (int r = 0; r < H; r++)
        for (int q = 0; q < OW; q++) {
            double s[5] = {0, 0, 0, 0, 0};
            for (int t = 0; t < MT_WIN; t++) {
                const double a = (double)x[r * W + q + t], b = (double)y[r * W + q + t];
                s[0] += a; s[1] += b; s[2] += a * a; s[3] += b * b; s[4] += a * b;
            }
            for (int m = 0; m < 5; m++) row[((size_t)m * H + r) * OW + q] = s[m];
        }
    double acc = 0;
    for (int r = 0; r < OH; r++)
        for (int q = 0; q < OW; q++) {
            double s[5];
            for (int m = 0; m < 5; m++) {
                double v = 0;
                for (int t = 0; t < MT_WIN; t++) v += row[((size_t)m * H + r + t) * OW + q];
                s[m] = v; sums[((size_t)r * OW + q) * 5 + m] = v;
            }
            acc += mt_ssim_window(s, R);
        }
    return acc / ((double)OH * OW);
}

// mt_find_bin on a whole histogram
int mt_find(const uint32_t* h, int nb, uint32_t before, uint32_t k, uint32_t* rank_in_bin) { return mt_find_bin(h, nb, before, k, rank_in_bin); }

// ... and the way a scan's threads call it: each on `per` bins with its exclusive prefix.  Returns the bin, or -1 - (number of threads that
// claimed the rank) if that number is not 1.
int mt_find_chunked(const uint32_t* h, int nb, int per, uint32_t k, uint32_t* rank_in_bin)
{
    int found = 0, bin = -1;
    uint32_t before = 0;
    for (int t = 0; t < nb / per; t++) {
        uint32_t r = 0;
        const int b = mt_find_bin(h + t * per, per, before, k, &r);
        if (b >= 0) { found++; bin = t * per + b; *rank_in_bin = r; }
        for (int i = 0; i < per; i++) before += h[t * per + i];
    }
    return found == 1 ? bin : -1 - found;
}

// The three-level selection over n keys: keys_out[2] = the elements of rank (n - 1) / 2 and n / 2 of the sorted keys; *split = the first level
// whose scan put the two ranks into different bins (0: never); returns 0, or the level at which a rank was not found.
int mt_select(int n, const uint32_t* keys, uint32_t* keys_out, int* split)
{
    uint32_t prefix[2] = {0, 0}, rank[2] = {mt_rank_lo((uint32_t)n), mt_rank_hi((uint32_t)n)};
    *split = 0;
    for (int level = 1; level <= 3; level++) {
        const int nb = level == 1 ? MT_L1_BINS : level == 2 ? MT_L2_BINS : MT_L3_BINS, per = nb / 256;
        for (int s = 0; s < 2; s++) {
            std::vector<uint32_t> h(nb, 0u);
            for (int i = 0; i < n; i++)
                if (mt_prefix(keys[i], level) == prefix[s]) h[mt_digit(keys[i], level)]++;
            uint32_t r = 0;
            const int b = mt_find_chunked(h.data(), nb, per, rank[s], &r);
            if (b < 0) return level;
            prefix[s] = mt_extend(prefix[s], (uint32_t)b, level); rank[s] = r;
        }
        if (*split == 0 && prefix[0] != prefix[1]) *split = level;
    }
    keys_out[0] = prefix[0]; keys_out[1] = prefix[1];
    return 0;
}

float mt_median_of(uint32_t lo, uint32_t hi) { return mt_median(lo, hi); }
double mt_window(const double* s, double R) { return mt_ssim_window(s, R); }
double mt_f1_of(double tp, double fp, double fn) { return mt_f1(tp, fp, fn); }
double mt_fscore_of(double ba, double na, double bb, double nb) { return mt_fscore(ba, na, bb, nb); }
double mt_psnr_of(double sum_sq, double n, double peak) { return mt_psnr(sum_sq, n, peak); }
double mt_rmse_of(double sum_sq, double n) { return mt_rmse(sum_sq, n); }

}  // extern "C"
