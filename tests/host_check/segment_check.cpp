// segment_check.cpp -- lrt_segment_math.h compiled for the host (g++ -ffp-contract=off): the rules' text evaluated on one frame read from a file.
//
//   in : int32 H, W, n_inc, rh, rw, 0, 0, 0; float64 off, yaw, min_depth, max_depth, m_abs, m_rel, d_abs, c_h, c_v, up[3], z_lo, z_hi, slope, 0;
//        float64 inc[n_inc], X[12], pose[12]; float32 points[H W 3]; uint8 mask[H W]; float32 tgt_range[H W]; uint8 tgt_mask[H W]
//   out: uint8 ground[H W]; uint8 join_right[H W] (pixel (h, w) with (h, (w + 1) % W), both masked in), join_down[H W] (with (h + 1, w));
//        int8 ev[H W]; int64 quant[H W 3]; int64 actor_quant[H W 3] (llrint(R^T (p - t) * 1024) for `pose`)
//
// Prints "SEGCHECK ok".
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_segment_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "segment_check: short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: segment_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = rd<int>(f, 8);
    const std::vector<double> par = rd<double>(f, 16);
    const int H = hd[0], W = hd[1], n_inc = hd[2], rh = hd[3], rw = hd[4];
    if (H < 1 || W < 1 || (n_inc != 2 && n_inc != H) || rh < 0 || rh > 4 || rw < 0 || rw > 16) { fprintf(stderr, "segment_check: bad header\n"); return 2; }
    const size_t HW = (size_t)H * W;
    const std::vector<double> inc = rd<double>(f, n_inc), X = rd<double>(f, 12), pose = rd<double>(f, 12);
    const std::vector<float> p = rd<float>(f, 3 * HW);
    const std::vector<unsigned char> m = rd<unsigned char>(f, HW);
    const std::vector<float> tr = rd<float>(f, HW);
    const std::vector<unsigned char> tm = rd<unsigned char>(f, HW);
    fclose(f);
    PjRule R;
    R.H = H; R.W = W; R.n_inc = n_inc; R.wrap = 1; R.off = par[0]; R.yaw = par[1]; R.min_depth = par[2]; R.max_depth = par[3];
    const float da = (float)par[6], ch = (float)par[7], cv = (float)par[8];
    const float dabs2 = da * da, ch2 = ch * ch, cv2 = cv * cv;
    std::vector<unsigned char> ground(HW, 0), jr(HW, 0), jd(HW, 0);
    std::vector<signed char> ev(HW, -1);
    std::vector<long long> q(3 * HW), aq(3 * HW);
    for (int w = 0; w < W; w++) {
        SgGround s;
        s.have = 0; s.h = 0.0; s.g[0] = s.g[1] = s.g[2] = 0.0;
        for (int k = 0; k < H; k++) {
            const size_t i = (size_t)sg_row_at(k, H, inc.data(), n_inc) * W + w;
            if (m[i]) ground[i] = (unsigned char)sg_ground_step(p.data() + 3 * i, par.data() + 9, par[12], par[13], par[14], &s);
        }
    }
    for (int h = 0; h < H; h++)
        for (int w = 0; w < W; w++) {
            const size_t i = (size_t)h * W + w, r = (size_t)h * W + (w + 1) % W, d = i + W;
            if (W > 1 && m[i] && m[r]) jr[i] = sg_join(p.data() + 3 * i, p.data() + 3 * r, dabs2, ch2);
            if (h + 1 < H && m[i] && m[d]) jd[i] = sg_join(p.data() + 3 * i, p.data() + 3 * d, dabs2, cv2);
            if (m[i]) ev[i] = (signed char)sg_freespace(X.data(), p.data() + 3 * i, R, inc.data(), tr.data(), tm.data(), rh, rw, par[4], par[5]);
            double a[3];
            sg_actor_point(pose.data(), p.data() + 3 * i, a);
            for (int k = 0; k < 3; k++) { q[3 * i + k] = sg_quant(p[3 * i + k]); aq[3 * i + k] = sg_quant64(a[k]); }
        }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(ground.data(), 1, HW, o); fwrite(jr.data(), 1, HW, o); fwrite(jd.data(), 1, HW, o); fwrite(ev.data(), 1, HW, o);
    fwrite(q.data(), sizeof(long long), 3 * HW, o); fwrite(aq.data(), sizeof(long long), 3 * HW, o);
    fclose(o);
    printf("SEGCHECK ok\n");
    return 0;
}
