// sweepfuse_check.cpp -- lrt_sweepfuse_math.h (with lrt_mesh_math.h and lrt_sweepproj_math.h) compiled for the host (g++ -ffp-contract=off): one
// call of the fusion under the sweep model over every voxel of a grid, from a file.  The column table is formed as the device forms it:
// sp_column_entry(twist[f], tau[w]) per frame and column, the identity without a twist.
//
//   in : int32 X, Y, Z, F, H, W, n_inc, has_intensity, has_twist, hostile, 0, 0; float64 voxel, trunc, off, yaw, min_depth, max_depth, 0, 0;
//        float64 T[F 12]; float64 inc[n_inc]; float64 twist[F 6], tau[W] (has_twist); float32 depth[F H W]; uint8 mask[F H W];
//        float32 frame_intensity[F H W] (has_intensity); float32 tsdf[N]; int32 weight[N]; float32 intensity[N] (has_intensity)
//   out: float32 tsdf[N]; int32 weight[N]; float32 intensity[N] (has_intensity); int64 unseen, fused, evals[SP_MAX_EVAL + 1]
//
// hostile: after the call, the same voxels run again over inputs that no caller may send past the checks but that the rule must survive without
// reading outside its arrays -- a NaN twist, infinite and huge column times, a huge yaw (columns far outside [0, W) before the range check), a
// NaN and a non-monotonic inclination.  Their results are discarded; a sanitizer build reports any read outside the table or the images.
//
// Prints "SWEEPFUSECHECK ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_sweepfuse_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "sweepfuse_check: short input\n"); exit(2); }
    return v;
}

struct Call {
    int X, Y, Z, F, H, W, has_int;
    double voxel, trunc;
    PjRule R;
    const double *T, *inc;
    const float *depth, *fint;
    const unsigned char* mask;
};

// The exactly sized table of one call: W entries per frame, nothing behind them.
static std::vector<double> make_table(int F, int W, const double* twist, const double* tau)
{
    std::vector<double> table((size_t)F * W * SP_TABLE);
    for (int f = 0; f < F; f++)
        for (int w = 0; w < W; w++) {
            double* E = table.data() + ((size_t)f * W + w) * SP_TABLE;
            if (twist) sp_column_entry(twist + 6 * f, tau[w], E); else sf_identity(E);
        }
    return table;
}

static void run(const Call& c, const std::vector<double>& table, const float* tsdf, const int* weight, const float* inten, float* o_tsdf, int* o_w,
                float* o_int, long long* counts)
{
    const size_t HW = (size_t)c.H * c.W;
    for (int v = 0; v < c.X * c.Y * c.Z; v++) {
        const int i = v / (c.Y * c.Z), j = (v / c.Z) % c.Y, k = v % c.Z;
        double D = tsdf[v], Wt = weight[v], I = c.has_int ? inten[v] : 0.0;
        int seen = 0;
        for (int fr = 0; fr < c.F; fr++) {
            MhFrame m;
            m.depth = c.depth + fr * HW; m.mask = c.mask + fr * HW; m.intensity = c.has_int ? c.fint + fr * HW : nullptr;
            int cls, evals;
            const int took = sf_fuse(c.T + 12 * fr, mh_centre(c.voxel, i), mh_centre(c.voxel, j), mh_centre(c.voxel, k), table.data() + (size_t)fr * c.W * SP_TABLE,
                                     c.R, c.inc, m, c.trunc, &D, &I, &Wt, &cls, &evals);
            seen |= took;
            counts[0] += cls == SP_UNSEEN;
            counts[1] += took;
            counts[2 + evals] += 1;
        }
        o_tsdf[v] = seen ? (float)D : tsdf[v];
        o_w[v] = seen ? (int)Wt : weight[v];
        if (c.has_int) o_int[v] = seen ? (float)I : inten[v];
    }
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: sweepfuse_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = rd<int>(f, 12);
    const std::vector<double> par = rd<double>(f, 8);
    Call c;
    c.X = hd[0]; c.Y = hd[1]; c.Z = hd[2]; c.F = hd[3]; c.H = hd[4]; c.W = hd[5]; c.has_int = hd[7];
    const int n_inc = hd[6], has_twist = hd[8], hostile = hd[9];
    if (c.X < 1 || c.Y < 1 || c.Z < 1 || c.F < 0 || c.H < 1 || c.W < 1 || !(n_inc == 2 || (n_inc == c.H && c.H >= 3))) { fprintf(stderr, "sweepfuse_check: bad header\n"); return 2; }
    const size_t N = (size_t)c.X * c.Y * c.Z, HW = (size_t)c.H * c.W, F = (size_t)c.F;
    const std::vector<double> T = rd<double>(f, 12 * F), inc = rd<double>(f, n_inc);
    const std::vector<double> twist = rd<double>(f, has_twist ? 6 * F : 0), tau = rd<double>(f, has_twist ? c.W : 0);
    const std::vector<float> depth = rd<float>(f, F * HW);
    const std::vector<unsigned char> mask = rd<unsigned char>(f, F * HW);
    const std::vector<float> fint = rd<float>(f, c.has_int ? F * HW : 0);
    const std::vector<float> tsdf = rd<float>(f, N);
    const std::vector<int> weight = rd<int>(f, N);
    const std::vector<float> inten = rd<float>(f, c.has_int ? N : 0);
    fclose(f);
    c.voxel = par[0]; c.trunc = par[1];
    c.R.H = c.H; c.R.W = c.W; c.R.n_inc = n_inc; c.R.wrap = 1; c.R.off = par[2]; c.R.yaw = par[3]; c.R.min_depth = par[4]; c.R.max_depth = par[5];
    c.T = T.data(); c.inc = inc.data(); c.depth = depth.data(); c.mask = mask.data(); c.fint = fint.data();
    std::vector<float> o_tsdf(N), o_int(c.has_int ? N : 0);
    std::vector<int> o_w(N);
    std::vector<long long> counts(2 + SP_MAX_EVAL + 1, 0);
    run(c, make_table(c.F, c.W, has_twist ? twist.data() : nullptr, tau.data()), tsdf.data(), weight.data(), inten.data(), o_tsdf.data(), o_w.data(), o_int.data(),
        counts.data());
    if (hostile && c.F > 0) {
        const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
        std::vector<float> t2(N), i2(c.has_int ? N : 0);
        std::vector<int> w2(N);
        std::vector<long long> n2(counts.size(), 0);
        std::vector<double> tw(6 * F, 0.7), ta(c.W);
        // 1. a NaN twist: every entry of the table is NaN, every u is NaN
        std::vector<double> bad = tw;
        for (size_t k = 0; k < bad.size(); k += 4) bad[k] = nan;
        for (int w = 0; w < c.W; w++) ta[w] = (w + 0.5) / c.W;
        run(c, make_table(c.F, c.W, bad.data(), ta.data()), tsdf.data(), weight.data(), inten.data(), t2.data(), w2.data(), i2.data(), n2.data());
        // 2. infinite and huge column times: infinite, NaN and huge q, columns far outside [0, W) before the range check
        for (int w = 0; w < c.W; w++) ta[w] = w % 3 == 0 ? inf : (w % 3 == 1 ? -1e300 : 1e9 * w);
        run(c, make_table(c.F, c.W, tw.data(), ta.data()), tsdf.data(), weight.data(), inten.data(), t2.data(), w2.data(), i2.data(), n2.data());
        // 3. a huge yaw: u of the order of 1e18 W, whose remainder mod W is not exact
        Call h = c;
        for (const double yaw : {1e18, -1e300, 3e9}) {
            h.R.yaw = yaw;
            run(h, make_table(c.F, c.W, has_twist ? twist.data() : nullptr, tau.data()), tsdf.data(), weight.data(), inten.data(), t2.data(), w2.data(), i2.data(), n2.data());
        }
        // 4. an inclination that is NaN, and one that is not monotonic: the row is a row of the image or the pixel is not read
        std::vector<double> in2 = inc;
        in2[0] = nan;
        h = c; h.inc = in2.data();
        run(h, make_table(c.F, c.W, has_twist ? twist.data() : nullptr, tau.data()), tsdf.data(), weight.data(), inten.data(), t2.data(), w2.data(), i2.data(), n2.data());
        for (size_t k = 0; k < in2.size(); k++) in2[k] = (k % 2 ? 1.0 : -1.0) * 0.3 * (double)(k + 1) / (double)in2.size();
        run(h, make_table(c.F, c.W, has_twist ? twist.data() : nullptr, tau.data()), tsdf.data(), weight.data(), inten.data(), t2.data(), w2.data(), i2.data(), n2.data());
        long long searched = 0;
        for (size_t k = 3; k < n2.size(); k++) searched += n2[k];
        printf("hostile: %lld searches, %lld fused\n", searched, n2[1]);
    }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(o_tsdf.data(), sizeof(float), N, o); fwrite(o_w.data(), sizeof(int), N, o); fwrite(o_int.data(), sizeof(float), o_int.size(), o);
    fwrite(counts.data(), sizeof(long long), counts.size(), o);
    fclose(o);
    printf("SWEEPFUSECHECK ok\n");
    return 0;
}
