// place_check.cpp -- lrt_place_math.h compiled for the host (g++ -ffp-contract=off): the rules' text evaluated on frames read from a file.
//
//   in : int32 F, H, W, NR, NS, gap, 0, 0; float64 up[3], r_min, r_max, z_lo, z_step, 0; float32 points[F H W 3]; uint8 mask[F H W]
//   out: uint8 desc[F NS NRP]; int32 sum[F]; int32 best_d[F F]; int32 best_s[F F]
//
// Prints "PLACECHECK ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../lidar_rt_amd/csrc/lrt_place_math.h"

template <class T> static std::vector<T> rd(FILE* f, size_t n)
{
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "place_check: short input\n"); exit(2); }
    return v;
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: place_check in out\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int> hd = rd<int>(f, 8);
    const std::vector<double> par = rd<double>(f, 8);
    const int F = hd[0], H = hd[1], W = hd[2], NR = hd[3], NS = hd[4], gap = hd[5];
    if (F < 1 || H < 1 || W < 1 || NR < 1 || NR > PL_MAX_RINGS || NS < 1 || NS > PL_MAX_SECTORS || NS > W || gap < 0) { fprintf(stderr, "place_check: bad header\n"); return 2; }
    const size_t HW = (size_t)H * W;
    const std::vector<float> p = rd<float>(f, 3 * HW * F);
    const std::vector<unsigned char> m = rd<unsigned char>(f, HW * F);
    fclose(f);
    PlRule R;
    R.NR = NR; R.NS = NS; R.up[0] = par[0]; R.up[1] = par[1]; R.up[2] = par[2]; R.r_min = par[3]; R.r_max = par[4]; R.z_lo = par[5]; R.z_step = par[6];
    const int NRP = pl_padded(NR), NRW = NRP / 4;
    std::vector<unsigned char> desc((size_t)F * NS * NRP, 0);
    std::vector<int> sum(F, 0), best_d((size_t)F * F, -1), best_s((size_t)F * F, -1);
    for (int fr = 0; fr < F; fr++) {
        unsigned char* d = desc.data() + (size_t)fr * NS * NRP;
        for (size_t i = 0; i < HW; i++) {
            const size_t g = (size_t)fr * HW + i;
            int ring, value;
            if (!m[g] || !pl_cell(p.data() + 3 * g, R, &ring, &value)) continue;
            unsigned char* cell = d + (size_t)pl_sector((int)(i % W), NS, W) * NRP + ring;
            if (value > *cell) *cell = (unsigned char)value;
        }
        for (int k = 0; k < NS * NRP; k++) sum[fr] += d[k];
    }
    std::vector<unsigned> words((size_t)F * NS * NRW);
    memcpy(words.data(), desc.data(), desc.size());
    for (int i = 0; i < F; i++)
        for (int j = 0; j + gap <= i; j++) {
            int best = PL_NO_KEY;
            for (int s = 0; s < NS; s++) {
                unsigned acc = 0;
                for (int c = 0; c < NS; c++)
                    for (int k = 0; k < NRW; k++)
                        acc = pl_sad4(words[((size_t)i * NS + (c + s) % NS) * NRW + k], words[((size_t)j * NS + c) * NRW + k], acc);
                const int key = pl_key(acc, s);
                if (key < best) best = key;
            }
            best_d[(size_t)i * F + j] = best >> PL_SHIFT_BITS;
            best_s[(size_t)i * F + j] = best & ((1 << PL_SHIFT_BITS) - 1);
        }
    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    fwrite(desc.data(), 1, desc.size(), o); fwrite(sum.data(), sizeof(int), F, o);
    fwrite(best_d.data(), sizeof(int), best_d.size(), o); fwrite(best_s.data(), sizeof(int), best_s.size(), o);
    fclose(o);
    printf("PLACECHECK ok\n");
    return 0;
}
