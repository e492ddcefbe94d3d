// lrt_place.hip -- the place matcher (include/lrt_place.h), gfx950.  Compiled into liblrt_place.so, a library of its own.  No allocation, no host
// wait, no float atomic; the rules are lrt_place_math.h.
//
//   k_place_describe   one workgroup per frame.  The cells of the frame are 32-bit words in LDS (NR * NS <= 4096 of them); the lanes walk the
//                      frame's pixels, consecutive lanes on consecutive columns, and raise a cell with an integer atomicMax in LDS.  After the
//                      barrier the words are packed to bytes, one dword of four rings per lane and store, and the bytes are summed with an integer
//                      atomicAdd in LDS.  Nothing is accumulated in global memory: there is no fill launch and no workspace.
//   k_place_match      one workgroup per (query i, tile of 16 candidates).  The query's descriptor sits in LDS twice in a row, so sector c + s
//                      needs no modulo; the sector stride is NRP / 4 dwords made odd, so that the 32 lanes of a ds_read_b32 group, on consecutive
//                      sectors, fall on 32 different banks (a stride of 8 dwords would put them on 4).  A wave takes four candidates side by side
//                      and a lane takes a shift: one LDS read of the query's dword serves four v_sad_u8 against the four candidates' dwords,
//                      which are wave-uniform (scalar loads).  NS > 64 is a second pass of the wave over the shifts.  The key D << 7 | s goes
//                      through one butterfly of integer min.  A tile outside the triangle writes its -1 and returns before it loads anything.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_place_math.h"
#include "../../include/lrt_place.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_PLACE_BLOCK;
constexpr int ND = LRT_PLACE_DESCRIBE_BLOCK;
constexpr int TILE = LRT_PLACE_TILE;
constexpr int CPW = TILE / (NT / 64);                                 // candidates per wave
constexpr int MAX_CELLS = LRT_PLACE_MAX_RINGS * LRT_PLACE_MAX_SECTORS;
constexpr int MAX_STRIDE = LRT_PLACE_MAX_RINGS / 4 + 1;               // dwords per sector in LDS, made odd

static_assert(NT == 256 && CPW == 4, "k_place_match is written for four waves of four candidates");
static_assert(LRT_PLACE_MAX_RINGS == PL_MAX_RINGS && LRT_PLACE_MAX_SECTORS == PL_MAX_SECTORS, "the header and the rule disagree");
static_assert(LRT_PLACE_MAX_SECTORS <= (1 << PL_SHIFT_BITS), "a shift must fit the key's low bits");
static_assert(255LL * MAX_CELLS < (1LL << (31 - PL_SHIFT_BITS)), "D << 7 | s must fit a positive int");

// ---- describe -----------------------------------------------------------------------------------------------------------------------------------------
struct DescribeArgs {
    int H, W, HW;
    const float* points;
    const unsigned char* mask;
    PlRule rule;
    unsigned* desc;                                                   // (F, NS, NRP / 4) dwords
    int* sum;
};

__global__ __launch_bounds__(ND) void k_place_describe(DescribeArgs a)
{
    __shared__ int cells[MAX_CELLS];
    __shared__ int total;
    const int NR = a.rule.NR, NS = a.rule.NS, NRW = pl_padded(NR) / 4;
    const int n_cells = NR * NS;
    for (int c = threadIdx.x; c < n_cells; c += ND) cells[c] = 0;
    if (threadIdx.x == 0) total = 0;
    __syncthreads();
    const long long base = (long long)blockIdx.x * a.HW;
    for (int i = threadIdx.x; i < a.HW; i += ND) {
        if (!a.mask[base + i]) continue;
        const float p[3] = {a.points[3 * (base + i)], a.points[3 * (base + i) + 1], a.points[3 * (base + i) + 2]};
        int ring, value;
        if (!pl_cell(p, a.rule, &ring, &value)) continue;
        const int w = i % a.W;
        atomicMax(&cells[pl_sector(w, NS, a.W) * NR + ring], value);
    }
    __syncthreads();
    int part = 0;
    unsigned* out = a.desc + (long long)blockIdx.x * NS * NRW;
    for (int d = threadIdx.x; d < NS * NRW; d += ND) {
        const int c = d / NRW, r0 = 4 * (d - c * NRW);
        unsigned word = 0;
        for (int k = 0; k < 4; k++) {
            const int v = r0 + k < NR ? cells[c * NR + r0 + k] : 0;
            word |= (unsigned)v << (8 * k);
            part += v;
        }
        out[d] = word;
    }
    if (part) atomicAdd(&total, part);                                // an integer sum: the order cannot show
    __syncthreads();
    if (threadIdx.x == 0) a.sum[blockIdx.x] = total;
}

// ---- match --------------------------------------------------------------------------------------------------------------------------------------------
struct MatchArgs {
    int F, NS, NRW;
    long long gap;
};

// desc is a parameter of its own, const and restrict: the candidates' dwords are then loads the compiler may issue as scalar ones
__global__ __launch_bounds__(NT) void k_place_match(MatchArgs a, const unsigned* __restrict__ desc, int* __restrict__ best_d, int* __restrict__ best_s)
{
    __shared__ unsigned q[2 * LRT_PLACE_MAX_SECTORS * MAX_STRIDE];
    const int i = blockIdx.y, j0 = blockIdx.x * TILE;
    const int NS = a.NS, NRW = a.NRW, stride = NRW | 1;
    const long long row = (long long)i * a.F;
    if (j0 + a.gap > i) {                                             // the whole tile lies outside the triangle (uniform: before any barrier)
        if (threadIdx.x < TILE && j0 + (int)threadIdx.x < a.F) {
            best_d[row + j0 + threadIdx.x] = -1;
            best_s[row + j0 + threadIdx.x] = -1;
        }
        return;
    }
    const int words = NS * NRW;
    const unsigned* mine = desc + (long long)i * words;
    for (int idx = threadIdx.x; idx < 2 * words; idx += NT) {
        const int c2 = idx / NRW, k = idx - c2 * NRW;
        const int c = c2 >= NS ? c2 - NS : c2;
        q[c2 * stride + k] = mine[c * NRW + k];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int j[CPW];
    bool ok[CPW];
    const unsigned* cand[CPW];
    int best[CPW];
#pragma unroll
    for (int m = 0; m < CPW; m++) {
        j[m] = j0 + wave * CPW + m;
        ok[m] = j[m] < a.F && j[m] + a.gap <= i;
        cand[m] = desc + (long long)(ok[m] ? j[m] : i) * words;    // a candidate that does not count reads the query's own row: in bounds
        best[m] = PL_NO_KEY;
    }
    if (!ok[0]) {                                                     // candidates ascend: none of this wave's counts (wave-uniform, after the barrier)
        if (lane < CPW && j0 + wave * CPW + lane < a.F) {
            best_d[row + j0 + wave * CPW + lane] = -1;
            best_s[row + j0 + wave * CPW + lane] = -1;
        }
        return;
    }
    for (int s0 = 0; s0 < NS; s0 += 64) {
        const int s = s0 + lane;
        const int sa = s < NS ? s : NS - 1;                           // a lane without a shift reads in bounds and gives no key
        unsigned acc[CPW];
#pragma unroll
        for (int m = 0; m < CPW; m++) acc[m] = 0;
        const unsigned* qs = q + sa * stride;
        for (int c = 0; c < NS; c++) {
            for (int k = 0; k < NRW; k++) {
                const unsigned mine_w = qs[c * stride + k];
#pragma unroll
                for (int m = 0; m < CPW; m++) acc[m] = pl_sad4(mine_w, cand[m][c * NRW + k], acc[m]);
            }
        }
#pragma unroll
        for (int m = 0; m < CPW; m++) {
            const int key = s < NS ? pl_key(acc[m], s) : PL_NO_KEY;
            best[m] = key < best[m] ? key : best[m];
        }
    }
#pragma unroll
    for (int m = 0; m < CPW; m++) {
        int v = best[m];
        for (int off = 32; off > 0; off >>= 1) {
            const int o = __shfl_xor(v, off, 64);
            v = o < v ? o : v;
        }
        if (lane == 0 && j[m] < a.F) {
            best_d[row + j[m]] = ok[m] ? v >> PL_SHIFT_BITS : -1;
            best_s[row + j[m]] = ok[m] ? v & ((1 << PL_SHIFT_BITS) - 1) : -1;
        }
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define PL_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)
#define PL_LAUNCHED(what) do { hipError_t e_ = hipGetLastError(); \
    if (e_ != hipSuccess) PL_FAIL(LRT_ERR_HIP, "%s: launch of %s failed: %s", fn, what, hipGetErrorString(e_)); } while (0)

static bool finite_d(double x) { return x - x == 0.0; }

static int check_grid(const char* fn, int NR, int NS)
{
    if (NR < 1 || NR > LRT_PLACE_MAX_RINGS || NS < 1 || NS > LRT_PLACE_MAX_SECTORS)
        PL_FAIL(LRT_ERR_ARG, "%s: a descriptor of %d rings x %d sectors (1 to %d rings, 1 to %d sectors)", fn, NR, NS, LRT_PLACE_MAX_RINGS, LRT_PLACE_MAX_SECTORS);
    return LRT_OK;
}

static int select_device(const char* fn, int device)
{
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) PL_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    return LRT_OK;
}

extern "C" {

int lrt_place_abi_version(void) { return LRT_PLACE_ABI_VERSION; }

const char* lrt_place_last_error(void) { return g_err; }

int lrt_place_describe(int device, long long F, int H, int W, const float* points, const unsigned char* mask, int NR, int NS, double up_x,
                       double up_y, double up_z, double r_min, double r_max, double z_lo, double z_step, unsigned char* desc, int* sum,
                       void* stream_)
{
    const char* fn = "lrt_place_describe";
    int rc;
    if (F < 1 || H < 1 || W < 1 || F > LRT_PLACE_MAX_FRAMES || (long long)H * W > LRT_PLACE_MAX_PIXELS || F > LRT_PLACE_MAX_PIXELS / ((long long)H * W))
        PL_FAIL(LRT_ERR_ARG, "%s: %lld frames of %d x %d pixels (each at least 1, at most %d frames, F H W at most %lld)", fn, F, H, W, LRT_PLACE_MAX_FRAMES,
                LRT_PLACE_MAX_PIXELS);
    if ((rc = check_grid(fn, NR, NS)) != LRT_OK) return rc;
    if (NS > W) PL_FAIL(LRT_ERR_ARG, "%s: %d sectors over %d columns (a sector is at least one column)", fn, NS, W);
    if (!points || !mask) PL_FAIL(LRT_ERR_ARG, "%s: null points / mask pointer", fn);
    if (!desc || !sum) PL_FAIL(LRT_ERR_ARG, "%s: null desc / sum pointer", fn);
    if ((uintptr_t)desc & 3) PL_FAIL(LRT_ERR_ARG, "%s: desc must be 4-byte aligned", fn);
    const double n2 = up_x * up_x + up_y * up_y + up_z * up_z;
    if (!(n2 > 1.0 - 1e-6 && n2 < 1.0 + 1e-6)) PL_FAIL(LRT_ERR_ARG, "%s: up (%g, %g, %g) is not a unit vector", fn, up_x, up_y, up_z);
    if (!(r_min >= 0.0 && r_min < r_max && finite_d(r_max))) PL_FAIL(LRT_ERR_ARG, "%s: the ground range [%g, %g) (0 <= r_min < r_max)", fn, r_min, r_max);
    if (!finite_d(z_lo)) PL_FAIL(LRT_ERR_ARG, "%s: z_lo %g", fn, z_lo);
    if (!(z_step > 0.0 && finite_d(z_step))) PL_FAIL(LRT_ERR_ARG, "%s: z_step %g (positive)", fn, z_step);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) PL_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    DescribeArgs a;
    a.H = H; a.W = W; a.HW = H * W; a.points = points; a.mask = mask;
    a.rule.NR = NR; a.rule.NS = NS; a.rule.up[0] = up_x; a.rule.up[1] = up_y; a.rule.up[2] = up_z;
    a.rule.r_min = r_min; a.rule.r_max = r_max; a.rule.z_lo = z_lo; a.rule.z_step = z_step;
    a.desc = (unsigned*)desc; a.sum = sum;
    hipLaunchKernelGGL(k_place_describe, dim3((unsigned)F), dim3(ND), 0, (hipStream_t)stream_, a);
    PL_LAUNCHED("the descriptors");
    return LRT_OK;
}

int lrt_place_match(int device, long long F, int NR, int NS, const unsigned char* desc, long long gap, int* best_d, int* best_s, void* stream_)
{
    const char* fn = "lrt_place_match";
    int rc;
    if (F < 1 || F > LRT_PLACE_MAX_FRAMES) PL_FAIL(LRT_ERR_ARG, "%s: %lld frames (1 to %d)", fn, F, LRT_PLACE_MAX_FRAMES);
    if ((rc = check_grid(fn, NR, NS)) != LRT_OK) return rc;
    if (gap < 0) PL_FAIL(LRT_ERR_ARG, "%s: a gap of %lld frames (not negative)", fn, gap);
    if (!desc) PL_FAIL(LRT_ERR_ARG, "%s: null desc pointer", fn);
    if ((uintptr_t)desc & 3) PL_FAIL(LRT_ERR_ARG, "%s: desc must be 4-byte aligned", fn);
    if (!best_d || !best_s) PL_FAIL(LRT_ERR_ARG, "%s: null best_d / best_s pointer", fn);
    if ((rc = select_device(fn, device)) != LRT_OK) return rc;
    LrtDeviceGuard guard(device);
    if (!guard.ok) PL_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    MatchArgs a;
    a.F = (int)F; a.NS = NS; a.NRW = pl_padded(NR) / 4; a.gap = gap;
    hipLaunchKernelGGL(k_place_match, dim3((unsigned)((F + TILE - 1) / TILE), (unsigned)F), dim3(NT), 0, (hipStream_t)stream_, a, (const unsigned*)desc, best_d, best_s);
    PL_LAUNCHED("the matcher");
    return LRT_OK;
}

}  // extern "C"
