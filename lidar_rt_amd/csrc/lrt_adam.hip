// lrt_adam.hip -- the fused Adam step over the parameter groups of one Gaussian asset (include/lrt_adam.h), gfx950.  Compiled into liblrt_adam.so,
// a library of its own.
//
// One launch, no workspace, no atomics:
//   k_adam_step   a workgroup of 256 threads owns 256 consecutive rows (Gaussians).  It reads their mask bytes into LDS once (no mask: all
//                 ones) and then, group after group, walks the contiguous 256 * width floats of those rows in the group's four tensors: sixteen
//                 bytes per lane where all four pointers are 16-byte aligned (a block's start, 256 * width * 4 bytes, always is), four bytes per
//                 lane otherwise.  A 16-byte vector may span rows (width 3: always); each component obeys its own row's flag.  A vector whose four
//                 flags are set is one load per tensor and one store per written tensor; one with some flags set goes component by component;
//                 one with none issues nothing -- the rows a sweep did not touch cost the mask byte and no other traffic.
//                 The group table travels by value in the kernel arguments.  The arithmetic is lrt_adam_math.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_adam_math.h"
#include "../../include/lrt_adam.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = 256;                        // threads = rows per workgroup

struct AdGroup {
    float* p; const float* g; float* m; float* v;
    long long rows;
    int width;
    LrtAdamStep<float> step;
};

struct AdArgs {
    AdGroup grp[LRT_ADAM_MAX_GROUPS];
    const unsigned char* mask;                 // nullptr: every row
    long long mask_rows;
    LrtAdamRule rule;
    int n_groups;
};

__global__ __launch_bounds__(NT) void k_adam_step(AdArgs a)
{
    __shared__ unsigned char s_on[NT + 4];     // the flag of row row0 + i; four zeros behind it: the row index one past a short block's last element
    const int tid = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * NT;
    s_on[tid] = a.mask ? (unsigned char)(row0 + tid < a.mask_rows && a.mask[row0 + tid] != 0) : (unsigned char)1;
    if (tid < 4) s_on[NT + tid] = 0;
    __syncthreads();
#pragma unroll 1
    for (int gi = 0; gi < a.n_groups; gi++) {
        const AdGroup& G = a.grp[gi];
        const long long left = G.rows - row0;
        if (left <= 0) continue;
        const unsigned w = (unsigned)G.width;
        const int nel = (left < NT ? (int)left : NT) * G.width;        // floats of this block: at most 256 * LRT_ADAM_MAX_WIDTH = 2^28
        const size_t base = (size_t)row0 * w;
        float* __restrict__ p = G.p + base;
        const float* __restrict__ g = G.g + base;
        float* __restrict__ m = G.m + base;
        float* __restrict__ v = G.v + base;
        const LrtAdamStep<float> st = G.step;
        const bool aligned = ((((uintptr_t)G.p) | ((uintptr_t)G.g) | ((uintptr_t)G.m) | ((uintptr_t)G.v)) & 15) == 0;
        if (aligned) {
            const int nv = (nel + 3) >> 2;
            for (int i = tid; i < nv; i += NT) {
                const int e = 4 * i;
                unsigned r = (unsigned)e / w, rem = (unsigned)e - r * w;
                bool on[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    on[k] = e + k < nel && s_on[r] != 0;               // r <= 256 + 3 / w here: inside s_on
                    if (++rem == w) { rem = 0; r++; }
                }
                if (on[0] && on[1] && on[2] && on[3]) {
                    float4 P = *reinterpret_cast<const float4*>(p + e);
                    const float4 Gr = *reinterpret_cast<const float4*>(g + e);
                    float4 M = *reinterpret_cast<const float4*>(m + e);
                    float4 V = *reinterpret_cast<const float4*>(v + e);
                    lrt_adam_update(P.x, Gr.x, M.x, V.x, a.rule, st);
                    lrt_adam_update(P.y, Gr.y, M.y, V.y, a.rule, st);
                    lrt_adam_update(P.z, Gr.z, M.z, V.z, a.rule, st);
                    lrt_adam_update(P.w, Gr.w, M.w, V.w, a.rule, st);
                    *reinterpret_cast<float4*>(p + e) = P;
                    *reinterpret_cast<float4*>(m + e) = M;
                    *reinterpret_cast<float4*>(v + e) = V;
                } else {
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        if (!on[k]) continue;                          // on[k] implies e + k < nel
                        float P = p[e + k], M = m[e + k], V = v[e + k];
                        lrt_adam_update(P, g[e + k], M, V, a.rule, st);
                        p[e + k] = P; m[e + k] = M; v[e + k] = V;
                    }
                }
            }
        } else {
            for (int e = tid; e < nel; e += NT) {
                if (s_on[(unsigned)e / w] == 0) continue;
                float P = p[e], M = m[e], V = v[e];
                lrt_adam_update(P, g[e], M, V, a.rule, st);
                p[e] = P; m[e] = M; v[e] = V;
            }
        }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define AD_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

extern "C" {

int lrt_adam_abi_version(void) { return LRT_ADAM_ABI_VERSION; }

const char* lrt_adam_last_error(void) { return g_err; }

int lrt_adam_step(int device, int n_groups, const lrt_adam_group* groups, const unsigned char* row_mask, long long mask_rows,
                  double beta1, double beta2, double eps, void* stream_)
{
    const char* fn = "lrt_adam_step";
    // the arguments first, the device after them: a bad call is refused on a machine without one, too
    if (n_groups < 1 || n_groups > LRT_ADAM_MAX_GROUPS) AD_FAIL(LRT_ERR_ARG, "%s: %d groups (1 .. %d in one call)", fn, n_groups, LRT_ADAM_MAX_GROUPS);
    if (!groups) AD_FAIL(LRT_ERR_ARG, "%s: null group table", fn);
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0) || !(eps >= 0.0)) AD_FAIL(LRT_ERR_ARG, "%s: beta1 = %g, beta2 = %g (0 <= beta < 1), eps = %g (>= 0)", fn, beta1, beta2, eps);
    if (row_mask && mask_rows < 0) AD_FAIL(LRT_ERR_ARG, "%s: a mask of %lld rows", fn, mask_rows);
    AdArgs a;
    long long max_rows = 0;
    for (int i = 0; i < n_groups; i++) {
        const lrt_adam_group& s = groups[i];
        if (!s.param || !s.grad || !s.exp_avg || !s.exp_avg_sq) AD_FAIL(LRT_ERR_ARG, "%s: group %d: null parameter / gradient / moment pointer", fn, i);
        if (s.width < 1 || s.width > LRT_ADAM_MAX_WIDTH) AD_FAIL(LRT_ERR_ARG, "%s: group %d: width %d (1 .. %d floats per row)", fn, i, s.width, LRT_ADAM_MAX_WIDTH);
        if (s.rows < 0 || s.rows > ((long long)INT32_MAX - 1) * NT) AD_FAIL(LRT_ERR_ARG, "%s: group %d: %lld rows", fn, i, s.rows);
        if (row_mask && s.rows != mask_rows) AD_FAIL(LRT_ERR_ARG, "%s: group %d has %lld rows, the row mask %lld", fn, i, s.rows, mask_rows);
        if (!(s.lr == s.lr) || !(s.bias_correction1 > 0.0) || !(s.bias_correction2_sqrt > 0.0))
            AD_FAIL(LRT_ERR_ARG, "%s: group %d: lr = %g, bias_correction1 = %g, bias_correction2_sqrt = %g (corrections > 0)", fn, i, s.lr, s.bias_correction1, s.bias_correction2_sqrt);
        AdGroup& d = a.grp[i];
        d.p = s.param; d.g = s.grad; d.m = s.exp_avg; d.v = s.exp_avg_sq; d.rows = s.rows; d.width = s.width;
        d.step = lrt_adam_step_of<float>(s.lr, s.bias_correction1, s.bias_correction2_sqrt);
        if (s.rows > max_rows) max_rows = s.rows;
    }
    for (int i = n_groups; i < LRT_ADAM_MAX_GROUPS; i++) { AdGroup& d = a.grp[i]; d.p = nullptr; d.g = nullptr; d.m = nullptr; d.v = nullptr; d.rows = 0; d.width = 1; d.step.step_size = 0.f; d.step.bc2_sqrt = 1.f; }
    a.mask = row_mask; a.mask_rows = row_mask ? mask_rows : 0; a.rule = lrt_adam_rule(beta1, beta2, eps); a.n_groups = n_groups;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) AD_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    if (max_rows == 0) return LRT_OK;                                   // nothing to step: nothing to launch
    LrtDeviceGuard guard(device);
    if (!guard.ok) AD_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    const unsigned nblk = (unsigned)((max_rows + NT - 1) / NT);
    hipLaunchKernelGGL(k_adam_step, dim3(nblk), dim3(NT), 0, (hipStream_t)stream_, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) AD_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
