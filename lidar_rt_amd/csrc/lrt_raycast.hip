// lrt_raycast.hip -- ray casting of a TSDF grid (include/lrt_raycast.h), gfx950.  Compiled into liblrt_raycast.so, a library of its own.  No
// allocation, no host wait, no atomic, no LDS; the rule is lrt_raycast_math.h, which the host check compiles as it is.
//
//   k_raycast   one lane per ray, in the rays' memory order (for a range image: consecutive columns of a row).  A wave lasts as long as its
//               longest ray; whether this order or a pixel tile keeps a wave's sample counts closer was NOT measured (no tile order is built; on
//               the bench's room the largest sample count of a cast is about three times the mean).  The grid's scalars are wave-uniform kernel
//               arguments; each lane gathers the eight corners of a cell only when its sample leaves the previous sample's cell.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include "lrt_device_guard.h"
#include "lrt_raycast_math.h"
#include "../../include/lrt_raycast.h"

#define LRT_OK 0
#define LRT_ERR_ARG (-1)
#define LRT_ERR_HIP (-2)

constexpr int NT = LRT_RAYCAST_BLOCK;

__global__ __launch_bounds__(NT) void k_raycast(RcGrid g, RcParams P, long long N, const float* __restrict__ ray_o, const float* __restrict__ ray_d,
                                                float* __restrict__ depth, unsigned char* __restrict__ hit, float* __restrict__ out_intensity,
                                                int* __restrict__ samples)
{
    const long long q = (long long)blockIdx.x * NT + threadIdx.x;
    if (q >= N) return;
    const float ro[3] = {ray_o[3 * q], ray_o[3 * q + 1], ray_o[3 * q + 2]};
    const float rd[3] = {ray_d[3 * q], ray_d[3 * q + 1], ray_d[3 * q + 2]};
    const RcOut r = rc_ray(g, P, ro, rd);
    depth[q] = r.depth;
    hit[q] = r.hit;
    if (out_intensity) out_intensity[q] = r.intensity;
    if (samples) samples[q] = r.samples;
}

// ---- host -----------------------------------------------------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

#define RC_FAIL(code, ...) do { snprintf(g_err, sizeof g_err, __VA_ARGS__); return (code); } while (0)

static bool finite_d(double x) { return x - x == 0.0; }

extern "C" {

int lrt_raycast_abi_version(void) { return LRT_RAYCAST_ABI_VERSION; }

const char* lrt_raycast_last_error(void) { return g_err; }

int lrt_raycast(int device, int X, int Y, int Z, double voxel, double trunc, double origin_x, double origin_y, double origin_z, const float* tsdf,
                const int* weight, const float* intensity, int min_weight, long long N, const float* ray_o, const float* ray_d, double step,
                double far_step, double min_depth, double max_depth, float* depth, unsigned char* hit, float* out_intensity, int* samples,
                void* stream_)
{
    const char* fn = "lrt_raycast";
    if (X < 1 || Y < 1 || Z < 1 || (long long)X * Y * Z > LRT_RAYCAST_MAX_VOXELS)
        RC_FAIL(LRT_ERR_ARG, "%s: a grid of %d x %d x %d voxels (each at least 1, X Y Z at most %lld)", fn, X, Y, Z, LRT_RAYCAST_MAX_VOXELS);
    if (!(voxel > 0.0 && finite_d(voxel)) || !(trunc > 0.0 && finite_d(trunc))) RC_FAIL(LRT_ERR_ARG, "%s: voxel %g, trunc %g (both positive)", fn, voxel, trunc);
    if (!finite_d(origin_x) || !finite_d(origin_y) || !finite_d(origin_z)) RC_FAIL(LRT_ERR_ARG, "%s: origin (%g, %g, %g) (finite)", fn, origin_x, origin_y, origin_z);
    if (min_weight < 1) RC_FAIL(LRT_ERR_ARG, "%s: min_weight %d (at least 1: weight 0 is unobserved)", fn, min_weight);
    if (N < 0 || N > LRT_RAYCAST_MAX_RAYS) RC_FAIL(LRT_ERR_ARG, "%s: %lld rays (0 to %lld)", fn, N, LRT_RAYCAST_MAX_RAYS);
    if (!(step > 0.0 && finite_d(step))) RC_FAIL(LRT_ERR_ARG, "%s: step %g (positive)", fn, step);
    if (!(far_step >= step && far_step < trunc)) RC_FAIL(LRT_ERR_ARG, "%s: far_step %g (step %g <= far_step < trunc %g)", fn, far_step, step, trunc);
    if (!(min_depth >= 0.0 && min_depth < max_depth && finite_d(max_depth))) RC_FAIL(LRT_ERR_ARG, "%s: depths [%g, %g] (0 <= min_depth < max_depth)", fn, min_depth, max_depth);
    if (!(max_depth + step > max_depth)) RC_FAIL(LRT_ERR_ARG, "%s: step %g does not advance t at max_depth %g", fn, step, max_depth);
    const double diag = voxel * sqrt((double)X * X + (double)Y * Y + (double)Z * Z);
    if (!(diag / step <= (double)LRT_RAYCAST_MAX_SAMPLES)) RC_FAIL(LRT_ERR_ARG, "%s: step %g: the grid's diagonal %g m is more than %d steps", fn, step, diag, LRT_RAYCAST_MAX_SAMPLES);
    if (!tsdf || !weight) RC_FAIL(LRT_ERR_ARG, "%s: null tsdf / weight pointer", fn);
    if ((N > 0 && !intensity != !out_intensity) || (!intensity && out_intensity))
        RC_FAIL(LRT_ERR_ARG, "%s: the grid's intensity and the output intensity go together", fn);
    if (N > 0 && (!ray_o || !ray_d || !depth || !hit)) RC_FAIL(LRT_ERR_ARG, "%s: null ray_o / ray_d / depth / hit pointer", fn);
    if (N == 0) return LRT_OK;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev) RC_FAIL(LRT_ERR_ARG, "%s: no HIP device %d (count %d)", fn, device, ndev);
    LrtDeviceGuard guard(device);
    if (!guard.ok) RC_FAIL(LRT_ERR_HIP, "%s: cannot select device %d", fn, device);
    RcGrid g;
    g.X = X; g.Y = Y; g.Z = Z; g.min_weight = min_weight; g.voxel = voxel; g.ox = origin_x; g.oy = origin_y; g.oz = origin_z;
    g.tsdf = tsdf; g.weight = weight; g.intensity = intensity;
    RcParams P;
    P.step = step; P.far_step = far_step; P.min_depth = min_depth; P.max_depth = max_depth;
    hipLaunchKernelGGL(k_raycast, dim3((unsigned)((N + NT - 1) / NT)), dim3(NT), 0, (hipStream_t)stream_, g, P, N, ray_o, ray_d, depth, hit,
                       out_intensity, samples);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) RC_FAIL(LRT_ERR_HIP, "%s: launch failed: %s", fn, hipGetErrorString(e));
    return LRT_OK;
}

}  // extern "C"
