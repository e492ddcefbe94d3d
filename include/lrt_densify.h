/*
 * lrt_densify.h -- C ABI of the fused densify-and-prune of one Gaussian asset (liblrt_densify.so, a library of its own next to liblrt_hip.so,
 * liblrt_loss.so, liblrt_gridcd.so, liblrt_init.so, liblrt_metrics.so and liblrt_adam.so).
 *
 * What GaussianAsset.add_densification_stats and GaussianAsset.densify_and_prune (lidar_rt_amd/training.py) do with PyTorch bookkeeping, as
 * one decision per row and ONE stream compaction of the asset:
 *
 *   lrt_densify_stats            one launch per asset and iteration: accum[i] += sqrt(gx^2 + gy^2 + gz^2), denom[i] += (weight[i] > 0).  The norm
 *                                and the sum are formed in double and rounded to float32 once.
 *   lrt_densify_workspace_bytes  the size of the workspace of plan and apply for an asset of P rows.
 *   lrt_densify_plan             two launches: the code of every row and the counts of every block of 256 rows; then the scan of the block
 *                                counts and the totals, written to `totals` (device, LRT_DENSIFY_N_TOTALS x int64):
 *                                P_new, n_clone, n_split, n_scale, n_opa, n_outside, prune_applied, 0.
 *   lrt_densify_apply            one launch: every group and both of its moments move from the old buffers into buffers of P_new rows.
 *
 * The caller reads `totals` between plan and apply (the one host wait of an event: the outputs have to be allocated) and passes P_new on.
 *
 * The rule per row (lidar_rt_amd/csrc/lrt_densify_math.h holds the text): g = accum / denom in float32 (NaN -> 0, +inf -> FLT_MAX);
 * hot = g >= grad_thr; big = max_k expf(scaling_k) > big_thr.  hot & !big is a CLONE (the row stays, an unchanged copy is emitted),
 * hot & big a SPLIT (two children replace the row: xyz + R(q / |q|) (exp(scaling) * split_noise[i, c, :S]), scaling - log 1.6, everything else
 * copied), anything else a KEEP.  Every output is marked for pruning when sigmoid(opacity) < opa_thr, or (size_limit) max_k expf(scaling_k)
 * > huge_thr, or (size_limit and a box) not both samples out_xyz + R (exp(out_scaling) * box_noise[i, slot, s]) lie within the box.  n_opa and
 * n_scale count the marks (overlaps in both).  Marks that would remove EVERY output are not applied (prune_applied = 0).
 *
 * Order of the result: the surviving originals in source order, then the surviving clones, the surviving children 0 and the surviving
 * children 1, each in source order.  A surviving original keeps both moments; a clone or a child gets zero moments.
 *
 * Conventions: as in lrt_adam.h -- device pointers to contiguous float32, stream-ordered on `device`; no allocation, no host wait and no
 * atomics inside a call, so two calls on equal inputs give equal bits.  0 or a negative code (the LRT_ERR_* values of lrt.h) with
 * lrt_densify_last_error(); the arguments are checked before the device is touched and a refused call launches nothing.  P == 0 launches
 * nothing (plan then writes zero totals with one asynchronous memset).
 */
#ifndef LRT_DENSIFY_H_INCLUDED
#define LRT_DENSIFY_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_DENSIFY_ABI_VERSION 1
#define LRT_DENSIFY_MAX_GROUPS 8
#define LRT_DENSIFY_MAX_WIDTH 1024
#define LRT_DENSIFY_MAX_ROWS (1LL << 30)
#define LRT_DENSIFY_N_TOTALS 8
#define LRT_DENSIFY_BLOCK_ROWS 256          /* rows per block of plan and apply */
#define LRT_DENSIFY_SCAN_BLOCKS 1024        /* blocks per pass of the scan: more than SCAN_BLOCKS * BLOCK_ROWS rows take several passes */

#define LRT_DENSIFY_ROLE_COPY 0
#define LRT_DENSIFY_ROLE_XYZ 1              /* children get the split positions */
#define LRT_DENSIFY_ROLE_SCALING 2          /* children get scaling - log 1.6 */

typedef struct {
    const float* src;                /* (P, width) */
    const float* src_exp_avg;        /* both moments or neither (an asset that has not stepped yet) */
    const float* src_exp_avg_sq;
    float* dst;                      /* (P_new, width) */
    float* dst_exp_avg;              /* set exactly when the source moments are */
    float* dst_exp_avg_sq;
    int width;                       /* floats per row, 1 .. LRT_DENSIFY_MAX_WIDTH */
    int role;                        /* LRT_DENSIFY_ROLE_* */
} lrt_densify_group;

typedef struct {
    float grad_thr, big_thr, huge_thr, opa_thr;
    int size_limit;                  /* 0: only the opacity test prunes */
    int has_box;                     /* with size_limit: the box test, box_noise required */
    float box_min[3], box_max[3];
} lrt_densify_rule;

int lrt_densify_abi_version(void);

/* Message of the calling thread's last failed lrt_densify_* call. */
const char* lrt_densify_last_error(void);

/* mean_grads (P, 3), weights (P), accum (P), denom (P). */
int lrt_densify_stats(int device, long long P, const float* mean_grads, const float* weights, float* accum, float* denom, void* stream);

/* Bytes of the workspace for P rows (a multiple of 256, at least 256); negative for a P outside 0 .. LRT_DENSIFY_MAX_ROWS. */
long long lrt_densify_workspace_bytes(long long P);

/* S: 2 or 3 floats per scaling row.  split_noise (P, 2, 3); box_noise (P, 2, 2, 3), read with rule->size_limit and rule->has_box only.
 * workspace: 256-byte aligned device memory of workspace_bytes >= lrt_densify_workspace_bytes(P); totals: device, 8 x int64. */
int lrt_densify_plan(int device, long long P, int S, const float* xyz, const float* scaling, const float* rotation, const float* opacity,
                     const float* accum, const float* denom, const float* split_noise, const float* box_noise, const lrt_densify_rule* rule,
                     void* workspace, long long workspace_bytes, long long* totals, void* stream);

/* After lrt_densify_plan on the same P, inputs and workspace.  P_new: totals[0] as the caller read it; no row at or beyond it is written.
 * groups: n_groups (1 .. LRT_DENSIFY_MAX_GROUPS) entries in host memory, read before the call returns; exactly one has the role XYZ and one
 * the role SCALING (their sources are xyz and scaling of the plan; widths 3 and S). */
int lrt_densify_apply(int device, long long P, long long P_new, int S, const float* rotation, const float* split_noise, int n_groups,
                      const lrt_densify_group* groups, const void* workspace, long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_DENSIFY_H_INCLUDED */
