/*
 * lrt_adam.h -- C ABI of the fused Adam step over the parameter groups of one Gaussian asset (liblrt_adam.so, a library of its own next to
 * liblrt_hip.so, liblrt_loss.so, liblrt_gridcd.so, liblrt_init.so and liblrt_metrics.so).
 *
 * One call = one kernel launch = one optimizer step of up to LRT_ADAM_MAX_GROUPS tensors that share their first dimension (the Gaussians):
 * xyz (P, 3), f_dc (P, 1, 3), f_rest (P, 15, 3), opacity (P, 1), scaling (P, 2) or (P, 3), rotation (P, 4).  Per element the rule of
 * torch.optim.Adam without weight decay, amsgrad or maximize (lidar_rt_amd/csrc/lrt_adam_math.h holds the text):
 *
 *   m += (1 - beta1) * (g - m)
 *   v  = beta2 * v + (1 - beta2) * g * g
 *   p -= (lr / bias_correction1) * m / (sqrt(v) / bias_correction2_sqrt + eps)
 *
 * Parameter, gradient and both moments are float32 in memory.  The two moment lines are evaluated in double and rounded to float32 ONCE each,
 * which is what torch's fused kernel does (its betas are doubles).  bias_correction1 = 1 - beta1^step and bias_correction2_sqrt =
 * sqrt(1 - beta2^step) are the caller's, computed in float64 for the step this call takes: lr / bias_correction1 is one double division
 * rounded to float32 once, bias_correction2_sqrt is rounded to float32 once, the parameter line then runs in float32.
 *
 * row_mask (NULL: every row): one byte per row.  A row whose byte is 0 keeps its parameter and both moments bit for bit in every group of the
 * call -- nothing of it is loaded or stored; a row whose byte is non-zero gets the full update with the call's bias corrections.  An all-ones
 * mask gives the bits of the call without a mask.  With a mask every group must have mask_rows rows.
 *
 * Conventions: as in lrt_loss.h -- device pointers to contiguous float32 (row_mask: uint8), stream-ordered on `device`; no allocation, no
 * workspace, no host wait and no atomics inside a call, so two calls on equal inputs give equal bits.  0 or a negative code (the LRT_ERR_*
 * values of lrt.h) with lrt_adam_last_error(); the arguments are checked before the device is touched and a refused call launches nothing.
 * Pointers that are all 16-byte aligned take 16-byte loads and stores, any other group the 4-byte path: same values.
 */
#ifndef LRT_ADAM_H_INCLUDED
#define LRT_ADAM_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_ADAM_ABI_VERSION 1
#define LRT_ADAM_MAX_GROUPS 8
#define LRT_ADAM_MAX_WIDTH (1 << 20)

typedef struct {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long rows;                  /* first dimension */
    int width;                       /* floats per row: 3, 3, 45, 1, 2 or 3, 4, ...; 1 .. LRT_ADAM_MAX_WIDTH */
    double lr;
    double bias_correction1;         /* 1 - beta1^step, float64 */
    double bias_correction2_sqrt;    /* sqrt(1 - beta2^step), float64 */
} lrt_adam_group;

int lrt_adam_abi_version(void);

/* Message of the calling thread's last failed lrt_adam_* call. */
const char* lrt_adam_last_error(void);

/* groups: n_groups (1 .. LRT_ADAM_MAX_GROUPS) entries in host memory, read before the call returns. */
int lrt_adam_step(int device, int n_groups, const lrt_adam_group* groups, const unsigned char* row_mask, long long mask_rows,
                  double beta1, double beta2, double eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_ADAM_H_INCLUDED */
