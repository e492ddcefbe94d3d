/*
 * lrt_refine.h -- C ABI of the ray-drop refinement network's inference (liblrt_refine.so, a library of its own next to liblrt_hip.so and the
 * eight operator libraries).
 *
 * The network is lidar_rt_amd/raydrop_refine.py's RaydropUNet (the reference's lib/scene/unet.py): with c = channels and sizes
 * (H_l, W_l) = (H >> l, W >> l), l = 0 .. 4,
 *
 *     x0 = in(x)                                      1x1, Cin -> c, with bias                                  level 0
 *     x_l = pair(maxpool2(x_{l-1}))                   l = 1 .. 4: c -> 2c -> 4c -> 8c -> 8c                      level l
 *     x4 = x4 + proj(attention(bn(x4)))               8 heads over channel chunks, T = H_4 W_4 tokens
 *     y_l = pair(cat[x_l, pad(up2(y_{l+1}))])         l = 3 .. 0: 16c -> 4c, 8c -> 2c, 4c -> c, 2c -> c          level l
 *     logit = out(y_0), prob = sigmoid(logit)         bn, ReLU, 1x1 to one channel with bias
 *
 * pair = (bn, ReLU, 3x3 convolution without bias) twice; the zero padding of a convolution follows bn and ReLU (an out-of-image tap adds 0),
 * the padding of the up path precedes them (a padded pixel holds relu(b)).  maxpool2 floors odd sizes.  up2 is bilinear with aligned corners
 * (source coordinate dst (in - 1) / (out - 1)); the result is placed at offset (diff / 2) of the skip's grid.  The attention's product, laid out
 * (head, token, d), is read back as (token, channel) WITHOUT moving the head axis, as the reference does.  Every bn is the folded affine
 * a x + b of the stored statistics; there is no dropout.
 *
 * params: one float32 array, in this order (K-major weights: row k, column c_out):
 *     in:    w (Cin, c), bias (c)
 *     then the pairs of down1 .. down4, the attention block, the pairs of up1 .. up4, each pair as a1 (Ci), b1 (Ci), w1 (9 Ci, Cm), a2 (Cm),
 *     b2 (Cm), w2 (9 Cm, Co) with k = (3 ky + kx) C + ci; Cm = Co going down, Cm = Ci going up
 *     attention (after down4): a (8c), b (8c), w_qkv (8c, 24c), w_proj (8c, 8c)
 *     out:   a (c), b (c), w (c), bias (1)
 *
 * Kernels: k_rf_in (the input planes, read where the renderer left them, to a channels-last workspace), k_rf_conv<SRC, TAPS, NT, KS> (implicit GEMM
 * pixels x C_out over K = TAPS C_in on the float32-input MFMA 32x32x2: exact float32, one k-ordered fma chain per output, or four over the quarters of K added in a fixed order where a layer has few tiles; the A-operand gather
 * applies the source mapping -- same level, 2x2 maximum of the finer level, or skip | bilinear sample of the coarser level -- then the affine and
 * the ReLU, so that pooled, upsampled, padded and concatenated tensors never exist), k_rf_attn (one wave per query token and head: scores, softmax and value product, the scores in LDS), k_rf_out.
 *
 * Conventions: as in lrt_sweep.h -- device pointers, all work ordered on `stream` of `device`, no allocation and no host wait inside a call,
 * no atomics, every sum in a fixed order (equal inputs give equal bits), every output element written, the inputs unchanged.  What a call
 * reads from the workspace it has written before.  0 or a negative code (the LRT_ERR_* values of lrt.h) with lrt_refine_last_error(); the
 * arguments are checked before the device is touched and a refused call launches nothing.
 */
#ifndef LRT_REFINE_H_INCLUDED
#define LRT_REFINE_H_INCLUDED

#ifdef __cplusplus
extern "C" {
#endif

#define LRT_REFINE_ABI_VERSION 1
#define LRT_REFINE_HEADS 8
#define LRT_REFINE_MAX_TOKENS 2048         /* H_4 W_4: the scores of one query live in LDS */
#define LRT_REFINE_MAX_PIXELS 16777216     /* H W */
#define LRT_REFINE_MAX_CHANNELS 64         /* c; a multiple of 8 */

int lrt_refine_abi_version(void);

/* Message of the calling thread's last failed lrt_refine_* call. */
const char* lrt_refine_last_error(void);

/* Number of floats of `params`; negative for a refused (Cin, channels). */
long long lrt_refine_param_count(int Cin, int channels);

/* Bytes of the workspace for one H x W frame (a multiple of 256).  Negative, with a message, for a refused shape: Cin not 3 or 9, channels not
 * a multiple of 8 in 8 .. LRT_REFINE_MAX_CHANNELS, H or W below 16 (the coarsest level would be empty), H W above LRT_REFINE_MAX_PIXELS, or
 * (H >> 4) (W >> 4) above LRT_REFINE_MAX_TOKENS. */
long long lrt_refine_work_bytes(int H, int W, int Cin, int channels);

/* raydrop, intensity, depth: float32 planes of H x W pixels, pixel (h, w) at element (h W + w) stride_*; ray_o, ray_d: (H, W, 3) float32,
 * required for Cin == 9 and NULL for Cin == 3.  prob (H, W) float32; logits (H, W) float32 or NULL.
 * workspace: 256-byte aligned device memory of work_bytes >= lrt_refine_work_bytes(H, W, Cin, channels). */
int lrt_refine_forward(int device, int H, int W, int Cin, int channels, const float* params, long long n_params,
                       const float* raydrop, const float* intensity, const float* depth, int stride_raydrop, int stride_intensity, int stride_depth,
                       const float* ray_o, const float* ray_d, float* prob, float* logits, void* workspace, long long work_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LRT_REFINE_H_INCLUDED */
