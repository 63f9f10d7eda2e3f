/*
 * corr_mi355x_train_head.h — the training tail of libcorr_mi355x.so with the mask head inside it:
 * the update block's 256 -> 576 1x1 convolution mask[2] and its 0.25 (model/update.py:99-107), the
 * convex upsampling (model/eraft.py:75-86) and the sequence loss (train.py:47-75) in one launch per
 * direction, so the 576-channel mask is neither stored nor saved for backward.  Same library and
 * conventions as corr_mi355x_train.h (ABI 202: these are additions): fp32 device pointers, 4-byte
 * aligned; every call is enqueued on the caller's `stream`, allocates nothing, does not synchronise,
 * and returns CORR_OK or a negative status with a message in corr_last_error().  Every argument is
 * checked before any HIP call.
 *
 * Inputs, as for corr_mask_upsample_forward: hidden [N][hidden_channels][h][w], of which channels
 * hidden_offset .. hidden_offset + 255 are read; flow [N][2][h][w]; `packed` from
 * corr_mask_upsample_pack_weights (16-byte aligned); bias [576]; mask_scale (finite).  The logits,
 * the softmax over the 9 taps and the prediction are computed op for op as
 * corr_mask_upsample_forward does, so a sub-pixel's prediction carries the bits that call stores.
 *
 * The loss of the prediction's last H rows and W columns (H <= 8h, W <= 8w: the pad is at the top
 * and left) against gt [N][2][H][W] and valid [N][H][W], the six fp64 words of `out`, want_metrics
 * and the non-finite rule are exactly those of corr_mi355x_train.h.
 *
 * Backward, with `scale` a DEVICE pointer to one float and G_c = scale v sign(pred_c - gt_c):
 *   dz [N][576][h][w]: the gradient of the convolution's output (bias included, before mask_scale),
 *     dz_k = mask_scale p_k (dv_k - sum_k' p_k' dv_k'), dv_k = G_0 u_k0 + G_1 u_k1; every element
 *     is written, 0 where the crop removes the sub-pixel;
 *   dflow [N][2][h][w].
 * The gradients of the weight, the bias and hidden are the caller's convolution backward over dz.
 * Workspace: 8-byte aligned, of at least corr_mask_upsample_loss_workspace's bytes (it serves both
 * calls), no initialisation needed.  Sizes of 2^31 elements or more (hidden, dz, gt) are refused.
 */
#ifndef CORR_MI355X_TRAIN_HEAD_H
#define CORR_MI355X_TRAIN_HEAD_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t corr_mask_upsample_loss_workspace(int N, int h, int w);
int corr_mask_upsample_loss(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                            const void *packed, const float *bias, float mask_scale, const float *gt,
                            const float *valid, int N, int h, int w, int H, int W, float max_flow, int want_metrics,
                            double *out, void *workspace, size_t workspace_bytes, void *stream);
int corr_mask_upsample_loss_bwd(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                                const void *packed, const float *bias, float mask_scale, const float *gt,
                                const float *valid, const float *scale, int N, int h, int w, int H, int W,
                                float max_flow, float *dflow, float *dz, void *workspace, size_t workspace_bytes,
                                void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CORR_MI355X_TRAIN_HEAD_H */
