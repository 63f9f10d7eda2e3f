/*
 * corr_mi355x_train.h — the training tail of libcorr_mi355x.so: the reference's sequence_loss
 * (train.py:47-75), alone over a stored prediction and fused with the convex upsampling
 * (model/eraft.py:75-86).  Same library and conventions as corr_mi355x.h (ABI 202: these are
 * additions): fp32 device pointers, 4-byte aligned; every call is enqueued on the caller's
 * `stream`, allocates nothing, does not synchronise, and returns CORR_OK or a negative status
 * with a message in corr_last_error().  Arguments are checked before any HIP call.
 *
 * The loss of one prediction pred [N][2][H][W] against gt [N][2][H][W] and valid [N][H][W]:
 *   v = (valid >= 0.5) && (sqrt(gt_x^2 + gt_y^2) < max_flow), as 0.f / 1.f, multiplied into
 *   |pred - gt| (so a non-finite prediction or ground truth poisons the sum exactly where the
 *   reference's does, masked pixel or not).
 * out: six fp64 words on the device, 8-byte aligned, all written:
 *   0  sum v (|d_x| + |d_y|)      (the reference's term is this / (N 2 H W), times gamma^(n-1-i))
 *   1  n_valid
 *   2  sum over valid pixels of epe = sqrt(d_x^2 + d_y^2)
 *   3, 4, 5  the number of valid pixels with epe < 1, < 3, < 5
 * Words 2..5 are computed only with want_metrics != 0 (the last prediction) and are 0 otherwise.
 * A thread sums at most 16 terms in fp32; everything above is fp64 in a fixed order and the
 * counts are integers: two runs agree bit for bit.
 *
 * Backward: G = scale v sign(pred - gt) with sign(0) = 0, where `scale` is a DEVICE pointer to
 * one float (upstream gradient * gamma^(n-1-i) / (N 2 H W), made on the device: no host sync).
 *
 * Fused with the upsampling: flow [N][2][h][w] and mask [N][576][h][w] as for
 * corr_convex_upsample; the prediction is its output (bit for bit) cropped to the last H rows and
 * W columns of the 8h x 8w frame (the pad 8h - H >= 0, 8w - W >= 0 is at the top and left), and is
 * never stored.  corr_upsample_loss_bwd writes dflow [N][2][h][w] and every element of dmask
 * [N][576][h][w] (0 where the crop removes the sub-pixel); it reads no grad_out.
 * Workspaces: 8-byte aligned, of at least the size function's bytes, no initialisation needed;
 * corr_upsample_loss_workspace serves both fused calls.
 */
#ifndef CORR_MI355X_TRAIN_H
#define CORR_MI355X_TRAIN_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

size_t corr_upsample_loss_workspace(int N, int h, int w);
int corr_upsample_loss(const float *flow, const float *mask, const float *gt, const float *valid, int N, int h,
                       int w, int H, int W, float max_flow, int want_metrics, double *out, void *workspace,
                       size_t workspace_bytes, void *stream);
int corr_upsample_loss_bwd(const float *flow, const float *mask, const float *gt, const float *valid,
                           const float *scale, int N, int h, int w, int H, int W, float max_flow, float *dflow,
                           float *dmask, void *workspace, size_t workspace_bytes, void *stream);

size_t corr_sequence_loss_workspace(int N, int H, int W);
int corr_sequence_loss(const float *pred, const float *gt, const float *valid, int N, int H, int W, float max_flow,
                       int want_metrics, double *out, void *workspace, size_t workspace_bytes, void *stream);
/* dpred [N][2][H][W], every element written; no workspace. */
int corr_sequence_loss_bwd(const float *pred, const float *gt, const float *valid, const float *scale, int N, int H,
                           int W, float max_flow, float *dpred, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CORR_MI355X_TRAIN_H */
