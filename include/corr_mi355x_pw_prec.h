/*
 * corr_mi355x_pw_prec.h — the two pointwise (1x1) convolutions of the update loop that are fused
 * with their neighbours, in a precision mode: the window lookup with convc1 and the mask head
 * with the convex upsampling.  Same library and conventions as corr_mi355x.h (ABI 202: these are
 * additions): fp32 device pointers, 4-byte aligned; every call is enqueued on the caller's
 * `stream`, allocates nothing, does not synchronise, and returns CORR_OK or a negative status with
 * a message in corr_last_error().  Arguments are checked before any HIP call.
 *
 * Each entry point is its counterpart of corr_mi355x.h (corr_lookup_conv,
 * corr_mask_upsample_forward: the arguments, the sizes, the packs and every refusal are described
 * there) with `precision`, a CORR_PREC_* value, before `stream`.  The mode names the pieces of the
 * exact three-piece bf16 split (x = hi + mid + lo) that the kernel keeps of BOTH operands of the
 * 1x1 convolution, and with them the products of one K step, in this order:
 *
 *   CORR_PREC_BF16X6  hi, mid, lo  the six products of the counterpart: bit-identical to it
 *   CORR_PREC_BF16X3  hi, mid      acs += wm xh; acs += wh xm; acc += wh xh   (joined at the end)
 *   CORR_PREC_BF16    hi           acc += wh xh                              (one accumulator)
 *
 * The pieces are the full split's, guards included (an infinite operand is (inf, 0, 0) in every
 * mode, so the non-finite pattern stays fp32's); accumulation is fp32 and the K order is the
 * counterpart's; the packs are the same buffers in every mode.  Only the convolution's products
 * change: corr_lookup_conv_prec's window lookup gives the values of corr_lookup bit for bit in
 * every mode (they are split afterwards), and corr_mask_upsample_forward_prec's bias, scale,
 * softmax and convex combination are fp32 as in the counterpart.  Operand error: 2^-18 relative
 * per operand and the dropped wm xm at 2^-16 (BF16X3), 2^-9 relative per operand (BF16).
 *
 * Forward only: corr_lookup_conv_backward and the training kernels that share the mask head's
 * pack have no modes.
 *
 * An unknown precision is CORR_EINVAL; it is refused before every other check.
 */
#ifndef CORR_MI355X_PW_PREC_H
#define CORR_MI355X_PW_PREC_H

#include <stddef.h>

#include "corr_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int corr_lookup_conv_prec(const float *const *pyr, const float *coords, int B, int H, int W, int levels, int radius,
                          const void *packed_weight, const float *bias, int relu, float *out, int precision,
                          void *stream);
int corr_mask_upsample_forward_prec(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                                    const void *packed, const float *bias, float mask_scale, int B, int H, int W,
                                    float *out, int precision, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CORR_MI355X_PW_PREC_H */
