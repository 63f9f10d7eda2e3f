/*
 * corr_mi355x_enc_prec.h — the encoders' convolutions of libcorr_mi355x.so in a precision mode.
 * Same library and conventions as corr_mi355x.h (ABI 202: these are additions): fp32 device
 * pointers, 4-byte aligned; every call is enqueued on the caller's `stream`, allocates nothing,
 * does not synchronise, and returns CORR_OK or a negative status with a message in
 * corr_last_error().  Arguments are checked before any HIP call.
 *
 * Each entry point is its counterpart of corr_mi355x.h (corr_enc_conv_forward,
 * corr_enc_stem_forward, corr_enc_pw_forward: the arguments, the sizes, the packs, the statistics
 * and every refusal are described there) with `precision`, a CORR_PREC_* value, before `stream`.
 * The mode names the pieces of the exact three-piece bf16 split (x = hi + mid + lo) that the
 * kernel keeps of BOTH operands, and with them the products of one K step, in this order:
 *
 *   CORR_PREC_BF16X6  hi, mid, lo  the six products of the counterpart: bit-identical to it
 *   CORR_PREC_BF16X3  hi, mid      acs += wm xh; acs += wh xm; acc += wh xh   (joined at the end)
 *   CORR_PREC_BF16    hi           acc += wh xh                              (one accumulator)
 *
 * The pieces are the full split's, guards included (an infinite operand is (inf, 0, 0) in every
 * mode, so the non-finite pattern stays fp32's); accumulation is fp32 and the K order is the
 * counterpart's; the packs are the same buffers in every mode.  corr_enc_conv_forward_prec's norm
 * on load (relu(in * in_scale + in_shift), two rounded fp32 operations) is applied before the
 * split, and `stats` holds the statistics of the values this launch stored, in every mode.
 * Operand error: 2^-18 relative per operand and the dropped wm xm at 2^-16 (BF16X3), 2^-9 relative
 * per operand (BF16).
 *
 * An unknown precision is CORR_EINVAL; it is refused before every other check.
 */
#ifndef CORR_MI355X_ENC_PREC_H
#define CORR_MI355X_ENC_PREC_H

#include <stddef.h>

#include "corr_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int corr_enc_conv_forward_prec(const float *in, int cin, int B, int H, int W, int stride, const float *in_scale,
                               const float *in_shift, int norm_per_batch, const void *packed, const float *bias,
                               int cout, float *out, void *stats, size_t stats_bytes, int precision, void *stream);
int corr_enc_stem_forward_prec(const float *in, int cin, int B, int H, int W, const void *packed, const float *bias,
                               int cout, float *out, void *stats, size_t stats_bytes, int precision, void *stream);
int corr_enc_pw_forward_prec(const float *in, int cin, int B, int H, int W, int stride, const void *packed,
                             const float *bias, int cout, float *out, void *stats, size_t stats_bytes, int precision,
                             void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CORR_MI355X_ENC_PREC_H */
