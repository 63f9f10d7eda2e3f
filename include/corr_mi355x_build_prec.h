/*
 * corr_mi355x_build_prec.h — the all-pairs correlation build of libcorr_mi355x.so in a precision
 * mode.  Same library and conventions as corr_mi355x.h (ABI 202: these are additions): fp32 device
 * pointers, 4-byte aligned; every call is enqueued on the caller's `stream`, allocates nothing,
 * does not synchronise, and returns CORR_OK or a negative status with a message in
 * corr_last_error().  Arguments are checked before any HIP call.
 *
 * Each entry point is its counterpart of corr_mi355x.h (corr_build_ex, corr_build_region: the
 * arguments, the tiled pyramid, the workspace of corr_build_workspace and every refusal are
 * described there) with `precision`, a CORR_PREC_* value, before `stream`.  The mode names the
 * pieces of the exact three-piece bf16 split (x = hi + mid + lo) that the build keeps of BOTH
 * feature maps, and with them the products of one 32-deep K step, in this order (t = target,
 * q = query):
 *
 *   CORR_PREC_BF16X6  hi, mid, lo  the six products of the counterpart: bit-identical to it
 *   CORR_PREC_BF16X3  hi, mid      acs += mid_t hi_q; acs += hi_t mid_q; acc += hi_t hi_q
 *                                  (the two accumulators joined at the end, as the counterpart's)
 *   CORR_PREC_BF16    hi           acc += hi_t hi_q                       (one accumulator)
 *
 * The pieces are the full split's, guards included (an infinite feature is (inf, 0, 0) in every
 * mode, so the non-finite pattern stays the counterpart's); accumulation is fp32, the K order,
 * the 1/sqrt(D) scale and the pyramid (levels 1.. are avg_pool2d of the launch's own level 0, bit
 * for bit) are the counterpart's.  Error against the exact product, relative to
 * sum_k |f1_k| |f2_k| / sqrt(D): at most 2^-16 (BF16X3: the dropped lo pieces and mid x mid) and
 * 2^-8 + 2^-18 (BF16: each operand to 2^-9), plus the fp32 accumulation of the counterpart.
 *
 * Workspace: corr_build_workspace's size and layout in every mode.  A reduced mode writes and
 * reads only the pieces it keeps; the other bytes of the workspace keep what they held.  So:
 *   - CORR_BUILD_ONLY_MFMA in a mode needs a pack made in that mode or a finer one;
 *   - all corr_build_region_prec calls of one build (the CORR_REGION_PACK_QUERIES call and those
 *     that reuse its packed queries) must use ONE precision.
 *
 * Refusals, in this order: an unknown precision is CORR_EINVAL, before every other check; a
 * reduced precision with an algorithm other than CORR_BUILD_BF16X6 (CORR_BUILD_ONLY_PACK /
 * CORR_BUILD_ONLY_MFMA may be OR-ed in) is CORR_EUNSUPPORTED; then the counterpart's checks.
 */
#ifndef CORR_MI355X_BUILD_PREC_H
#define CORR_MI355X_BUILD_PREC_H

#include <stddef.h>

#include "corr_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

int corr_build_ex_prec(int algo, const float *fmap1_rows, int NQ, const float *fmap2, int B, int D, int H, int W,
                       int levels, float *const *pyr, void *workspace, size_t workspace_bytes, int precision,
                       void *stream);
int corr_build_region_prec(int algo, const float *fmap1_rows, int NQ, const float *fmap2_rows, int y0, int y1, int B,
                           int D, int H, int W, int levels, float *const *pyr, void *workspace,
                           size_t workspace_bytes, int flags, int precision, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CORR_MI355X_BUILD_PREC_H */
