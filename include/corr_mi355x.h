/*
 * corr_mi355x.h — C-ABI of libcorr_mi355x.so, the MI355X (gfx950) E-RAFT correlation hot path.
 *
 * Drop-in boundary for the reference CorrBlock (AhmedHumais/E-RAFT, model/corr.py:12-60).
 * Plain pointers and sizes only; no torch types.  Every pointer argument except the host
 * arrays of level pointers is DEVICE memory on the current HIP device; the caller allocates
 * everything (pyramid, outputs, gradients, workspace) and the library never allocates,
 * frees or synchronises.  All work is enqueued asynchronously on `stream` (a hipStream_t;
 * NULL = the default stream) and calls are graph-capturable.
 *
 * Layouts (fp32, C-contiguous), N = H*W, K = (2*radius+1)^2:
 *   fmap1, fmap2          [B][D][H][W]                       (corr.py:53-56)
 *   pyramid level l       B*N query maps of H_l x W_l cells, H_l = H>>l, W_l = W>>l
 *                         (corr.py:21-27, floor halving), each map TILED: 4x4-cell tiles of 64 B,
 *                         tiles row-major, cells row-major inside a tile:
 *                           cell (y, x) at ((y/4) * ceil(W_l/4) + x/4) * 16 + (y%4) * 4 + x%4,
 *                         corr_map_floats(H_l, W_l) = ceil(H_l/4) * ceil(W_l/4) * 16 floats per
 *                         map, maps consecutive (query q's map at q * corr_map_floats).  Cells
 *                         past W_l / H_l are padding (the builds may write them; never read).
 *                         Level pointers 16-byte aligned.  The reference's [B*N][H_l][W_l]
 *                         (corr.py's corr_pyramid) is corr_pyramid_export's output.
 *   coords                [B][2][H][W], ch0 = x, ch1 = y     (utils.py:24-27, corr.py:31)
 *   lookup output         [B][levels*K][H][W]                (corr.py:46-50)
 *   gradient pyramids     [B*N][H>>l][W>>l] row-major (corr_lookup_bwd, corr_pool_bwd,
 *                         corr_backward's scratch: the reference's layout; level 0 = dC [B*N][N])
 *
 * Return value: CORR_OK (0) or a negative CORR_E* code; corr_last_error() then returns a
 * thread-local message.  The reference performs no validation (torch raises inside
 * avg_pool2d / grid_sample); here bad arguments are rejected up front with CORR_EINVAL.
 * A level of height or width 1 is accepted and, like the reference (utils.py:11-12 divides
 * by W_l - 1 = 0), produces NaN for all of that level's channels and no gradient.
 */
#ifndef CORR_MI355X_H
#define CORR_MI355X_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CORR_OK 0
#define CORR_EINVAL -1       /* bad sizes / null or misaligned pointers            */
#define CORR_EUNSUPPORTED -2 /* valid for the reference, not built here (e.g. lookup_conv r != 4) */
#define CORR_EHIP -3         /* HIP launch / runtime error                          */

#define CORR_MAX_LEVELS 8
#define CORR_MAX_RADIUS 7

/* ABI version (major * 100 + minor).
 *   101: first ABI.
 *   102: corr_lookup_conv's weight argument is the opaque buffer written by
 *        corr_lookup_conv_weights (it was an fp32 [L*K][256] transpose under 101); callers
 *        built against 101 must check this version before calling it.
 *   103: CORR_BUILD_BF16X6, corr_build_region, corr_lookup_conv_bwd (the packed weight buffer
 *        grew: size it with corr_lookup_conv_weights_bytes()).
 *   104: corr_build_bwd_ex / corr_backward accept CORR_BUILD_BF16X6 (backward GEMMs on the exact
 *        bf16 split); E-RAFT's default backward for the BF16X6 build.
 *   200: the value pyramid (the builds' output, the lookups' input) is TILED (see Layouts;
 *        16-B aligned levels, corr_map_floats per map); corr_map_floats, corr_pyramid_export,
 *        corr_pyramid_import.  Gradient pyramids keep the reference layout.
 *   201: corr_backward's fused fold takes the separable closed form by default (dC within ~1e-7
 *        of the staged path, not bitwise); CORR_BACKWARD_EXACT_FOLD restores the bit-exact replay.
 *   202: the CORR_BUILD_BF16X6 backward GEMMs (corr_build_bwd_ex, corr_backward) give the fp32
 *        reference's results for non-finite inputs (+-inf where fp32 has +-inf; NaN only where it
 *        has NaN) instead of NaN for every output an infinity reaches.
 *        Added under 202 (purely additive, no version change): corr_ondemand_workspace,
 *        corr_ondemand_prepare, corr_ondemand_lookup; corr_ondemand_bwd_workspace,
 *        corr_ondemand_backward; corr_mask_upsample_weights_bytes,
 *        corr_mask_upsample_pack_weights, corr_mask_upsample_forward; corr_flow_enc_weights_bytes,
 *        corr_flow_enc_pack_weights, corr_flow_enc_forward, corr_flow_head_weights_bytes,
 *        corr_flow_head_pack_weights, corr_flow_head_forward. */
int corr_version(void);

/* Thread-local description of the last error on this thread ("" if none). */
const char *corr_last_error(void);

/* Floats of one query's tiled level map of H_l x W_l cells (ceil(H_l/4) * ceil(W_l/4) * 16). */
size_t corr_map_floats(int Hl, int Wl);

/*
 * The tiled pyramid <-> the reference's layout.  corr_pyramid_export writes every level as
 * [BN][H>>l][W>>l] row-major (the reference's corr_pyramid[l] viewed [B*N, 1, H_l, W_l],
 * corr.py:16,24,27,36); corr_pyramid_import tiles such levels into a pyramid (padding cells
 * zeroed), so a pyramid computed elsewhere can be looked up.  BN = B * NQ query maps; `pyr`,
 * `src`, `out` are host arrays of `levels` device pointers; the tiled side 16-B aligned.
 */
int corr_pyramid_export(const float *const *pyr, int BN, int H, int W, int levels, float *const *out, void *stream);
int corr_pyramid_import(const float *const *src, int BN, int H, int W, int levels, float *const *pyr, void *stream);

/*
 * All-pairs correlation + average-pool pyramid.  Replaces CorrBlock.__init__
 * (model/corr.py:13-27) together with CorrBlock.corr (model/corr.py:52-60):
 *   pyr[0][b*N + n](y, x) = sum_d fmap1[b][d][n] * fmap2[b][d][y*W + x] / sqrt(float(D))
 *   pyr[l][q](y, x)       = avg_pool2d(pyr[l-1], 2, stride 2)[q](y, x)   (floor)
 * (cell (y, x) of query q's tiled map, see Layouts.)  `pyr` is a HOST array of `levels` device
 * pointers.  levels == 1 gives CorrBlock.corr's [B,H,W,1,H,W] volume (export it for that view).  fp32 in / fp32 MFMA accumulate / fp32 out (CORR_BUILD_FP32;
 * corr_build_ex selects the faster CORR_BUILD_BF16X6, no less accurate, or CORR_BUILD_F16X3).
 */
int corr_build(const float *fmap1, const float *fmap2, int B, int D, int H, int W, int levels,
               float *const *pyr, void *stream);

/*
 * Build algorithms for corr_build_ex (same outputs, same pyramid arithmetic; they differ only
 * in how the fp32 dot products are formed — all accumulate in fp32):
 *   CORR_BUILD_FP32   fp32 operands on v_mfma_f32_32x32x2_f32 (the corr_build path).
 *   CORR_BUILD_BF16X6 each fp32 feature is split EXACTLY into three bf16 pieces, x = hi + mid +
 *                     lo (bf16 keeps fp32's exponent range: no scale, no flush — the one floor
 *                     is lo's bf16 subnormal range, |x| < ~2^-110); six bf16 MFMAs per product
 *                     (every piece pair of weight >= 2^-16: lo*hi + hi*lo + mid*mid + mid*hi +
 *                     hi*mid + hi*hi) into two fp32 accumulators (hi*hi; the five smaller ones),
 *                     added once.  The dropped terms are <= 2^-23 of |x_t x_q| and the main
 *                     accumulator rounds D/32 times per dot product (an fp32 fmaf chain: D
 *                     times): no narrower than CORR_BUILD_FP32 (checked per query row against
 *                     an fp64 oracle).  +-inf features split as (inf, 0, 0); a result whose
 *                     hi*hi sum is infinite is that sum, so infinities and NaNs land where the
 *                     fp32 build puts them (one exception: an infinity against a nonzero feature
 *                     below bf16's range, |x| < 2^-133, whose hi is 0: NaN where fp32 gives inf).
 *                     Needs a workspace for the split operands.
 *                     ~2x faster than CORR_BUILD_FP32 on gfx950.
 *   CORR_BUILD_F16X3  each fp32 feature x of pixel n is split as 2^e_n * (hi + lo), f16 hi/lo,
 *                     e_n putting the pixel's largest |x| in [2^14, 2^15); three f16 MFMAs
 *                     (hi*hi + hi*lo + lo*hi) per product into one fp32 accumulator.  Each
 *                     feature is carried to 2^-22 relative (fp32: 2^-24), and each product to
 *                     ~2^-21; features below 2^-38 of their pixel's largest flush to zero.
 *                     Needs a workspace for the packed operands.  ~1.5-1.7x faster on gfx950.
 */
#define CORR_BUILD_FP32 0
#define CORR_BUILD_F16X3 1
#define CORR_BUILD_BF16X6 2
/* Measurement only (OR-ed into CORR_BUILD_F16X3 / _BF16X6): run just one of its two kernels — the
 * operand pack, or the MFMA build from a workspace that already holds this pair's pack — so a
 * benchmark can time each kernel on its own.  The pyramid is complete only after both. */
#define CORR_BUILD_ONLY_PACK 0x100
#define CORR_BUILD_ONLY_MFMA 0x200

/* Bytes of device workspace corr_build_ex(algo, ...) needs (0 for CORR_BUILD_FP32;
 * (size_t)-1 if the algorithm does not support D). */
size_t corr_build_workspace(int algo, int B, int D, int NQ, int H, int W);

/*
 * corr_build_rows with an explicit algorithm and caller-allocated workspace (>= the size
 * corr_build_workspace returns, 256-byte aligned, also for corr_build_region; it may be reused
 * across calls on the same stream).
 * CORR_EUNSUPPORTED if `algo` cannot handle D.
 */
int corr_build_ex(int algo, const float *fmap1_rows, int NQ, const float *fmap2, int B, int D,
                  int H, int W, int levels, float *const *pyr, void *workspace,
                  size_t workspace_bytes, void *stream);

/*
 * One target-row region of corr_build_ex (CORR_BUILD_BF16X6 only): the pyramid entries of target
 * rows [y0, y1) — level l rows [y0 >> l, ceil(y1 / 2^l)) of every query's maps — from a slab
 * fmap2_rows [B][D][y1 - y0][W] holding just those rows of fmap2.  y0 a multiple of 8, y1 a
 * multiple of 8 or H, levels <= 4.  Calls over a partition of [0, H) with the same workspace
 * give the bits of one corr_build_ex call; the first call of a build sets
 * CORR_REGION_PACK_QUERIES (the query operand is packed into the workspace once and reused).
 * Lets a row-sharded caller build from fmap2 chunks as their broadcast arrives.
 */
#define CORR_REGION_PACK_QUERIES 1
int corr_build_region(int algo, const float *fmap1_rows, int NQ, const float *fmap2_rows, int y0, int y1, int B,
                      int D, int H, int W, int levels, float *const *pyr, void *workspace, size_t workspace_bytes,
                      int flags, void *stream);

/*
 * Window lookup.  Replaces CorrBlock.__call__ (model/corr.py:29-50) and bilinear_sampler
 * (model/utils.py:7-21):
 *   out[b][l*K + i*(2r+1) + j][h][w] = grid_sample(pyr[l][b*N + h*W + w],
 *        (x/2^l + i - r, y/2^l + j - r), bilinear, zeros, align_corners=True)
 * with (x, y) = coords[b][:][h][w].  The slow window index i moves x (corr.py:37-43).
 * Bit-identical to the reference on identical pyramids.  `pyr` is a host array.
 */
int corr_lookup(const float *const *pyr, const float *coords, int B, int H, int W, int levels,
                int radius, float *out, void *stream);

/*
 * Input-gradient of corr_lookup (autograd of model/utils.py:15; coords carry no gradient,
 * model/eraft.py:128).  ACCUMULATES into grad_pyr (host array of device pointers, same
 * shapes as the pyramid; zero it once before the first lookup of a build).  Deterministic:
 * a query's contributions stay inside its own map, summed in a fixed order, no atomics.
 */
int corr_lookup_bwd(const float *coords, const float *grad_out, int B, int H, int W, int levels,
                    int radius, float *const *grad_pyr, void *stream);

/*
 * avg_pool2d backward chain (autograd of model/corr.py:25-27), in place, coarse -> fine:
 *   grad_pyr[l-1][q][2y+a][2x+c] += grad_pyr[l][q][y][x] * 0.25      (l = levels-1 .. 1)
 * Afterwards grad_pyr[0] holds dLoss/dcorr.  BN = B*H*W query maps.
 */
int corr_pool_bwd(float *const *grad_pyr, int BN, int H, int W, int levels, void *stream);

/* Bytes of device workspace corr_build_bwd needs for these sizes. */
size_t corr_build_bwd_workspace(int B, int D, int H, int W);

/*
 * Backward of the all-pairs product and its 1/sqrt(D) scale (autograd of
 * model/corr.py:58-60).  grad_c: [B*N][N] (= grad_pyr[0] after corr_pool_bwd);
 *   dfmap1[b][d][n] = sum_m grad_c[b*N+n][m] * fmap2[b][d][m] / sqrt(D)
 *   dfmap2[b][d][m] = sum_n fmap1[b][d][n] * grad_c[b*N+n][m] / sqrt(D)
 * Both outputs are OVERWRITTEN.  Deterministic (split-K partial slabs summed in order).
 */
int corr_build_bwd(const float *grad_c, const float *fmap1, const float *fmap2, int B, int D,
                   int H, int W, float *dfmap1, float *dfmap2, void *workspace,
                   size_t workspace_bytes, void *stream);

/*
 * Row-slab variants, for query-row sharding across GPUs (no reference counterpart: the
 * reference has no multi-GPU CorrBlock).  The queries are NQ consecutive
 * pixels of fmap1 — a block of whole rows, NQ = rows*W — while the targets are all H*W
 * pixels of fmap2:
 *   fmap1_rows [B][D][NQ]; pyramid level l: B*NQ tiled maps of (H>>l) x (W>>l) cells;
 *   coords_rows [B][2][NQ]; out_rows [B][levels*K][NQ]; grad_c [B*NQ][H*W].
 * Every query's arithmetic is identical to the full-size call, so a row partition
 * reproduces the unsharded results bit for bit.  corr_build_bwd_rows writes this slab's
 * dfmap1 rows and its PARTIAL dfmap2 (sum it over the slabs, e.g. with an all-reduce).
 * The reference-shaped functions above are these with NQ = H*W.
 */
int corr_build_rows(const float *fmap1_rows, int NQ, const float *fmap2, int B, int D, int H,
                    int W, int levels, float *const *pyr, void *stream);
int corr_lookup_rows(const float *const *pyr, const float *coords_rows, int B, int NQ, int H,
                     int W, int levels, int radius, float *out_rows, void *stream);
int corr_lookup_bwd_rows(const float *coords_rows, const float *grad_out_rows, int B, int NQ,
                         int H, int W, int levels, int radius, float *const *grad_pyr,
                         void *stream);
size_t corr_build_bwd_rows_workspace(int B, int D, int NQ, int H, int W);
int corr_build_bwd_rows(const float *grad_c, const float *fmap1_rows, int NQ, const float *fmap2,
                        int B, int D, int H, int W, float *dfmap1_rows, float *dfmap2,
                        void *workspace, size_t workspace_bytes, void *stream);

/*
 * Backward GEMMs with an explicit algorithm (the corr_build_ex counterpart of
 * corr_build_bwd_rows; same outputs and contract).  CORR_BUILD_FP32 is corr_build_bwd_rows;
 * CORR_BUILD_BF16X6 splits every element of F1 / F2 / dC EXACTLY into three bf16 pieces while
 * staging it (no scales, no maxima; the one floor as for the build: |x| < ~2^-110) and runs the
 * six piece products of weight >= 2^-16 per product on the bf16 MFMA into one fp32 accumulator
 * (6 roundings per 16 k, an fp32 fmaf chain 16): every element within (3 + 6 ceil(K/16) + splits)
 * u sum|ab| (an fp32 dot product: K u sum|ab|), worst and mean row error below the fp32 GEMMs',
 * checked against fp64 — but with one accumulator not every single row (unlike the build's).
 * Non-finite inputs give the fp32 reference's results: an output the split makes NaN (an
 * infinite element meets zero pieces: inf * 0) is recomputed by the split-K reduce as the
 * reference computes it (dC / sqrt(D), then an fp32 dot product), so it becomes +-inf where
 * fp32 has +-inf and stays NaN where fp32 has NaN; finite inputs are unaffected
 * (tests/test_gpu_parity.py::test_build_bwd_bf16x6_inf_matches_fp32).
 * CORR_BUILD_F16X3 packs F1, F2 (per feature row d) and dC (per query
 * row for dfmap1, per target column for dfmap2) as 2^e (hi + lo) f16 pairs and runs three f16
 * MFMAs per product (~2^-22 relative: narrower than fp32).  Split-K partial sums are reduced in
 * split order (deterministic).
 * Workspace: corr_build_bwd_ex_workspace(algo, ...) bytes ((size_t)-1: unknown algo).
 * Replaces the autograd of model/corr.py:58-60 (bmm + division by sqrt(D)).
 */
size_t corr_build_bwd_ex_workspace(int algo, int B, int D, int NQ, int H, int W);
int corr_build_bwd_ex(int algo, const float *grad_c, const float *fmap1_rows, int NQ,
                      const float *fmap2, int B, int D, int H, int W, float *dfmap1_rows,
                      float *dfmap2, void *workspace, size_t workspace_bytes, void *stream);

/*
 * The backward of one build and all its lookups in three launches (autograd of model/corr.py:
 * 25-27, 45, 58-60 for the whole GRU loop at once; coords carry no gradient, eraft.py:128).
 * coords_rows / grad_out_rows: HOST arrays of T device pointers, the lookups' coords and upstream
 * gradients ([B][2][NQ], [B][levels*K][NQ]), accumulated in this order.
 *   corr_lookup_bwd_multi: the T lookups' input-gradients into grad_pyr, which it OVERWRITES
 *     (zero-initialised inside the kernel: no memset; each workgroup's RMWs stay L2-resident).
 *     Per cell G = ((0 + S_0) + S_1) + ... with S_t lookup t's scatter-order sum: bit-identical to
 *     zeroing grad_pyr and calling corr_lookup_bwd_rows for t = 0..T-1.
 *   corr_pool_fold: the avg_pool2d backward of every level folded into level 0 in place (one pass;
 *     bit-identical to corr_pool_bwd): afterwards grad_pyr[0] = dLoss/dcorr.
 *   corr_backward: both, then the two GEMMs of corr_build_bwd_ex; grad_pyr is scratch (left =
 *     dC in level 0), the outputs dfmap1_rows / dfmap2 as corr_build_bwd_ex.  When the
 *     workgroup's LDS image fits (levels <= 4, T <= 32, BQ = 64 / pow2ceil(2r+3) queries' maps of
 *     every level in 160 KiB: e.g. r = 4 up to 60x80 fmaps), the lookups and the fold run as ONE
 *     kernel whose gradient maps live in LDS and which writes only dC (plus dC's row maxima and
 *     per-workgroup column maxima for the F16X3 packs; BF16X6 needs none); otherwise corr_lookup_bwd_multi +
 *     corr_pool_fold.  At radius 4 the fused kernel sums a window's cells separably (the column's
 *     x-taps first, then the y-taps: the same (tap, corner) terms per cell with the reference's
 *     per-tap weights, rounded in another order — dC within ~1e-7 norm-relative of the staged
 *     path; windows whose taps are not all on a regular grid, e.g. the cold-start integer grid,
 *     by the general form with four slots per tap; a window with a corner outside its
 *     neighbourhood, or in a wave holding a non-finite upstream gradient, by the reference's
 *     sequential scatter, so infinities give the staged path's inf / NaN cells);
 *     algo | CORR_BACKWARD_EXACT_FOLD makes it replay grid_sampler_2d_backward's
 *     per-tap products instead, bit-identical to corr_lookup_bwd_multi + corr_pool_fold (as every
 *     other radius and the non-fused path always are).  Workspace: corr_backward_workspace
 *     (radius sizes the column-maxima partials; the flag does not change it).
 */
#define CORR_BACKWARD_EXACT_FOLD 0x400
int corr_lookup_bwd_multi(const float *const *coords_rows, const float *const *grad_out_rows, int T, int B,
                          int NQ, int H, int W, int levels, int radius, float *const *grad_pyr, void *stream);
int corr_pool_fold(float *const *grad_pyr, int B, int NQ, int H, int W, int levels, void *stream);
size_t corr_backward_workspace(int algo, int B, int D, int NQ, int H, int W, int radius);
int corr_backward(int algo, const float *const *coords_rows, const float *const *grad_out_rows, int T,
                  const float *fmap1_rows, int NQ, const float *fmap2, int B, int D, int H, int W, int levels,
                  int radius, float *const *grad_pyr, float *dfmap1_rows, float *dfmap2, void *workspace,
                  size_t workspace_bytes, void *stream);

/*
 * On-demand window lookup: corr_lookup's output without the all-pairs pyramid (RAFT's
 * AlternateCorrBlock; the reference keeps its import commented out, model/corr.py:5-9).  Average
 * pooling is linear, so level l of the pyramid is the correlation of fmap1 with fmap2 pooled l
 * times, and only the entries a lookup touches are computed, straight from the feature maps:
 *   P_0 = fmap2,  P_l = avg_pool2d(P_{l-1}, 2, stride 2)            (fp32, corr_build's pool order)
 *   C_l[b][n](y, x) = (sum_d fmap1[b][d][n] * P_l[b][d][y][x]) / sqrt(float(D))   inside H_l x W_l, else 0
 *   out[b][l*K + i*(2r+1) + j][n] = bilinear(C_l[b][n], tap (i, j))
 * Tap coordinates, floors, corner weights, zero padding, the corner order (nw, ne, sw, se, fmaf)
 * and the channel order are corr_lookup's, bit for bit; out-of-map, far, NaN and +-inf coordinates
 * and one-cell levels give exactly corr_lookup's zeros and NaNs.
 *
 * Accuracy: fp32 operands, fp32 fmaf accumulation (nothing is rounded to a narrower format); the
 * dot products are summed in another order than the builds', so the output equals corr_lookup's
 * on a corr_build pyramid within 1e-4 norm-relative (measured ~1e-6), not bit for bit.  Non-finite
 * FEATURE values are not parity-checked: inf * 0 lands in other cells when features are pooled
 * first.  Deterministic: no atomics, a fixed summation order.
 *
 * corr_ondemand_prepare pools fmap2 and writes both operands pixel-major into the workspace
 * (16-byte aligned, >= corr_ondemand_workspace bytes), Dp = D rounded up to a multiple of 4:
 *   float fmap1_rows[B][H*W][Dp]; then for l = 0 .. levels-1: float P_l[B][H_l*W_l][Dp]
 * (channels D .. Dp-1 zero), so one cell's features are one contiguous row (1 KiB at D = 256):
 * 4*B*Dp*(H*W + sum_l H_l*W_l) bytes, e.g. 92 MB at 160x240, D = 256, 4 levels, where the pyramid
 * takes 7.9 GB.  corr_ondemand_lookup may then be called any number of times (every GRU
 * iteration) with the same sizes.  corr_ondemand_workspace returns 0 for sizes the calls reject
 * (B, D, H, W < 1, levels outside 1..CORR_MAX_LEVELS, a map too small for the levels, operands
 * beyond 2^37 floats).
 *
 * flags: 0 = the library picks the path per workgroup; CORR_ONDEMAND_GENERAL forces the general
 * path everywhere (so the two can be compared).
 *   general: a wave per query and level gathers the rows of the (2r+2)^2 cells its taps touch and
 *            forms the dot products with VALU fmaf.  Any radius, levels, D, coordinates.
 *   tiled:   (radius <= 4) a workgroup owns an 8x8 block of queries of one batch item at one level,
 *            stages the rows of the bounding box of their neighbourhoods in LDS and forms the
 *            query x cell products on v_mfma_f32_32x32x2_f32 (fp32 operands, fp32 fmaf chain).
 *            Cap: the box (unclipped) holds at most 416 cells — 18x18 = 324 is uniform flow at
 *            level 0 and radius 4; 20x20 fits.  A workgroup whose box exceeds the cap, or that
 *            holds a query with far / non-finite coordinates or irregular taps (|coordinate|
 *            near 2^20), takes the general path: the choice is a function of the coordinates
 *            only, so results are deterministic run to run.
 * The two paths sum the dot products in different orders: equal within the accuracy contract
 * above, not bit for bit.  The backward is corr_ondemand_backward (below).
 */
#define CORR_ONDEMAND_GENERAL 1
size_t corr_ondemand_workspace(int B, int D, int H, int W, int levels);
int corr_ondemand_prepare(const float *fmap1, const float *fmap2, int B, int D, int H, int W, int levels,
                          void *workspace, size_t workspace_bytes, void *stream);
int corr_ondemand_lookup(const void *workspace, const float *coords, int B, int D, int H, int W, int levels,
                         int radius, int flags, float *out, void *stream);

/*
 * The on-demand lookup's backward: dfmap1 / dfmap2 of one corr_ondemand_prepare and its T lookups
 * (coords[t], grads[t] = the upstream gradient of lookup t, [B][levels*K][H*W]; host arrays of
 * device pointers, processed in list order), without the all-pairs volume or its gradient.  With
 * Wg_t[b][n][l][cell] = the sum, over the taps and corners of query n that land on `cell` inside
 * H_l x W_l, of corner weight * grads[t][b][l*K + i*(2r+1) + j][n] (the forward's weights):
 *   dF1[b][n][:]     = 1/sqrt(D) * sum_t sum_l sum_cell Wg_t[b][n][l][cell] * P_l[b][cell][:]
 *   dP_l[b][cell][:] = 1/sqrt(D) * sum_t sum_n Wg_t[b][n][l][cell] * F1[b][n][:]
 *   dfmap2 = dP_0 + poolT(dP_1 + poolT(dP_2 + ...))   (a coarse cell gives 0.25 of itself to each of
 *            its four children; rows / columns dropped by the floor halving receive nothing)
 * i.e. autograd of the lookups above with respect to both feature maps (there is no gradient to the
 * coordinates).  Far, NaN and +-inf coordinates and one-cell levels contribute nothing, as in
 * corr_backward.  fp32 throughout, no float atomics, a fixed summation order: reruns are
 * bit-identical.  dfmap1 / dfmap2 ([B][D][H][W], overwritten) may each be NULL: that side's work is
 * skipped; both NULL is an error.
 *
 * fwd_workspace: as prepared by corr_ondemand_prepare for the same B, D, H, W, levels.
 * bwd_workspace: 16-byte aligned, uninitialised, >= corr_ondemand_bwd_workspace bytes,
 * Dp = D rounded up to a multiple of 4, S = 2*radius + 1:
 *   float dF1rows[B][H*W][Dp]; for l = 0 .. levels-1: float dProws_l[B][H_l*W_l][Dp];
 *   for l = 1 .. levels-1: float part_l[seg_l][B][H_l*W_l][Dp], seg_l = min(4^l, 64)   (the dP gather
 *   cuts a coarse level's queries into seg_l segments; one lookup's partial sums, reused);
 *   int origin[B][levels][H*W][2]; float block[B][levels][H*W][(S+2)*(S+2)]   (one lookup's, reused)
 * = 4 * B * (Dp * (H*W + sum_l H_l*W_l + sum_{l>=1} seg_l*H_l*W_l) + levels * H*W * ((S+2)*(S+2) + 2))
 * bytes, e.g. 285 MB at 160x240, D = 256, 4 levels, radius 4 (CorrBlock's training there holds the
 * 7.9 GB pyramid and as much again of its gradient).  corr_ondemand_bwd_workspace returns 0 for the sizes
 * corr_ondemand_workspace rejects, a radius outside 0..CORR_MAX_RADIUS, and H or W above 65536.
 */
size_t corr_ondemand_bwd_workspace(int B, int D, int H, int W, int levels, int radius);
int corr_ondemand_backward(const void *fwd_workspace, const float *const *coords, const float *const *grads, int T,
                           int B, int D, int H, int W, int levels, int radius, void *bwd_workspace,
                           size_t bwd_workspace_bytes, float *dfmap1, float *dfmap2, void *stream);

/*
 * Warm-start forward splat.  Replaces forward_interpolate_pytorch (utils/image_utils.py:52-83)
 * with grid_sample_values (:10-50): flow [B][2][H][W] -> out [B][2][H][W], every source pixel
 * splatted to its floor / ceil neighbours with bilinear weights, out = sum(z w) / (sum(w) +
 * 1e-15).  Deterministic and bit-identical to the reference's CPU put_(accumulate=True) order
 * (corner-major, source order; an integer coordinate's floor == ceil corner counts twice, as
 * in the reference).  Workspace: corr_forward_splat_workspace(B, H, W) bytes.
 */
size_t corr_forward_splat_workspace(int B, int H, int W);

/*
 * Lookup fused with its consumer, BasicMotionEncoder's cor = relu(convc1(corr))
 * (model/update.py:68,75; a 1x1 convolution L*(2r+1)^2 -> 256): the window lookup of
 * corr_lookup into an on-chip tile, then out[b][o][h][w] = (relu?)(bias[o] +
 * sum_c weight[o][c] * corr[b][c][h][w]) on the bf16 MFMA with CORR_BUILD_BF16X6's exact
 * three-piece split (six products per fp32 product, no scales: no narrower than fp32).  The weight (convc1.weight viewed [256][L*K], fp32) is split once
 * per weight version by corr_lookup_conv_weights into a corr_lookup_conv_weights_bytes() buffer;
 * out [B][256][H][W].  radius 4, levels <= 4 (E-RAFT); CORR_EUNSUPPORTED otherwise.  This call
 * is the forward; corr_lookup_conv_bwd below is its training backward.
 */
size_t corr_lookup_conv_weights_bytes(void);
int corr_lookup_conv_weights(const float *weight, int out_channels, int in_channels, void *packed, void *stream);
int corr_lookup_conv(const float *const *pyr, const float *coords, int B, int H, int W,
                     int levels, int radius, const void *packed_weight, const float *bias, int relu,
                     float *out, void *stream);

/*
 * The ON-DEMAND lookup fused with the same consumer: out[b][o][h][w] = (relu?)(bias[o] +
 * sum_c weight[o][c] * lookup[b][c][h][w]) where lookup = what corr_ondemand_lookup writes for the
 * same workspace, coords and flags — in one launch, the [B][levels*81][H][W] lookup is never
 * stored.  workspace: as prepared by corr_ondemand_prepare for the same B, D, H, W, levels;
 * packed_weight: corr_lookup_conv_weights' pack (the same buffer serves corr_lookup_conv);
 * bias [256]; out [B][256][H][W], overwritten.  flags as corr_ondemand_lookup's: the route (tiled
 * / general) is chosen per 8x8 block of queries and level from the coordinates only, and
 * CORR_ONDEMAND_GENERAL forces the general routine for every block.  radius 4, levels <= 4
 * (E-RAFT); CORR_EUNSUPPORTED otherwise.  Inference only: there is no fused backward (compose
 * corr_ondemand_lookup with the convolution for training).
 *
 * Accuracy contract.  The values entering the convolution equal corr_ondemand_lookup's bit for
 * bit (same routines, same route choice, same summation order), so a weight that selects single
 * channels returns them exactly.  The convolution is corr_lookup_conv's: each fp32 product
 * weight * lookup is formed from the exact three-piece bf16 splits of both factors (x = hi + mid +
 * lo) as six piece products on v_mfma_f32_16x16x32_bf16 with fp32 accumulation — no narrower
 * than fp32, no scales.  Summation order per output: c = l*81 + i*9 + j ascending, padded with
 * zeros to 352, in 11 steps of 32 channels; within a step and across steps the leading products
 * (hi * hi) accumulate in one fp32 register and the five smaller ones (lo*hi, hi*lo, mid*mid,
 * mid*hi, hi*mid, in that order) in a second; out = (first is infinite ? first : first + second) +
 * bias, then ReLU as torch's (a NaN stays a NaN).  Against relu(conv2d(lookup)) in fp64: within
 * 1e-5 of the largest output (measured ~2e-7).  A non-finite lookup value (non-finite
 * coordinates and one-cell levels give NaN, as in corr_ondemand_lookup; non-finite features may
 * give one) reaches all 256 outputs of its query.  Deterministic:
 * no atomics, reruns are bit-identical.
 */
int corr_ondemand_lookup_conv(const void *workspace, const float *coords, int B, int D, int H, int W, int levels,
                              int radius, int flags, const void *packed_weight, const float *bias, int relu,
                              float *out /* [B][256][H][W] */, void *stream);

/*
 * Training backward of corr_lookup_conv (autograd of update.py:68,75 through corr.py:29-50).
 * grad_out = dL/d out [B][256][H][W]; with relu, g' = grad_out where out > 0 (or out is NaN),
 * else 0 (torch's threshold backward; `out` is the forward's output, unused without relu).
 *   grad_weight [256][levels*K] = sum_{b,n} g'[b][o][n] lookup[b][c][n]    (OVERWRITTEN)
 *   grad_bias   [256]           = sum_{b,n} g'[b][o][n]                    (OVERWRITTEN)
 *   grad_lookup [B][levels*K][H][W] = sum_o weight[o][c] g'[b][o][n]  — the lookup's upstream
 *               gradient, to be passed to corr_backward / corr_lookup_bwd like a plain lookup's
 * Any of the three may be NULL (not computed).  The lookup is recomputed on chip (bit-identical
 * to corr_lookup's values) and never written.  Both products run on the bf16 MFMA with the
 * exact three-piece split of CORR_BUILD_BF16X6 (six products per fp32 product, no scales);
 * dW and the bias sum per-workgroup partials in a fixed order (deterministic).  packed_weight
 * from corr_lookup_conv_weights; workspace of corr_lookup_conv_bwd_workspace(B, H, W, levels)
 * bytes (16-B aligned) when grad_weight or grad_bias is requested.  When H*W is a multiple of 4
 * the kernels take 16-byte loads of grad_out and (with relu) out, which must then be 16-byte
 * aligned (CORR_EINVAL otherwise).  radius 4, levels <= 4.
 */
size_t corr_lookup_conv_bwd_workspace(int B, int H, int W, int levels);
int corr_lookup_conv_bwd(const float *const *pyr, const float *coords, int B, int H, int W, int levels, int radius,
                         const void *packed_weight, const float *out, int relu, const float *grad_out,
                         float *grad_weight, float *grad_bias, float *grad_lookup, void *workspace,
                         size_t workspace_bytes, void *stream);

/*
 * DSEC event -> voxel grid.  Replaces VoxelGrid.convert (utils/dsec_utils.py:26-64) as the DSEC
 * loader calls it (loader/loader_dsec.py:245-257): events as float32 device arrays x, y, t
 * (t in [0, 1], ascending), p in {0, 1}; out [C][H][W].  Bilinear in x and y, nearest-lower
 * bin in t (the reference's t loop is commented out); the raw grid is bit-identical to the
 * reference run single-threaded (main.py:2-5) — deterministic, no float atomics.  normalize:
 * nonzero cells -> (v - mean) / std (unbiased std; fp64 statistics, tolerance-level).
 * Workspace: corr_voxel_grid_workspace(n_events, C, H, W) bytes.
 */
size_t corr_voxel_grid_workspace(int n_events, int C, int H, int W);
int corr_voxel_grid(const float *x, const float *y, const float *t, const float *p, int n_events,
                    int C, int H, int W, int normalize, float *out, void *workspace,
                    size_t workspace_bytes, void *stream);

/*
 * MVSEC event -> voxel grid.  Replaces EventSequenceToVoxelGrid_Pytorch.__call__
 * (utils/transformers.py:36-126), the representation of loader/loader_mvsec_flow.py:35:
 * events [n_events][4] float64 device rows (t, x, y, p), as the loader's event_sequence.features
 * .astype('float') holds them (t ascending in practice; t_0 = row 0, t_end = the last row);
 * out [C][H][W].  Bilinear in t: t_n = (C-1)(t - t_0)/(t_end - t_0) (fp64), each event adds
 * p(1 - dt) at bin floor(t_n) and p dt at floor(t_n) + 1 (p = 0 -> -1, dt rounded to fp32),
 * at flat index trunc(x) + trunc(y) W + bin H W.  The raw grid is bit-identical to the
 * reference's two index_add_ passes (left then right, event order) — deterministic, no float
 * atomics.  An entry whose flat index falls outside the grid is dropped (the reference raises).
 * normalize: as corr_voxel_grid.  Workspace: corr_voxel_grid_tbilinear_workspace(...) bytes.
 */
size_t corr_voxel_grid_tbilinear_workspace(int n_events, int C, int H, int W);
int corr_voxel_grid_tbilinear(const double *events, int n_events, int C, int H, int W,
                              int normalize, float *out, void *workspace, size_t workspace_bytes,
                              void *stream);

/*
 * Convex upsampling of the 1/8-resolution flow after every GRU iteration.  Replaces
 * ERAFT.upsample_flow (model/eraft.py:75-86): softmax over the 9 taps of mask
 * [N][9*64][h][w], weighted sum of the zero-padded 3x3 neighbourhood of 8*flow [N][2][h][w]
 * -> out [N][2][8h][8w], in one pass (fp32; tolerance-level parity, the reference's
 * reduction order is ATen's).
 */
int corr_convex_upsample(const float *flow, const float *mask, int N, int h, int w, float *out,
                         void *stream);
/*
 * Backward of corr_convex_upsample (autograd of model/eraft.py:75-86 w.r.t. flow and mask):
 * grad_out [N][2][8h][8w] -> dflow [N][2][h][w], dmask [N][576][h][w] (both overwritten).
 * Softmax backward p_k (dv_k - sum p dv) per sub-pixel; dflow gathers 8 * sum p_k G over the
 * sub-pixels and taps that read each coarse pixel.  Workspace: the per-tap partial sums,
 * corr_convex_upsample_bwd_workspace(N, h, w) bytes.  fp32, tolerance-level parity.
 */
size_t corr_convex_upsample_bwd_workspace(int N, int h, int w);
int corr_convex_upsample_bwd(const float *flow, const float *mask, const float *grad_out, int N, int h, int w,
                             float *dflow, float *dmask, void *workspace, size_t workspace_bytes, void *stream);
int corr_forward_splat(const float *flow, int B, int H, int W, float *out, void *workspace,
                       size_t workspace_bytes, void *stream);

/*
 * One half step of the update block's SepConvGRU (model/update.py:45-60), inference only (no
 * backward).  dir 0 = the horizontal 1x5 convolutions (padding (0,2)), dir 1 = the vertical 5x1
 * ones (padding (2,0)); C = hidden + input:
 *   z  = sigmoid(bz + convz([h, x]))        r = sigmoid(br + convr([h, x]))
 *   q  = tanh(bq + convq([r*h, x]))         h_out = (1 - z) * h + z * q
 * Layouts: h, h_out [B][hidden][H][W]; x [B][input][H][W] (h and x are two pointers, no cat);
 * wz, wr, wq [hidden][C][5] (a contiguous (1,5) and a contiguous (5,1) Conv2d weight both are),
 * tap t multiplies the pixel (t - 2) columns (dir 0) or rows (dir 1) away, zero outside the map;
 * bz, br, bq [hidden].  All fp32, 4-byte aligned.
 * Arithmetic: two launches (gates: z and r*h into the workspace, r is never stored; candidate:
 * q and the blend).  Each convolution is an implicit GEMM with K = 5 C on the bf16 MFMA with
 * CORR_BUILD_BF16X6's exact three-piece split (six products per fp32 product, no scales: no
 * narrower than fp32), fp32 accumulation in a fixed order (32-channel chunk outer, tap inner), so
 * results are deterministic.  sigmoid(v) = 1 / (1 + expf(-v)) and tanhf(v), each fp32 op rounded
 * once.  Finite inputs give finite outputs; non-finite inputs are NOT parity-checked (an
 * infinite activation meets the zero low pieces of the weights and comes out NaN).
 * The weights are split once per weight version by corr_gru_pack_weights into a
 * corr_gru_weights_bytes(hidden, input) buffer (16-B aligned, opaque; 0 for unsupported sizes).
 * Workspace: corr_gru_workspace(B, hidden, H, W) bytes, 16-B aligned = z then r*h, each
 * [B][hidden][H][W] fp32 rounded up to 256 bytes (0 when a size is < 1).  h_out must not alias
 * h or x.  hidden = 128, C a multiple of 32 and <= 1024, any B, H, W >= 1 with B*H*W < 2^31;
 * other channel counts return CORR_EUNSUPPORTED.  No allocation, no synchronisation; the
 * launches go on `stream` and can be captured into a graph.
 */
size_t corr_gru_weights_bytes(int hidden, int input);
int corr_gru_pack_weights(const float *wz, const float *wr, const float *wq, int hidden, int input, void *packed,
                          void *stream);
size_t corr_gru_workspace(int B, int hidden, int H, int W);
int corr_gru_half_step(const float *h, const float *x, int B, int hidden, int input, int H, int W, int dir,
                       const void *packed, const float *bz, const float *br, const float *bq, void *workspace,
                       size_t workspace_bytes, float *h_out, void *stream);

/*
 * Reduced precision for the per-iteration kernels (opt-in; the counterpart of the reference's
 * mixed_precision, model/eraft.py:31,102-133).  A mode keeps fewer of the pieces of the exact
 * three-piece bf16 split x = hi + mid + lo of BOTH operands (the split's guards included, so an
 * infinite operand still splits as (inf, 0, 0) and the non-finite pattern stays fp32's) and
 * multiplies only the products among the kept pieces, in this order per K step:
 *   CORR_PREC_BF16X6  hi, mid, lo  the six products of corr_gru_half_step / corr_conv_forward
 *   CORR_PREC_BF16X3  hi, mid      acs += wm xh; acs += wh xm; acc += wh xh   (joined at the end)
 *   CORR_PREC_BF16    hi           acc += wh xh                              (one accumulator)
 * The accumulators are fp32 in every mode and the K order is unchanged.  With S = sum |w| |x|
 * over an output's products, the operand rounding adds at most 2^-16 S (BF16X3) or
 * (2^-8 + 2^-18) S (BF16) to the fp32 accumulation error.  The packs are the same for every mode.
 * corr_gru_half_step_prec and corr_conv_forward_prec are corr_gru_half_step and corr_conv_forward
 * with `precision` (before `stream`); CORR_PREC_BF16X6 is bit-identical to them.  An unknown
 * precision is CORR_EINVAL, refused before every other check and before any HIP call.
 */
#define CORR_PREC_BF16X6 0
#define CORR_PREC_BF16X3 1
#define CORR_PREC_BF16 2
int corr_gru_half_step_prec(const float *h, const float *x, int B, int hidden, int input, int H, int W, int dir,
                            const void *packed, const float *bz, const float *br, const float *bq, void *workspace,
                            size_t workspace_bytes, float *h_out, int precision, void *stream);

/*
 * A 3x3 convolution (stride 1, zero padding 1) with bias and an optional ReLU, inference only
 * (no backward): the update block's convc2, convf2, conv and the first convolutions of the flow
 * head and the mask head (model/update.py:63-107).
 *   out[b][out_offset + o][y][x] =
 *       act(bias[o] + sum_c sum_ky sum_kx w[o][c][ky][kx] * in[b][c][y + ky - 1][x + kx - 1])
 * for o < cout; act is the identity (relu = 0) or max(., 0) (relu = 1).
 * Input: `in` is the channel-wise concatenation of in_a [B][ca][H][W] and in_b [B][cb][H][W],
 * two pointers and no cat; the boundary ca is any multiple of 32.  in_b is ignored (may be NULL)
 * when cb = 0.
 * Output: out is a [B][out_channels][H][W] tensor of which only channels out_offset ..
 * out_offset + cout - 1 are written; every other byte of it is left as it was, so a producer can
 * write straight into the buffer its consumer reads.  out's byte range must not overlap in_a's
 * or in_b's (a workgroup reads its neighbours' pixels).
 * Weights: w is a contiguous Conv2d weight [cout][cin][3][3], cin = ca + cb.  It is split once per
 * weight version by corr_conv_pack_weights into a corr_conv_weights_bytes(cout, cin) buffer (16-B
 * aligned, opaque; 0 for unsupported sizes).  Several convolutions over the same input run as one
 * launch by packing their weights stacked along cout.  The pack holds the rows padded with zeros
 * to a multiple of 64; padding rows are never stored to `out`.
 * bias is [cout], or NULL for no bias.  All tensors fp32, 4-byte aligned.
 * Arithmetic: one launch, an implicit GEMM with K = 9 cin on the bf16 MFMA with
 * CORR_BUILD_BF16X6's exact three-piece split (six products per fp32 product, no scales: no
 * narrower than fp32), fp32 accumulation in a fixed order (32-channel chunk outer, tap inner with
 * ky major and kx minor), then + bias and the ReLU, each fp32 op rounded once: deterministic.
 * Finite inputs give finite outputs; non-finite inputs are NOT parity-checked (an infinite
 * activation meets the zero low pieces of the weights and comes out NaN).
 * Sizes: ca >= 32 and cb >= 0, each a multiple of 32, ca + cb <= 1024; 1 <= cout <= 1024; any
 * B, H, W >= 1 with B*H*W < 2^31; other channel counts return CORR_EUNSUPPORTED.  CORR_EINVAL:
 * a NULL in_a, packed or out; in_b NULL with cb > 0; relu not 0 or 1; out_offset < 0 or
 * out_offset + cout > out_channels; packed not 16-byte aligned; B, H or W < 1; out overlapping
 * an input.  Every refusal comes before any HIP call.  No workspace, no allocation, no
 * synchronisation; the launch goes on `stream` and can be captured into a graph.
 */
size_t corr_conv_weights_bytes(int cout, int cin);
int corr_conv_pack_weights(const float *w, int cout, int cin, void *packed, void *stream);
int corr_conv_forward(const float *in_a, int ca, const float *in_b, int cb, int B, int H, int W,
                      const void *packed, const float *bias, int cout, int relu, float *out,
                      int out_channels, int out_offset, void *stream);
/* corr_conv_forward in a CORR_PREC_* mode (see corr_gru_half_step_prec). */
int corr_conv_forward_prec(const float *in_a, int ca, const float *in_b, int cb, int B, int H, int W,
                           const void *packed, const float *bias, int cout, int relu, float *out,
                           int out_channels, int out_offset, int precision, void *stream);

/*
 * The encoders' residual stages (model/extractor.py: ResidualBlock with norm_fn "instance" or,
 * in eval mode, "batch"), inference only.  A block is
 *   y1 = conv1(x) [stride 1 or 2];  y2 = conv2(relu(norm1(y1)));  out = relu(skip + relu(norm2(y2)))
 * and runs as corr_enc_conv_forward (statistics) -> corr_enc_norm_finalize -> corr_enc_conv_forward
 * (norm on load, statistics) -> corr_enc_norm_finalize -> corr_enc_join.  An eval-mode batch norm
 * passes its own scale = gamma / sqrt(running_var + eps), shift = beta - running_mean * scale
 * with norm_per_batch = 0 and needs neither statistics nor finalize.
 *
 * corr_enc_conv_forward: the 3x3 convolution of corr_conv_forward (same pack, from
 * corr_conv_pack_weights; same arithmetic, K order and six-product order) at stride 1 or 2 with
 * zero padding 1, Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1 (odd sizes allowed), bias
 * and no ReLU:
 *   out[b][o][y][x] = bias[o] + sum_c sum_ky sum_kx w[o][c][ky][kx] * n(in)[b][c][stride y + ky - 1][stride x + kx - 1]
 * in is [B][cin][H][W], out [B][cout][Ho][Wo].  With in_scale and in_shift given,
 *   n(v)[b][c] = max(v * in_scale[k] + in_shift[k], 0),  k = b cin + c (norm_per_batch = 1: [B][cin])
 *                                                         or c (norm_per_batch = 0: [cin]),
 * two fp32 operations rounded separately, then the max; with both NULL, n(v) = v.  Positions
 * outside the map are zero AFTER n: the padding is zero in the normalised domain.
 * stats (may be NULL) receives one pair of floats per (batch item, output channel, 4 x 16 pixel
 * tile of the output), layout [B][cout][ceil(Ho/4) * ceil(Wo/16)][2], tiles row-major: the sum of
 * out over the tile's pixels inside the map, and the sum of their squared deviations from that
 * tile's own mean.  Within a tile the values are combined in a fixed order (no atomics):
 * deterministic.  stats_bytes must be >= corr_enc_stats_bytes(B, cout, Ho, Wo), which is exactly
 * the bytes written (0 for sizes < 1); nothing past it is touched.
 *
 * corr_enc_norm_finalize: merges the tile pairs of each (b, c) in ascending tile order (Chan et
 * al.'s pairwise update, fp64; a tile's pixel count follows from Ho, Wo) into the biased variance
 * and writes scale[b][c] = 1 / sqrt(var + eps), shift[b][c] = -mean * scale as fp32 ([B][C] each):
 * InstanceNorm2d without affine parameters.  Ho * Wo = 1 gives scale = 1 / sqrt(eps).
 *
 * corr_enc_join: out = max(skip + max(y * scale[k] + shift[k], 0), 0) elementwise on [B][C][H][W]
 * tensors, k as above; each fp32 op rounded once.  out may be y (or skip) itself.
 *
 * Sizes: cin a multiple of 32 in 32 .. 1024 and 1 <= cout <= 1024, stride 1 or 2, otherwise
 * CORR_EUNSUPPORTED.  CORR_EINVAL: a NULL in, packed or out (finalize: stats, scale, shift; join:
 * y, scale, shift, skip, out); exactly one of in_scale / in_shift NULL; stats with stats_bytes too
 * small; packed not 16-byte aligned; B, C, H or W < 1 or B*H*W >= 2^31 (B*C >= 2^31); eps not
 * positive; out overlapping in.  Every refusal comes before any HIP call.  No allocation, no
 * synchronisation; everything goes on `stream` and can be captured into a graph.
 */
size_t corr_enc_stats_bytes(int B, int cout, int Ho, int Wo);
int corr_enc_conv_forward(const float *in, int cin, int B, int H, int W, int stride, const float *in_scale,
                          const float *in_shift, int norm_per_batch, const void *packed, const float *bias,
                          int cout, float *out, void *stats, size_t stats_bytes, void *stream);
int corr_enc_norm_finalize(const void *stats, int B, int C, int Ho, int Wo, float eps, float *scale,
                           float *shift, void *stream);
int corr_enc_join(const float *y, const float *scale, const float *shift, int norm_per_batch,
                  const float *skip, int B, int C, int H, int W, float *out, void *stream);

/*
 * The encoders around their residual stages (model/extractor.py:137-189: BasicEncoder's 7x7 stem,
 * the strided blocks' 1x1 projections, the 1x1 head), inference only.  With them
 *   y0 = stem(x);  layer1[0] reads relu(norm1(y0)) by norm on load and joins it as its skip;
 *   a strided block's skip is norm3(pw(x)) [stride 2], applied by its join;  out = pw(layer3) [stride 1]
 * so that no normalised map is stored.
 *
 * corr_enc_stem_forward: the 7x7 convolution at stride 2 with zero padding 3, bias, no ReLU:
 *   out[b][o][y][x] = bias[o] + sum_c sum_ky sum_kx w[o][c][ky][kx] * in[b][c][2 y + ky - 3][2 x + kx - 3]
 * in is [B][cin][H][W] (exactly cin planes are read), out [B][cout][Ho][Wo] with Ho = (H - 1) / 2
 * + 1, Wo = (W - 1) / 2 + 1; odd sizes and sizes below 7 are allowed.  w is a contiguous Conv2d
 * weight [cout][cin][7][7], split once per weight version by corr_enc_stem_pack_weights into a
 * corr_enc_stem_weights_bytes(cout, cin) buffer (16-B aligned, opaque; 0 for unsupported sizes).
 * K order: tap-major, tap = 7 ky + kx ascending, the channels of a tap ascending and padded with
 * zeros to 16; a K step of 32 is two taps, 25 steps.
 *
 * corr_enc_pw_forward: the 1x1 convolution at stride s = 1 or 2, no padding, bias, no ReLU:
 *   out[b][o][y][x] = bias[o] + sum_c w[o][c] * in[b][c][s y][s x]
 * with Ho = (H - 1) / s + 1, Wo = (W - 1) / s + 1.  At stride 2 only the even rows and columns of
 * in are read.  w is a contiguous [cout][cin] (a [cout][cin][1][1] Conv2d weight), split by
 * corr_enc_pw_pack_weights into a corr_enc_pw_weights_bytes(cout, cin) buffer (16-B aligned,
 * opaque; 0 for unsupported sizes).  K order: ascending 32-channel steps.
 *
 * Both: bias is [cout] or NULL; the packs hold the rows padded with zeros to a multiple of 64,
 * padding rows are never stored.  Arithmetic: corr_conv_forward's (the bf16 MFMA with the exact
 * three-piece split, six products per fp32 product in its order, fp32 accumulation in the K order
 * above, then + bias; each fp32 op rounded once; deterministic; non-finite inputs are NOT
 * parity-checked).  stats (may be NULL) is corr_enc_conv_forward's, layout and meaning:
 * [B][cout][ceil(Ho/4) * ceil(Wo/16)][2] of (sum, M2 about the tile's own mean), at least
 * corr_enc_stats_bytes(B, cout, Ho, Wo) bytes, for corr_enc_norm_finalize.  out's byte range must
 * not overlap in's.
 *
 * corr_enc_join_affine: corr_enc_join with an affine (and optionally a ReLU) on the skip,
 *   out = max(s(skip) + max(y * scale[k] + shift[k], 0), 0),   s(v) = v * skip_scale[k'] + skip_shift[k'],
 * s(v) = max(., 0) of that when skip_relu = 1, s(v) = v (then the ReLU, if asked for) when
 * skip_scale and skip_shift are both NULL.  k = b C + c (norm_per_batch = 1) or c (0), k' likewise
 * by skip_per_batch.  Each fp32 op is rounded once.  out may be y (or skip) itself.
 *
 * Sizes: stem 1 <= cin <= 16 (a larger cin: CORR_EUNSUPPORTED), pointwise cin a multiple of 32 in
 * 32 .. 1024, both 1 <= cout <= 1024, pointwise stride 1 or 2; otherwise CORR_EUNSUPPORTED.
 * CORR_EINVAL: a NULL in, packed, out (pack: w, packed; join: y, scale, shift, skip, out); stem
 * cin < 1; stats with stats_bytes too small; packed not 16-byte aligned; B, C, H or W < 1 or
 * B*H*W >= 2^31 (join: B*C >= 2^31); out overlapping in; exactly one of skip_scale / skip_shift
 * NULL; norm_per_batch, skip_per_batch or skip_relu not 0 or 1.  Every refusal comes before any
 * HIP call.  No workspace, no allocation, no synchronisation; everything goes on `stream` and can
 * be captured into a graph.
 */
size_t corr_enc_stem_weights_bytes(int cout, int cin);
int corr_enc_stem_pack_weights(const float *w, int cout, int cin, void *packed, void *stream);
int corr_enc_stem_forward(const float *in, int cin, int B, int H, int W, const void *packed, const float *bias,
                          int cout, float *out, void *stats, size_t stats_bytes, void *stream);
size_t corr_enc_pw_weights_bytes(int cout, int cin);
int corr_enc_pw_pack_weights(const float *w, int cout, int cin, void *packed, void *stream);
int corr_enc_pw_forward(const float *in, int cin, int B, int H, int W, int stride, const void *packed,
                        const float *bias, int cout, float *out, void *stats, size_t stats_bytes, void *stream);
int corr_enc_join_affine(const float *y, const float *scale, const float *shift, int norm_per_batch,
                         const float *skip, const float *skip_scale, const float *skip_shift, int skip_per_batch,
                         int skip_relu, int B, int C, int H, int W, float *out, void *stream);

/*
 * The update block's mask head fused with the convex upsampling (model/update.py:99-107: the
 * 256 -> 576 1x1 convolution mask[2] and its 0.25; model/eraft.py:75-86 upsample_flow), inference
 * only: one launch from the hidden activations relu(mask[0](net)) and the 1/8-resolution flow to
 * the full-resolution prediction.  The [B][576][H][W] mask is never stored.
 *   logit[k][i][j] = mask_scale * (bias[64k + 8i + j] + sum_c w[64k + 8i + j][c] * hidden[n][hidden_offset + c][y][x])
 *   p = softmax of logit over the 9 taps k (max-subtracted, summed in tap order k = 0..8)
 *   out[n][ch][8y + i][8x + j] = sum_k p[k] * 8 * flow[n][ch][y + k/3 - 1][x + k%3 - 1]
 * for c < 256, i, j < 8, ch < 2; a flow neighbour outside the map counts as 0.  The softmax and
 * the combination are corr_convex_upsample's, op for op.
 * Input: hidden is a [B][hidden_channels][H][W] tensor of which channels hidden_offset ..
 * hidden_offset + 255 are read in place (the mask half of the update block's stacked heads
 * buffer needs no copy); flow is [B][2][H][W]; out is [B][2][8H][8W], every float of it written
 * and nothing else; out's byte range must not overlap hidden's or flow's.
 * Weights: w is the contiguous Conv2d weight [576][256] (a [576][256][1][1] tensor).  It is split
 * once per weight version by corr_mask_upsample_pack_weights into a
 * corr_mask_upsample_weights_bytes() buffer (16-B aligned, opaque).  bias is [576].  All tensors
 * fp32, 4-byte aligned (a 16-byte aligned out takes 16-byte stores).
 * Arithmetic: the logits are an implicit GEMM with K = 256 on the bf16 MFMA with
 * CORR_BUILD_BF16X6's exact three-piece split (six products per fp32 product, no scales: no
 * narrower than fp32), fp32 accumulation in ascending 32-channel steps, then + bias and
 * * mask_scale, each fp32 op rounded once; deterministic.  Non-finite inputs are NOT
 * parity-checked.
 * CORR_EINVAL: a NULL hidden, flow, packed, bias or out; B, H or W < 1 or B*H*W >= 2^31;
 * hidden_offset < 0 or hidden_offset + 256 > hidden_channels; packed not 16-byte aligned; a
 * mask_scale that is not finite; out overlapping hidden or flow.  Every refusal comes before any
 * HIP call.  No workspace, no allocation, no synchronisation; the launch goes on `stream` and can
 * be captured into a graph.
 */
size_t corr_mask_upsample_weights_bytes(void);
int corr_mask_upsample_pack_weights(const float *w, void *packed, void *stream);
int corr_mask_upsample_forward(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                               const void *packed, const float *bias, float mask_scale, int B, int H, int W,
                               float *out, void *stream);

/*
 * The update block's tail (model/update.py:63-82 BasicMotionEncoder.convf1, :20-31 FlowHead.conv2,
 * and the coordinate update of model/eraft.py's refinement loop), inference only.
 *
 * corr_flow_enc_forward: the 7x7 convolution of the 2-channel flow at stride 1 with zero padding
 * 3, bias and an optional ReLU (relu = 1), written into a channel window of `out`:
 *   out[b][out_offset + o][y][x] = act(bias[o] + sum_c sum_ky sum_kx w[o][c][ky][kx] * flow[b][c][y + ky - 3][x + kx - 3])
 * flow is [B][2][H][W]; out is [B][out_channels][H][W], of which exactly channels out_offset ..
 * out_offset + cout - 1 are written.  Maps smaller than the window (1 x 1, 3 x 4) are allowed.
 * Pass-through: with flow_copy not NULL the launch also writes flow[b][c], bit for bit, into
 * channels copy_offset, copy_offset + 1 of the [B][copy_channels][H][W] tensor flow_copy (the flow
 * channels of the GRU input), and nothing else of it.  out and flow_copy must not overlap flow;
 * they may be one tensor (same pointer, same channel count) written through disjoint channel
 * windows, and must not overlap each other in any other way.
 * Weights: w is a contiguous Conv2d weight [cout][2][7][7], split once per weight version by
 * corr_flow_enc_pack_weights into a corr_flow_enc_weights_bytes(cout) buffer (16-B aligned,
 * opaque; 0 for unsupported sizes).  The pack holds the rows padded with zeros to a multiple of
 * 64; padding rows are never stored.  bias is [cout], or NULL for no bias.
 * Arithmetic: corr_conv_forward's (the bf16 MFMA with the exact three-piece split, six products
 * per fp32 product in its order, no scales: no narrower than fp32).  K order: tap-major, tap =
 * 7 ky + kx ascending, the two channels of a tap adjacent (k = 2 tap + c), K = 98 padded with zero
 * weights to 128: four K steps of 16 taps; then + bias, then the ReLU, each fp32 op rounded once.
 * Deterministic.  Non-finite inputs are NOT parity-checked.
 * Sizes: 1 <= cout <= 1024, otherwise CORR_EUNSUPPORTED (and a size of 0); any B, H, W >= 1 with
 * B*H*W < 2^31.  CORR_EINVAL: a NULL flow, packed or out (pack: w, packed); relu not 0 or 1;
 * out_offset < 0 or out_offset + cout > out_channels; with flow_copy, copy_offset < 0 or
 * copy_offset + 2 > copy_channels; packed not 16-byte aligned; B, H or W < 1 or B*H*W >= 2^31;
 * out or flow_copy overlapping flow, or each other as described above.
 *
 * corr_flow_head_forward: the 3x3 convolution from 256 to 2 channels at stride 1 with zero
 * padding 1, bias, no ReLU, and the coordinate update:
 *   delta[b][o][y][x] = bias[o] + sum_c sum_ky sum_kx w[o][c][ky][kx] * hidden[b][hidden_offset + c][y + ky - 1][x + kx - 1]
 *   coords_out = coords_in + delta            (when coords_in is not NULL)
 *   flow_out   = coords_out - coords0         (when coords0 is not NULL as well)
 * hidden is a [B][hidden_channels][H][W] tensor of which channels hidden_offset .. hidden_offset +
 * 255 are read in place (corr_mask_upsample_forward's convention: the flow half of the update
 * block's stacked heads buffer needs no copy); bias is [2]; coords_in, coords0, delta, coords_out
 * and flow_out are [B][2][H][W].  With coords_in NULL only delta is written (coords_out and
 * flow_out are ignored); with coords0 NULL flow_out is ignored.  The two updates are one fp32
 * operation each, rounded once, on the delta this launch stores.  No output may overlap hidden,
 * coords_in, coords0 or another output: a workgroup reads its neighbours' pixels, so there is no
 * in-place update (callers keep two coordinate buffers).
 * Weights: w is a contiguous Conv2d weight [2][256][3][3], split once per weight version by
 * corr_flow_head_pack_weights into a corr_flow_head_weights_bytes() buffer (16-B aligned, opaque).
 * Arithmetic and K order (NOT corr_conv_forward's): per pixel and tap = 3 ky + kx the product
 *   P[o][tap] = sum_c w[o][c][tap] * hidden[c]
 * is accumulated over ascending 32-channel steps on the bf16 MFMA with the exact three-piece split
 * (six products per fp32 product in corr_conv_forward's order); a pixel outside the map has P = 0.
 * Then delta = ((..(P[o][0] + P[o][1]) + ..) + P[o][8]) + bias[o], each P taken at its tap's
 * neighbour, taps ascending, each fp32 op rounded once.  Deterministic.  Non-finite inputs are
 * NOT parity-checked.
 * Sizes: any B, H, W >= 1 with B*H*W < 2^31.  CORR_EINVAL: a NULL hidden, packed, bias or delta
 * (pack: w, packed); coords0 given without coords_in; coords_out NULL with coords_in given;
 * flow_out NULL with coords0 given; hidden_offset < 0 or hidden_offset + 256 > hidden_channels;
 * packed not 16-byte aligned; B, H or W < 1 or B*H*W >= 2^31; an output overlapping an input or
 * another output.
 *
 * Both: all tensors fp32, 4-byte aligned.  Every refusal comes before any HIP call.  No workspace,
 * no allocation, no synchronisation; each is one launch on `stream` and can be captured into a
 * graph.
 */
size_t corr_flow_enc_weights_bytes(int cout);
int corr_flow_enc_pack_weights(const float *w, int cout, void *packed, void *stream);
int corr_flow_enc_forward(const float *flow, int B, int H, int W, const void *packed, const float *bias, int cout,
                          int relu, float *out, int out_channels, int out_offset, float *flow_copy,
                          int copy_channels, int copy_offset, void *stream);
size_t corr_flow_head_weights_bytes(void);
int corr_flow_head_pack_weights(const float *w, void *packed, void *stream);
int corr_flow_head_forward(const float *hidden, int hidden_channels, int hidden_offset, int B, int H, int W,
                           const void *packed, const float *bias, const float *coords_in, const float *coords0,
                           float *delta, float *coords_out, float *flow_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CORR_MI355X_H */
