// corr_api.cpp — the extern "C" boundary of libcorr_mi355x.so (declared in
// include/corr_mi355x.h).  Validates arguments, records thread-local errors and forwards to
// the gfx950 launchers.  No allocation and no synchronisation.  Global state: the thread-local
// error message, and per-kernel per-device "dynamic-LDS limit raised" bits (atomic, idempotent;
// ensure_lds_limit in corr_build_common.h) — re-entrant across threads, streams and devices.
//
// The reference-shaped entry points (corr_build, corr_lookup, ...) are the row-slab
// variants (corr_*_rows) with the slab = every query pixel (NQ = H*W).
#include <cstdarg>
#include <cstdint>
#include <cstdio>

#include "../../include/corr_mi355x_build_prec.h"
#include "../../include/corr_mi355x_enc_prec.h"
#include "../../include/corr_mi355x_pw_prec.h"
#include "../../include/corr_mi355x_train.h"
#include "../../include/corr_mi355x_train_head.h"
#include "corr_common.h"

namespace corr {

static thread_local char g_err[512] = "";

int fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int hip_status(hipError_t e, const char *what) {
    if (e == hipSuccess) return CORR_OK;
    return fail(CORR_EHIP, "%s: %s", what, hipGetErrorString(e));
}

static int check_dims(const char *fn, int B, int NQ, int H, int W, int levels) {
    if (B < 1 || H < 1 || W < 1)
        return fail(CORR_EINVAL, "%s: B, H, W must be >= 1 (got %d, %d, %d)", fn, B, H, W);
    if (NQ < 1 || NQ > H * (long long)W)
        return fail(CORR_EINVAL, "%s: NQ must be in [1, H*W] (got %d)", fn, NQ);
    if (levels < 1 || levels > CORR_MAX_LEVELS)
        return fail(CORR_EINVAL, "%s: levels must be in [1, %d] (got %d)", fn, CORR_MAX_LEVELS, levels);
    // avg_pool2d(2, 2) on a 1-pixel dimension raises in the reference (corr.py:26)
    if ((H >> (levels - 1)) < 1 || (W >> (levels - 1)) < 1)
        return fail(CORR_EINVAL, "%s: %dx%d is too small for %d pyramid levels", fn, H, W, levels);
    // the lookup's neighbourhood anchors assume |coordinate floors| of in-map taps < 2^20
    if (H > (1 << 20) || W > (1 << 20))
        return fail(CORR_EINVAL, "%s: H and W must be <= 2^20", fn);
    const long long N = (long long)H * W;
    if (N > (1LL << 30) || (long long)B * NQ > (1LL << 31) - 1)
        return fail(CORR_EINVAL, "%s: B*H*W too large", fn);
    return CORR_OK;
}

static int check_ptr(const char *fn, const void *p, const char *name) {
    if (!p) return fail(CORR_EINVAL, "%s: %s is NULL", fn, name);
    if ((uintptr_t)p % 4) return fail(CORR_EINVAL, "%s: %s is not 4-byte aligned", fn, name);
    return CORR_OK;
}

template <class P>
static int check_levels(const char *fn, P *const *src, int levels, const char *name, P **dst) {
    if (!src) return fail(CORR_EINVAL, "%s: %s is NULL", fn, name);
    for (int l = 0; l < levels; ++l) {
        int rc = check_ptr(fn, src[l], name);
        if (rc) return rc;
        dst[l] = src[l];
    }
    return CORR_OK;
}

// Value pyramids (tiled, corr_common.h): 16-B tile rows, so 16-B aligned level bases.
template <class P>
static int check_pyramid(const char *fn, P *const *src, int levels, const char *name, P **dst) {
    int rc = check_levels(fn, src, levels, name, dst);
    if (rc) return rc;
    for (int l = 0; l < levels; ++l)
        if ((uintptr_t)src[l] % 16) return fail(CORR_EINVAL, "%s: %s[%d] is not 16-byte aligned", fn, name, l);
    return CORR_OK;
}

static int check_radius(const char *fn, int radius) {
    if (radius < 0 || radius > CORR_MAX_RADIUS)
        return fail(CORR_EINVAL, "%s: radius must be in [0, %d] (got %d)", fn, CORR_MAX_RADIUS, radius);
    return CORR_OK;
}

// Sizes the on-demand calls share: check_dims plus D and the operands' total size.
static int check_ondemand(const char *fn, int B, int D, int H, int W, int levels) {
    int rc = check_dims(fn, B, 1, H, W, levels);
    if (rc) return rc;
    if (D < 1) return fail(CORR_EINVAL, "%s: D must be >= 1 (got %d)", fn, D);
    // the launch grids are sized for feature maps of up to 2^37 (padded) floats each
    if (D > (1 << 20) || (long double)B * H * W * ((D + 3) & ~3) > (long double)(1LL << 37))
        return fail(CORR_EINVAL, "%s: B*H*W*D too large", fn);
    return CORR_OK;
}

}  // namespace corr

using namespace corr;

extern "C" {

int corr_version(void) { return 202; }

const char *corr_last_error(void) { return g_err; }

size_t corr_map_floats(int Hl, int Wl) {
    if (Hl < 1 || Wl < 1) return 0;
    return map_floats(Hl, Wl);
}

int corr_pyramid_export(const float *const *pyr, int BN, int H, int W, int levels, float *const *out, void *stream) {
    static const char *fn = "corr_pyramid_export";
    g_err[0] = 0;
    int rc = check_dims(fn, 1, 1, H, W, levels);
    if (rc) return rc;
    if (BN < 1) return fail(CORR_EINVAL, "%s: BN must be >= 1", fn);
    ConstLevelPtrs src{};
    LevelPtrs dst{};
    if ((rc = check_pyramid(fn, pyr, levels, "pyr", src.p)) || (rc = check_levels(fn, out, levels, "out", dst.p)))
        return rc;
    return hip_status(launch_pyramid_export(src, BN, H, W, levels, dst, (hipStream_t)stream), fn);
}

int corr_pyramid_import(const float *const *src, int BN, int H, int W, int levels, float *const *pyr, void *stream) {
    static const char *fn = "corr_pyramid_import";
    g_err[0] = 0;
    int rc = check_dims(fn, 1, 1, H, W, levels);
    if (rc) return rc;
    if (BN < 1) return fail(CORR_EINVAL, "%s: BN must be >= 1", fn);
    ConstLevelPtrs s{};
    LevelPtrs dst{};
    if ((rc = check_levels(fn, src, levels, "src", s.p)) || (rc = check_pyramid(fn, pyr, levels, "pyr", dst.p)))
        return rc;
    return hip_status(launch_pyramid_import(s, BN, H, W, levels, dst, (hipStream_t)stream), fn);
}

int corr_build_rows(const float *fmap1_rows, int NQ, const float *fmap2, int B, int D, int H,
                    int W, int levels, float *const *pyr, void *stream) {
    static const char *fn = "corr_build";
    g_err[0] = 0;
    int rc = check_dims(fn, B, NQ, H, W, levels);
    if (rc) return rc;
    if (D < 1) return fail(CORR_EINVAL, "%s: D must be >= 1 (got %d)", fn, D);
    if ((rc = check_ptr(fn, fmap1_rows, "fmap1")) || (rc = check_ptr(fn, fmap2, "fmap2"))) return rc;
    LevelPtrs lp{};
    if ((rc = check_pyramid(fn, pyr, levels, "pyr", lp.p))) return rc;
    return hip_status(launch_build(fmap1_rows, NQ, fmap2, B, D, H, W, levels, lp, (hipStream_t)stream), fn);
}

size_t corr_build_workspace(int algo, int B, int D, int NQ, int H, int W) {
    if (B < 1 || D < 1 || NQ < 1 || H < 1 || W < 1) return 0;
    if (algo == CORR_BUILD_F16X3)
        return build_split_supported(D) ? build_split_workspace(B, D, NQ, H, W) : (size_t)-1;
    if (algo == CORR_BUILD_BF16X6) return build_bf16_workspace(B, D, NQ, H, W);
    if (algo == CORR_BUILD_FP32) return 0;
    return (size_t)-1;
}

// CORR_PREC_* of the build (corr_mi355x_build_prec.h): an unknown mode is refused before every
// other check, a reduced one runs on CORR_BUILD_BF16X6 only (phase flags allowed).
static int check_build_precision(const char *fn, int algo, int precision) {
    if (!precision_supported(precision))
        return fail(CORR_EINVAL, "%s: precision must be CORR_PREC_BF16X6 (0), _BF16X3 (1) or _BF16 (2) (got %d)", fn,
                    precision);
    if (precision != CORR_PREC_BF16X6 && (algo & ~(CORR_BUILD_ONLY_PACK | CORR_BUILD_ONLY_MFMA)) != CORR_BUILD_BF16X6)
        return fail(CORR_EUNSUPPORTED, "%s: a reduced precision needs CORR_BUILD_BF16X6 (got algorithm %d)", fn, algo);
    return CORR_OK;
}

static int build_ex(const char *fn, int algo, const float *fmap1_rows, int NQ, const float *fmap2, int B, int D, int H,
                    int W, int levels, float *const *pyr, void *workspace, size_t workspace_bytes, void *stream,
                    int precision) {
    g_err[0] = 0;
    int rc = check_build_precision(fn, algo, precision);
    if (rc) return rc;
    if (algo == CORR_BUILD_FP32) return corr_build_rows(fmap1_rows, NQ, fmap2, B, D, H, W, levels, pyr, stream);
    const int phase = algo & (CORR_BUILD_ONLY_PACK | CORR_BUILD_ONLY_MFMA);
    algo &= ~(CORR_BUILD_ONLY_PACK | CORR_BUILD_ONLY_MFMA);
    if ((algo != CORR_BUILD_F16X3 && algo != CORR_BUILD_BF16X6) ||
        phase == (CORR_BUILD_ONLY_PACK | CORR_BUILD_ONLY_MFMA))
        return fail(CORR_EINVAL, "%s: unknown algorithm %d", fn, algo | phase);
    const bool bf = algo == CORR_BUILD_BF16X6;
    if ((rc = check_dims(fn, B, NQ, H, W, levels))) return rc;
    if (D < 1) return fail(CORR_EINVAL, "%s: D must be >= 1 (got %d)", fn, D);
    if (!bf && !build_split_supported(D))
        return fail(CORR_EUNSUPPORTED, "%s: D = %d is too large for CORR_BUILD_F16X3", fn, D);
    if ((rc = check_ptr(fn, fmap1_rows, "fmap1")) || (rc = check_ptr(fn, fmap2, "fmap2"))) return rc;
    if ((uintptr_t)workspace % 256) return fail(CORR_EINVAL, "%s: workspace is not 256-byte aligned", fn);
    const size_t need = bf ? build_bf16_workspace(B, D, NQ, H, W) : build_split_workspace(B, D, NQ, H, W);
    if (workspace_bytes < need || !workspace)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    LevelPtrs lp{};
    if ((rc = check_pyramid(fn, pyr, levels, "pyr", lp.p))) return rc;
    const int part = phase == CORR_BUILD_ONLY_PACK ? 1 : phase == CORR_BUILD_ONLY_MFMA ? 2 : 0;
    if (bf)
        return hip_status(
            launch_build_bf16(fmap1_rows, NQ, fmap2, B, D, H, W, levels, lp, workspace, (hipStream_t)stream, part, precision),
            fn);
    return hip_status(launch_build_split(fmap1_rows, NQ, fmap2, B, D, H, W, levels, lp, workspace, (hipStream_t)stream, part),
                      fn);
}

int corr_build_ex(int algo, const float *fmap1_rows, int NQ, const float *fmap2, int B, int D,
                  int H, int W, int levels, float *const *pyr, void *workspace,
                  size_t workspace_bytes, void *stream) {
    return build_ex("corr_build_ex", algo, fmap1_rows, NQ, fmap2, B, D, H, W, levels, pyr, workspace, workspace_bytes,
                    stream, CORR_PREC_BF16X6);
}

int corr_build_ex_prec(int algo, const float *fmap1_rows, int NQ, const float *fmap2, int B, int D, int H, int W,
                       int levels, float *const *pyr, void *workspace, size_t workspace_bytes, int precision,
                       void *stream) {
    return build_ex("corr_build_ex_prec", algo, fmap1_rows, NQ, fmap2, B, D, H, W, levels, pyr, workspace,
                    workspace_bytes, stream, precision);
}

static int build_region(const char *fn, int algo, const float *fmap1_rows, int NQ, const float *fmap2_rows, int y0,
                        int y1, int B, int D, int H, int W, int levels, float *const *pyr, void *workspace,
                        size_t workspace_bytes, int flags, void *stream, int precision) {
    g_err[0] = 0;
    if (!precision_supported(precision))
        return fail(CORR_EINVAL, "%s: precision must be CORR_PREC_BF16X6 (0), _BF16X3 (1) or _BF16 (2) (got %d)", fn,
                    precision);
    if (algo != CORR_BUILD_BF16X6)
        return fail(CORR_EUNSUPPORTED, "%s: only CORR_BUILD_BF16X6 builds by target region (got %d)", fn, algo);
    int rc = check_dims(fn, B, NQ, H, W, levels);
    if (rc) return rc;
    if (D < 1) return fail(CORR_EINVAL, "%s: D must be >= 1 (got %d)", fn, D);
    if (levels > 4) return fail(CORR_EUNSUPPORTED, "%s: levels <= 4 (got %d)", fn, levels);
    if (y0 < 0 || y0 >= y1 || y1 > H || y0 % 8 || (y1 % 8 && y1 != H))
        return fail(CORR_EINVAL, "%s: need 0 <= y0 < y1 <= H, y0 %% 8 == 0, y1 %% 8 == 0 or y1 == H (got %d, %d, H %d)",
                    fn, y0, y1, H);
    if ((rc = check_ptr(fn, fmap1_rows, "fmap1")) || (rc = check_ptr(fn, fmap2_rows, "fmap2_rows"))) return rc;
    if ((uintptr_t)workspace % 256) return fail(CORR_EINVAL, "%s: workspace is not 256-byte aligned", fn);
    const size_t need = build_bf16_workspace(B, D, NQ, H, W);
    if (workspace_bytes < need || !workspace)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    LevelPtrs lp{};
    if ((rc = check_pyramid(fn, pyr, levels, "pyr", lp.p))) return rc;
    return hip_status(launch_build_bf16_region(fmap1_rows, NQ, fmap2_rows, y0, y1, B, D, H, W, levels, lp, workspace,
                                               (flags & CORR_REGION_PACK_QUERIES) != 0, (hipStream_t)stream, precision),
                      fn);
}

int corr_build_region(int algo, const float *fmap1_rows, int NQ, const float *fmap2_rows, int y0, int y1, int B,
                      int D, int H, int W, int levels, float *const *pyr, void *workspace, size_t workspace_bytes,
                      int flags, void *stream) {
    return build_region("corr_build_region", algo, fmap1_rows, NQ, fmap2_rows, y0, y1, B, D, H, W, levels, pyr,
                        workspace, workspace_bytes, flags, stream, CORR_PREC_BF16X6);
}

int corr_build_region_prec(int algo, const float *fmap1_rows, int NQ, const float *fmap2_rows, int y0, int y1, int B,
                           int D, int H, int W, int levels, float *const *pyr, void *workspace,
                           size_t workspace_bytes, int flags, int precision, void *stream) {
    return build_region("corr_build_region_prec", algo, fmap1_rows, NQ, fmap2_rows, y0, y1, B, D, H, W, levels, pyr,
                        workspace, workspace_bytes, flags, stream, precision);
}

int corr_build(const float *fmap1, const float *fmap2, int B, int D, int H, int W, int levels,
               float *const *pyr, void *stream) {
    return corr_build_rows(fmap1, H * W, fmap2, B, D, H, W, levels, pyr, stream);
}

int corr_lookup_rows(const float *const *pyr, const float *coords_rows, int B, int NQ, int H,
                     int W, int levels, int radius, float *out_rows, void *stream) {
    static const char *fn = "corr_lookup";
    g_err[0] = 0;
    int rc = check_dims(fn, B, NQ, H, W, levels);
    if (rc || (rc = check_radius(fn, radius))) return rc;
    if ((rc = check_ptr(fn, coords_rows, "coords")) || (rc = check_ptr(fn, out_rows, "out"))) return rc;
    ConstLevelPtrs lp{};
    if ((rc = check_pyramid(fn, pyr, levels, "pyr", lp.p))) return rc;
    return hip_status(launch_lookup(lp, coords_rows, B, NQ, H, W, levels, radius, out_rows, (hipStream_t)stream),
                      fn);
}

int corr_lookup(const float *const *pyr, const float *coords, int B, int H, int W, int levels,
                int radius, float *out, void *stream) {
    return corr_lookup_rows(pyr, coords, B, H * W, H, W, levels, radius, out, stream);
}

int corr_lookup_bwd_rows(const float *coords_rows, const float *grad_out_rows, int B, int NQ,
                         int H, int W, int levels, int radius, float *const *grad_pyr,
                         void *stream) {
    static const char *fn = "corr_lookup_bwd";
    g_err[0] = 0;
    int rc = check_dims(fn, B, NQ, H, W, levels);
    if (rc || (rc = check_radius(fn, radius))) return rc;
    if ((rc = check_ptr(fn, coords_rows, "coords")) || (rc = check_ptr(fn, grad_out_rows, "grad_out")))
        return rc;
    LevelPtrs lp{};
    if ((rc = check_levels(fn, grad_pyr, levels, "grad_pyr", lp.p))) return rc;
    return hip_status(
        launch_lookup_bwd(coords_rows, grad_out_rows, B, NQ, H, W, levels, radius, lp, (hipStream_t)stream), fn);
}

int corr_lookup_bwd(const float *coords, const float *grad_out, int B, int H, int W, int levels,
                    int radius, float *const *grad_pyr, void *stream) {
    return corr_lookup_bwd_rows(coords, grad_out, B, H * W, H, W, levels, radius, grad_pyr, stream);
}

int corr_pool_bwd(float *const *grad_pyr, int BN, int H, int W, int levels, void *stream) {
    static const char *fn = "corr_pool_bwd";
    g_err[0] = 0;
    int rc = check_dims(fn, 1, 1, H, W, levels);
    if (rc) return rc;
    if (BN < 1) return fail(CORR_EINVAL, "%s: BN must be >= 1", fn);
    LevelPtrs lp{};
    if ((rc = check_levels(fn, grad_pyr, levels, "grad_pyr", lp.p))) return rc;
    return hip_status(launch_pool_bwd(lp, BN, H, W, levels, (hipStream_t)stream), fn);
}

size_t corr_build_bwd_rows_workspace(int B, int D, int NQ, int H, int W) {
    if (B < 1 || D < 1 || NQ < 1 || H < 1 || W < 1) return 0;
    return build_bwd_workspace(B, D, NQ, H, W);
}

size_t corr_build_bwd_workspace(int B, int D, int H, int W) {
    return corr_build_bwd_rows_workspace(B, D, H * W, H, W);
}

int corr_build_bwd_rows(const float *grad_c, const float *fmap1_rows, int NQ, const float *fmap2,
                        int B, int D, int H, int W, float *dfmap1_rows, float *dfmap2,
                        void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_build_bwd";
    g_err[0] = 0;
    int rc = check_dims(fn, B, NQ, H, W, 1);
    if (rc) return rc;
    if (D < 1) return fail(CORR_EINVAL, "%s: D must be >= 1 (got %d)", fn, D);
    if ((rc = check_ptr(fn, grad_c, "grad_c")) || (rc = check_ptr(fn, fmap1_rows, "fmap1")) ||
        (rc = check_ptr(fn, fmap2, "fmap2")) || (rc = check_ptr(fn, dfmap1_rows, "dfmap1")) ||
        (rc = check_ptr(fn, dfmap2, "dfmap2")))
        return rc;
    const size_t need = build_bwd_workspace(B, D, NQ, H, W);
    if (workspace_bytes < need || (need && !workspace))
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    return hip_status(launch_build_bwd(grad_c, fmap1_rows, NQ, fmap2, B, D, H, W, dfmap1_rows, dfmap2,
                                       (float *)workspace, (hipStream_t)stream),
                      fn);
}

size_t corr_build_bwd_ex_workspace(int algo, int B, int D, int NQ, int H, int W) {
    if (B < 1 || D < 1 || NQ < 1 || H < 1 || W < 1) return 0;
    if (algo == CORR_BUILD_FP32) return build_bwd_workspace(B, D, NQ, H, W);
    if (algo == CORR_BUILD_F16X3 || algo == CORR_BUILD_BF16X6) return build_bwd_split_workspace(B, D, NQ, H, W);
    return (size_t)-1;
}

int corr_build_bwd_ex(int algo, const float *grad_c, const float *fmap1_rows, int NQ, const float *fmap2, int B,
                      int D, int H, int W, float *dfmap1_rows, float *dfmap2, void *workspace,
                      size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_build_bwd_ex";
    if (algo == CORR_BUILD_FP32)
        return corr_build_bwd_rows(grad_c, fmap1_rows, NQ, fmap2, B, D, H, W, dfmap1_rows, dfmap2, workspace,
                                   workspace_bytes, stream);
    g_err[0] = 0;
    if (algo != CORR_BUILD_F16X3 && algo != CORR_BUILD_BF16X6)
        return fail(CORR_EUNSUPPORTED, "%s: unknown algorithm %d", fn, algo);
    int rc = check_dims(fn, B, NQ, H, W, 1);
    if (rc) return rc;
    if (D < 1) return fail(CORR_EINVAL, "%s: D must be >= 1 (got %d)", fn, D);
    if ((rc = check_ptr(fn, grad_c, "grad_c")) || (rc = check_ptr(fn, fmap1_rows, "fmap1")) ||
        (rc = check_ptr(fn, fmap2, "fmap2")) || (rc = check_ptr(fn, dfmap1_rows, "dfmap1")) ||
        (rc = check_ptr(fn, dfmap2, "dfmap2")))
        return rc;
    const size_t need = build_bwd_split_workspace(B, D, NQ, H, W);
    if (workspace_bytes < need || !workspace)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    return hip_status(launch_build_bwd_split(grad_c, fmap1_rows, NQ, fmap2, B, D, H, W, dfmap1_rows, dfmap2,
                                             workspace, (hipStream_t)stream, algo == CORR_BUILD_BF16X6),
                      fn);
}

int corr_lookup_bwd_multi(const float *const *coords_rows, const float *const *grad_out_rows, int T, int B, int NQ,
                          int H, int W, int levels, int radius, float *const *grad_pyr, void *stream) {
    static const char *fn = "corr_lookup_bwd_multi";
    g_err[0] = 0;
    int rc = check_dims(fn, B, NQ, H, W, levels);
    if (rc || (rc = check_radius(fn, radius))) return rc;
    if (T < 0) return fail(CORR_EINVAL, "%s: T must be >= 0 (got %d)", fn, T);
    if (T > 0 && (!coords_rows || !grad_out_rows)) return fail(CORR_EINVAL, "%s: coords / grad_out arrays are NULL", fn);
    for (int t = 0; t < T; ++t)
        if ((rc = check_ptr(fn, coords_rows[t], "coords[t]")) || (rc = check_ptr(fn, grad_out_rows[t], "grad_out[t]")))
            return rc;
    LevelPtrs lp{};
    if ((rc = check_levels(fn, grad_pyr, levels, "grad_pyr", lp.p))) return rc;
    return hip_status(launch_lookup_bwd_multi(coords_rows, grad_out_rows, T, B, NQ, H, W, levels, radius, lp,
                                              (hipStream_t)stream),
                      fn);
}

int corr_pool_fold(float *const *grad_pyr, int B, int NQ, int H, int W, int levels, void *stream) {
    static const char *fn = "corr_pool_fold";
    g_err[0] = 0;
    int rc = check_dims(fn, B, NQ, H, W, levels);
    if (rc) return rc;
    LevelPtrs lp{};
    if ((rc = check_levels(fn, grad_pyr, levels, "grad_pyr", lp.p))) return rc;
    return hip_status(launch_pool_fold(lp, B, NQ, H, W, levels, nullptr, 1, (hipStream_t)stream), fn);
}

size_t corr_backward_workspace(int algo, int B, int D, int NQ, int H, int W, int radius) {
    if (B < 1 || D < 1 || NQ < 1 || H < 1 || W < 1 || radius < 0) return 0;
    return backward_workspace(algo & ~CORR_BACKWARD_EXACT_FOLD, B, D, NQ, H, W, radius);
}

int corr_backward(int algo, const float *const *coords_rows, const float *const *grad_out_rows, int T,
                  const float *fmap1_rows, int NQ, const float *fmap2, int B, int D, int H, int W, int levels,
                  int radius, float *const *grad_pyr, float *dfmap1_rows, float *dfmap2, void *workspace,
                  size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_backward";
    g_err[0] = 0;
    const int base = algo & ~CORR_BACKWARD_EXACT_FOLD;
    if (base != CORR_BUILD_FP32 && base != CORR_BUILD_F16X3 && base != CORR_BUILD_BF16X6)
        return fail(CORR_EUNSUPPORTED, "%s: unknown algorithm %d", fn, algo);
    int rc = check_dims(fn, B, NQ, H, W, levels);
    if (rc || (rc = check_radius(fn, radius))) return rc;
    if (D < 1) return fail(CORR_EINVAL, "%s: D must be >= 1 (got %d)", fn, D);
    if (T < 0) return fail(CORR_EINVAL, "%s: T must be >= 0 (got %d)", fn, T);
    if (T > 0 && (!coords_rows || !grad_out_rows)) return fail(CORR_EINVAL, "%s: coords / grad_out arrays are NULL", fn);
    for (int t = 0; t < T; ++t)
        if ((rc = check_ptr(fn, coords_rows[t], "coords[t]")) || (rc = check_ptr(fn, grad_out_rows[t], "grad_out[t]")))
            return rc;
    if ((rc = check_ptr(fn, fmap1_rows, "fmap1")) || (rc = check_ptr(fn, fmap2, "fmap2")) ||
        (rc = check_ptr(fn, dfmap1_rows, "dfmap1")) || (rc = check_ptr(fn, dfmap2, "dfmap2")))
        return rc;
    const size_t need = corr_backward_workspace(base, B, D, NQ, H, W, radius);
    if (workspace_bytes < need || (need && !workspace))
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    LevelPtrs lp{};
    if ((rc = check_levels(fn, grad_pyr, levels, "grad_pyr", lp.p))) return rc;
    return hip_status(launch_backward(algo, coords_rows, grad_out_rows, T, fmap1_rows, NQ, fmap2, B, D, H, W, levels,
                                      radius, lp, dfmap1_rows, dfmap2, workspace, (hipStream_t)stream),
                      fn);
}

size_t corr_ondemand_workspace(int B, int D, int H, int W, int levels) {
    if (check_ondemand("corr_ondemand_workspace", B, D, H, W, levels)) return 0;
    return ondemand_workspace_bytes(B, D, H, W, levels);
}

int corr_ondemand_prepare(const float *fmap1, const float *fmap2, int B, int D, int H, int W, int levels,
                          void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_ondemand_prepare";
    g_err[0] = 0;
    int rc = check_ondemand(fn, B, D, H, W, levels);
    if (rc) return rc;
    if ((rc = check_ptr(fn, fmap1, "fmap1")) || (rc = check_ptr(fn, fmap2, "fmap2"))) return rc;
    if (!workspace) return fail(CORR_EINVAL, "%s: workspace is NULL", fn);
    if ((uintptr_t)workspace % 16) return fail(CORR_EINVAL, "%s: workspace is not 16-byte aligned", fn);
    const size_t need = ondemand_workspace_bytes(B, D, H, W, levels);
    if (workspace_bytes < need)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    return hip_status(launch_ondemand_prepare(fmap1, fmap2, B, D, H, W, levels, workspace, (hipStream_t)stream), fn);
}

int corr_ondemand_lookup(const void *workspace, const float *coords, int B, int D, int H, int W, int levels,
                         int radius, int flags, float *out, void *stream) {
    static const char *fn = "corr_ondemand_lookup";
    g_err[0] = 0;
    int rc = check_ondemand(fn, B, D, H, W, levels);
    if (rc || (rc = check_radius(fn, radius))) return rc;
    if (flags & ~CORR_ONDEMAND_GENERAL) return fail(CORR_EINVAL, "%s: unknown flags 0x%x", fn, flags);
    if (!workspace) return fail(CORR_EINVAL, "%s: workspace is NULL", fn);
    if ((uintptr_t)workspace % 16) return fail(CORR_EINVAL, "%s: workspace is not 16-byte aligned", fn);
    if ((rc = check_ptr(fn, coords, "coords")) || (rc = check_ptr(fn, out, "out"))) return rc;
    return hip_status(
        launch_ondemand_lookup(workspace, coords, B, D, H, W, levels, radius, flags, out, (hipStream_t)stream), fn);
}

size_t corr_ondemand_bwd_workspace(int B, int D, int H, int W, int levels, int radius) {
    if (check_ondemand("corr_ondemand_bwd_workspace", B, D, H, W, levels) ||
        check_radius("corr_ondemand_bwd_workspace", radius))
        return 0;
    return ondemand_bwd_workspace_bytes(B, D, H, W, levels, radius);
}

int corr_ondemand_backward(const void *fwd_workspace, const float *const *coords, const float *const *grads, int T,
                           int B, int D, int H, int W, int levels, int radius, void *bwd_workspace,
                           size_t bwd_workspace_bytes, float *dfmap1, float *dfmap2, void *stream) {
    static const char *fn = "corr_ondemand_backward";
    g_err[0] = 0;
    int rc = check_ondemand(fn, B, D, H, W, levels);
    if (rc || (rc = check_radius(fn, radius))) return rc;
    if (T < 1) return fail(CORR_EINVAL, "%s: T must be >= 1 (got %d)", fn, T);
    if (!fwd_workspace) return fail(CORR_EINVAL, "%s: fwd_workspace is NULL", fn);
    if ((uintptr_t)fwd_workspace % 16) return fail(CORR_EINVAL, "%s: fwd_workspace is not 16-byte aligned", fn);
    if (!bwd_workspace) return fail(CORR_EINVAL, "%s: bwd_workspace is NULL", fn);
    if ((uintptr_t)bwd_workspace % 16) return fail(CORR_EINVAL, "%s: bwd_workspace is not 16-byte aligned", fn);
    if (!coords || !grads) return fail(CORR_EINVAL, "%s: coords / grads arrays are NULL", fn);
    for (int t = 0; t < T; ++t)
        if ((rc = check_ptr(fn, coords[t], "coords[t]")) || (rc = check_ptr(fn, grads[t], "grads[t]"))) return rc;
    if (!dfmap1 && !dfmap2) return fail(CORR_EINVAL, "%s: dfmap1 and dfmap2 are both NULL", fn);
    if ((dfmap1 && (rc = check_ptr(fn, dfmap1, "dfmap1"))) || (dfmap2 && (rc = check_ptr(fn, dfmap2, "dfmap2"))))
        return rc;
    const size_t need = ondemand_bwd_workspace_bytes(B, D, H, W, levels, radius);
    if (!need) return fail(CORR_EINVAL, "%s: H and W must be <= 65536 (got %d, %d)", fn, H, W);
    if (bwd_workspace_bytes < need)
        return fail(CORR_EINVAL, "%s: bwd_workspace of %zu bytes needed, got %zu", fn, need, bwd_workspace_bytes);
    return hip_status(launch_ondemand_backward(fwd_workspace, coords, grads, T, B, D, H, W, levels, radius,
                                               bwd_workspace, dfmap1, dfmap2, (hipStream_t)stream),
                      fn);
}

size_t corr_lookup_conv_weights_bytes(void) { return lookup_conv_weights_bytes(); }

int corr_lookup_conv_weights(const float *weight, int out_channels, int in_channels, void *packed, void *stream) {
    static const char *fn = "corr_lookup_conv_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_ptr(fn, weight, "weight")) || (rc = check_ptr(fn, packed, "packed"))) return rc;
    if (out_channels != 256 || in_channels < 1 || in_channels > 4 * 81)
        return fail(CORR_EUNSUPPORTED, "%s: built for 256 output and <= 324 input channels (got %d, %d)", fn,
                    out_channels, in_channels);
    return hip_status(launch_lookup_conv_weights(weight, out_channels, in_channels, packed, (hipStream_t)stream), fn);
}

static int check_precision(const char *fn, int precision);

static int lookup_conv(const char *fn, const float *const *pyr, const float *coords, int B, int H, int W, int levels,
                       int radius, const void *packed_weight, const float *bias, int relu, float *out, void *stream,
                       int precision) {
    g_err[0] = 0;
    int rc;
    if ((rc = check_precision(fn, precision))) return rc;
    if ((rc = check_dims(fn, B, H * W, H, W, levels))) return rc;
    if (radius != 4 || levels > 4)
        return fail(CORR_EUNSUPPORTED, "%s: built for radius 4 and <= 4 levels (got %d, %d)", fn, radius, levels);
    ConstLevelPtrs lp{};
    if ((rc = check_pyramid(fn, pyr, levels, "pyr", lp.p))) return rc;
    if ((rc = check_ptr(fn, coords, "coords")) || (rc = check_ptr(fn, packed_weight, "packed_weight")) ||
        (rc = check_ptr(fn, bias, "bias")) || (rc = check_ptr(fn, out, "out")))
        return rc;
    return hip_status(launch_lookup_conv(lp, coords, B, H * W, H, W, levels, radius, packed_weight, bias, relu, out,
                                         (hipStream_t)stream, precision),
                      fn);
}

int corr_lookup_conv(const float *const *pyr, const float *coords, int B, int H, int W, int levels, int radius,
                     const void *packed_weight, const float *bias, int relu, float *out, void *stream) {
    return lookup_conv("corr_lookup_conv", pyr, coords, B, H, W, levels, radius, packed_weight, bias, relu, out,
                       stream, CORR_PREC_BF16X6);
}

// include/corr_mi355x_pw_prec.h
int corr_lookup_conv_prec(const float *const *pyr, const float *coords, int B, int H, int W, int levels, int radius,
                          const void *packed_weight, const float *bias, int relu, float *out, int precision,
                          void *stream) {
    return lookup_conv("corr_lookup_conv_prec", pyr, coords, B, H, W, levels, radius, packed_weight, bias, relu, out,
                       stream, precision);
}

int corr_ondemand_lookup_conv(const void *workspace, const float *coords, int B, int D, int H, int W, int levels,
                              int radius, int flags, const void *packed_weight, const float *bias, int relu,
                              float *out, void *stream) {
    static const char *fn = "corr_ondemand_lookup_conv";
    g_err[0] = 0;
    int rc = check_ondemand(fn, B, D, H, W, levels);
    if (rc || (rc = check_radius(fn, radius))) return rc;
    if (flags & ~CORR_ONDEMAND_GENERAL) return fail(CORR_EINVAL, "%s: unknown flags 0x%x", fn, flags);
    if (!workspace) return fail(CORR_EINVAL, "%s: workspace is NULL", fn);
    if ((uintptr_t)workspace % 16) return fail(CORR_EINVAL, "%s: workspace is not 16-byte aligned", fn);
    if ((rc = check_ptr(fn, coords, "coords"))) return rc;
    if (radius != 4 || levels > 4)
        return fail(CORR_EUNSUPPORTED, "%s: built for radius 4 and <= 4 levels (got %d, %d)", fn, radius, levels);
    if ((rc = check_ptr(fn, packed_weight, "packed_weight")) || (rc = check_ptr(fn, bias, "bias")) ||
        (rc = check_ptr(fn, out, "out")))
        return rc;
    if ((uintptr_t)packed_weight % 16) return fail(CORR_EINVAL, "%s: packed_weight is not 16-byte aligned", fn);
    return hip_status(launch_ondemand_lookup_conv(workspace, coords, B, D, H, W, levels, radius, flags, packed_weight,
                                                  bias, relu, out, (hipStream_t)stream),
                      fn);
}

size_t corr_lookup_conv_bwd_workspace(int B, int H, int W, int levels) {
    if (B < 1 || H < 1 || W < 1 || levels < 1 || levels > 4) return 0;
    return lookup_conv_bwd_workspace(B, H * W, levels);
}

int corr_lookup_conv_bwd(const float *const *pyr, const float *coords, int B, int H, int W, int levels, int radius,
                         const void *packed_weight, const float *out, int relu, const float *grad_out,
                         float *grad_weight, float *grad_bias, float *grad_lookup, void *workspace,
                         size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_lookup_conv_bwd";
    g_err[0] = 0;
    int rc = check_dims(fn, B, H * W, H, W, levels);
    if (rc) return rc;
    if (radius != 4 || levels > 4)
        return fail(CORR_EUNSUPPORTED, "%s: built for radius 4 and <= 4 levels (got %d, %d)", fn, radius, levels);
    ConstLevelPtrs lp{};
    if ((rc = check_pyramid(fn, pyr, levels, "pyr", lp.p))) return rc;
    if ((rc = check_ptr(fn, coords, "coords")) || (rc = check_ptr(fn, packed_weight, "packed_weight")) ||
        (rc = check_ptr(fn, grad_out, "grad_out")))
        return rc;
    if (relu && (rc = check_ptr(fn, out, "out"))) return rc;
    if (!grad_weight && !grad_bias && !grad_lookup) return CORR_OK;
    if (grad_weight || grad_bias) {
        const size_t need = lookup_conv_bwd_workspace(B, H * W, levels);
        if (!workspace || workspace_bytes < need)
            return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
        if ((uintptr_t)workspace % 16)
            return fail(CORR_EINVAL, "%s: workspace must be 16-byte aligned", fn);
    }
    if ((H * W) % 4 == 0 && ((uintptr_t)grad_out % 16 || (relu && (uintptr_t)out % 16)))
        return fail(CORR_EINVAL, "%s: grad_out and out must be 16-byte aligned when H*W %% 4 == 0", fn);
    return hip_status(launch_lookup_conv_bwd(lp, coords, B, H * W, H, W, levels, radius, packed_weight, out, relu,
                                             grad_out, grad_weight, grad_bias, grad_lookup, workspace,
                                             (hipStream_t)stream),
                      fn);
}

// ---- checks shared by the bf16x6 convolution entry points.  The order of an entry point's checks
// decides which error a caller sees, so each call stands where the test it replaces stood. ----
// A pack: not NULL (an entry point that tests that earlier keeps its check_ptr there) and aligned
// for the kernels' 16-byte loads.
static int check_packed(const char *fn, const void *packed) {
    const int rc = check_ptr(fn, packed, "packed");
    if (rc || (uintptr_t)packed % 16 == 0) return rc;
    return fail(CORR_EINVAL, "%s: packed is not 16-byte aligned", fn);
}
static int check_pixels(const char *fn, int B, int H, int W) {  // pixels and tiles are int-indexed
    return (long long)B * H * W > (1LL << 31) - 1 ? fail(CORR_EINVAL, "%s: B*H*W too large", fn) : CORR_OK;
}
static int check_opt_ptr(const char *fn, const void *p, const char *name) {
    return p ? check_ptr(fn, p, name) : CORR_OK;
}
// Channels off .. off + n - 1 of a tensor with `channels` of them; n is an argument of the entry
// point (n_name) or a constant of the kernel.
static int check_window(const char *fn, const char *off_name, int off, int n, const char *ch_name, int channels,
                        const char *n_name = nullptr) {
    if (off >= 0 && (long long)off + n <= channels) return CORR_OK;
    char last[64], got[32] = "";
    if (n_name) snprintf(got, sizeof got, "%s = %d, ", n_name, n);
    if (n_name) snprintf(last, sizeof last, " .. %s + %s - 1", off_name, n_name);
    else snprintf(last, sizeof last, n == 2 ? ", %s + %d" : " .. %s + %d", off_name, n - 1);
    return fail(CORR_EINVAL, "%s: channels %s%s must lie in [0, %s) (got %s = %d, %s%s = %d)", fn, off_name, last,
                ch_name, off_name, off, got, ch_name, channels);
}

static int check_gru_channels(const char *fn, int hidden, int input) {
    if (!gru_supported(hidden, input))
        return fail(CORR_EUNSUPPORTED,
                    "%s: built for hidden = 128 and hidden + input a multiple of 32, <= 1024 (got %d, %d)", fn, hidden,
                    input);
    return CORR_OK;
}

size_t corr_gru_weights_bytes(int hidden, int input) {
    if (!gru_supported(hidden, input)) return 0;
    return gru_weights_bytes(hidden, input);
}

int corr_gru_pack_weights(const float *wz, const float *wr, const float *wq, int hidden, int input, void *packed,
                          void *stream) {
    static const char *fn = "corr_gru_pack_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_gru_channels(fn, hidden, input))) return rc;
    if ((rc = check_ptr(fn, wz, "wz")) || (rc = check_ptr(fn, wr, "wr")) || (rc = check_ptr(fn, wq, "wq")) ||
        (rc = check_packed(fn, packed)))
        return rc;
    return hip_status(launch_gru_pack(wz, wr, wq, hidden, input, packed, (hipStream_t)stream), fn);
}

size_t corr_gru_workspace(int B, int hidden, int H, int W) {
    if (B < 1 || hidden < 1 || H < 1 || W < 1) return 0;
    return gru_workspace(B, hidden, H, W);
}

// CORR_PREC_*: refused first, so that no other argument is looked at under an unknown mode.
static int check_precision(const char *fn, int precision) {
    if (precision_supported(precision)) return CORR_OK;
    return fail(CORR_EINVAL, "%s: precision must be CORR_PREC_BF16X6 (0), _BF16X3 (1) or _BF16 (2) (got %d)", fn,
                precision);
}

static int gru_half_step(const char *fn, const float *h, const float *x, int B, int hidden, int input, int H, int W,
                         int dir, const void *packed, const float *bz, const float *br, const float *bq,
                         void *workspace, size_t workspace_bytes, float *h_out, void *stream, int precision) {
    g_err[0] = 0;
    int rc;
    if ((rc = check_precision(fn, precision))) return rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1)) || (rc = check_pixels(fn, B, H, W))) return rc;
    if ((rc = check_gru_channels(fn, hidden, input))) return rc;
    if (dir != 0 && dir != 1) return fail(CORR_EINVAL, "%s: dir must be 0 (1x5) or 1 (5x1) (got %d)", fn, dir);
    if ((rc = check_ptr(fn, h, "h")) || (rc = check_ptr(fn, packed, "packed")) || (rc = check_ptr(fn, bz, "bz")) ||
        (rc = check_ptr(fn, br, "br")) || (rc = check_ptr(fn, bq, "bq")) || (rc = check_ptr(fn, h_out, "h_out")))
        return rc;
    if (input > 0 && (rc = check_ptr(fn, x, "x"))) return rc;
    if ((rc = check_packed(fn, packed))) return rc;
    if (h_out == h || h_out == x) return fail(CORR_EINVAL, "%s: h_out must not alias h or x", fn);
    const size_t need = gru_workspace(B, hidden, H, W);
    if (!workspace || workspace_bytes < need)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    if ((uintptr_t)workspace % 16) return fail(CORR_EINVAL, "%s: workspace is not 16-byte aligned", fn);
    return hip_status(launch_gru_half_step(h, x, B, hidden, input, H, W, dir, packed, bz, br, bq, workspace, h_out,
                                           (hipStream_t)stream, precision),
                      fn);
}

int corr_gru_half_step(const float *h, const float *x, int B, int hidden, int input, int H, int W, int dir,
                       const void *packed, const float *bz, const float *br, const float *bq, void *workspace,
                       size_t workspace_bytes, float *h_out, void *stream) {
    return gru_half_step("corr_gru_half_step", h, x, B, hidden, input, H, W, dir, packed, bz, br, bq, workspace,
                         workspace_bytes, h_out, stream, CORR_PREC_BF16X6);
}

int corr_gru_half_step_prec(const float *h, const float *x, int B, int hidden, int input, int H, int W, int dir,
                            const void *packed, const float *bz, const float *br, const float *bq, void *workspace,
                            size_t workspace_bytes, float *h_out, int precision, void *stream) {
    return gru_half_step("corr_gru_half_step_prec", h, x, B, hidden, input, H, W, dir, packed, bz, br, bq, workspace,
                         workspace_bytes, h_out, stream, precision);
}

static int check_conv_channels(const char *fn, int cout, int ca, int cb) {
    if (!conv_supported(cout, ca, cb))
        return fail(CORR_EUNSUPPORTED,
                    "%s: built for 1 <= cout <= 1024, ca >= 32 and cb >= 0 multiples of 32, ca + cb <= 1024 "
                    "(got cout = %d, ca = %d, cb = %d)",
                    fn, cout, ca, cb);
    return CORR_OK;
}

size_t corr_conv_weights_bytes(int cout, int cin) {
    if (!conv_supported(cout, cin, 0)) return 0;
    return conv_weights_bytes(cout, cin);
}

int corr_conv_pack_weights(const float *w, int cout, int cin, void *packed, void *stream) {
    static const char *fn = "corr_conv_pack_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_conv_channels(fn, cout, cin, 0))) return rc;
    if ((rc = check_ptr(fn, w, "w")) || (rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_conv_pack(w, cout, cin, packed, (hipStream_t)stream), fn);
}

// [p, p + n) and [q, q + m) share a byte
static bool ranges_overlap(const void *p, long double n, const void *q, long double m) {
    const long double a = (long double)(uintptr_t)p, b = (long double)(uintptr_t)q;
    return a < b + m && b < a + n;
}

static int conv_forward(const char *fn, const float *in_a, int ca, const float *in_b, int cb, int B, int H, int W,
                        const void *packed, const float *bias, int cout, int relu, float *out, int out_channels,
                        int out_offset, void *stream, int precision) {
    g_err[0] = 0;
    int rc;
    if ((rc = check_precision(fn, precision))) return rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1)) || (rc = check_pixels(fn, B, H, W))) return rc;
    if ((rc = check_conv_channels(fn, cout, ca, cb))) return rc;
    if (relu != 0 && relu != 1) return fail(CORR_EINVAL, "%s: relu must be 0 or 1 (got %d)", fn, relu);
    if ((rc = check_window(fn, "out_offset", out_offset, cout, "out_channels", out_channels, "cout"))) return rc;
    if ((rc = check_ptr(fn, in_a, "in_a")) || (rc = check_ptr(fn, packed, "packed")) ||
        (rc = check_ptr(fn, out, "out")))
        return rc;
    if (cb > 0 && (rc = check_ptr(fn, in_b, "in_b"))) return rc;
    if ((rc = check_opt_ptr(fn, bias, "bias"))) return rc;
    const long double px = (long double)B * H * W * sizeof(float), ob = px * out_channels;
    if (ob > (long double)(SIZE_MAX / 2)) return fail(CORR_EINVAL, "%s: B*out_channels*H*W too large", fn);
    if (ranges_overlap(out, ob, in_a, px * ca) || (cb > 0 && ranges_overlap(out, ob, in_b, px * cb)))
        return fail(CORR_EINVAL, "%s: out must not overlap in_a or in_b", fn);
    if ((rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_conv_forward(in_a, ca, in_b, cb, B, H, W, packed, bias, cout, relu, out, out_channels,
                                          out_offset, (hipStream_t)stream, precision),
                      fn);
}

int corr_conv_forward(const float *in_a, int ca, const float *in_b, int cb, int B, int H, int W, const void *packed,
                      const float *bias, int cout, int relu, float *out, int out_channels, int out_offset,
                      void *stream) {
    return conv_forward("corr_conv_forward", in_a, ca, in_b, cb, B, H, W, packed, bias, cout, relu, out, out_channels,
                        out_offset, stream, CORR_PREC_BF16X6);
}

int corr_conv_forward_prec(const float *in_a, int ca, const float *in_b, int cb, int B, int H, int W,
                           const void *packed, const float *bias, int cout, int relu, float *out, int out_channels,
                           int out_offset, int precision, void *stream) {
    return conv_forward("corr_conv_forward_prec", in_a, ca, in_b, cb, B, H, W, packed, bias, cout, relu, out,
                        out_channels, out_offset, stream, precision);
}

size_t corr_enc_stats_bytes(int B, int cout, int Ho, int Wo) {
    if (B < 1 || cout < 1 || Ho < 1 || Wo < 1) return 0;
    return enc_stats_bytes(B, cout, Ho, Wo);
}

static int enc_conv_forward(const char *fn, const float *in, int cin, int B, int H, int W, int stride,
                            const float *in_scale, const float *in_shift, int norm_per_batch, const void *packed,
                            const float *bias, int cout, float *out, void *stats, size_t stats_bytes, void *stream,
                            int precision) {
    g_err[0] = 0;
    int rc;
    if ((rc = check_precision(fn, precision))) return rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1)) || (rc = check_pixels(fn, B, H, W))) return rc;
    if (stride != 1 && stride != 2)
        return fail(CORR_EUNSUPPORTED, "%s: built for stride 1 and 2 (got %d)", fn, stride);
    if ((rc = check_conv_channels(fn, cout, cin, 0))) return rc;
    if ((rc = check_ptr(fn, in, "in")) || (rc = check_ptr(fn, packed, "packed")) || (rc = check_ptr(fn, out, "out")))
        return rc;
    if ((rc = check_opt_ptr(fn, bias, "bias"))) return rc;
    if (!in_scale != !in_shift)
        return fail(CORR_EINVAL, "%s: in_scale and in_shift must both be given or both be NULL", fn);
    if (in_scale && ((rc = check_ptr(fn, in_scale, "in_scale")) || (rc = check_ptr(fn, in_shift, "in_shift"))))
        return rc;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if (stats) {
        if ((rc = check_ptr(fn, stats, "stats"))) return rc;
        const size_t need = enc_stats_bytes(B, cout, Ho, Wo);
        if (stats_bytes < need)
            return fail(CORR_EINVAL, "%s: stats of %zu bytes needed, got %zu", fn, need, stats_bytes);
    }
    if ((rc = check_packed(fn, packed))) return rc;
    const long double ib = (long double)B * H * W * sizeof(float) * cin;
    const long double ob = (long double)B * Ho * Wo * sizeof(float) * cout;
    if (ranges_overlap(out, ob, in, ib)) return fail(CORR_EINVAL, "%s: out must not overlap in", fn);
    return hip_status(launch_enc_conv(in, cin, B, H, W, stride, in_scale, in_shift, norm_per_batch != 0, packed, bias,
                                      cout, out, static_cast<float *>(stats), (hipStream_t)stream, precision),
                      fn);
}

int corr_enc_conv_forward(const float *in, int cin, int B, int H, int W, int stride, const float *in_scale,
                          const float *in_shift, int norm_per_batch, const void *packed, const float *bias,
                          int cout, float *out, void *stats, size_t stats_bytes, void *stream) {
    return enc_conv_forward("corr_enc_conv_forward", in, cin, B, H, W, stride, in_scale, in_shift, norm_per_batch,
                            packed, bias, cout, out, stats, stats_bytes, stream, CORR_PREC_BF16X6);
}

// include/corr_mi355x_enc_prec.h
int corr_enc_conv_forward_prec(const float *in, int cin, int B, int H, int W, int stride, const float *in_scale,
                               const float *in_shift, int norm_per_batch, const void *packed, const float *bias,
                               int cout, float *out, void *stats, size_t stats_bytes, int precision, void *stream) {
    return enc_conv_forward("corr_enc_conv_forward_prec", in, cin, B, H, W, stride, in_scale, in_shift,
                            norm_per_batch, packed, bias, cout, out, stats, stats_bytes, stream, precision);
}

// B, C, H, W of the finalize and the join: every plane and the [B][C] tables are int-indexed
static int check_enc_planes(const char *fn, int B, int C, int H, int W) {
    if (B < 1 || C < 1 || H < 1 || W < 1)
        return fail(CORR_EINVAL, "%s: B, C, H, W must be >= 1 (got %d, %d, %d, %d)", fn, B, C, H, W);
    if ((long long)B * C > (1LL << 31) - 1 || (long long)H * W > (1LL << 30))
        return fail(CORR_EINVAL, "%s: B*C or H*W too large", fn);
    return CORR_OK;
}

int corr_enc_norm_finalize(const void *stats, int B, int C, int Ho, int Wo, float eps, float *scale, float *shift,
                           void *stream) {
    static const char *fn = "corr_enc_norm_finalize";
    g_err[0] = 0;
    int rc = check_enc_planes(fn, B, C, Ho, Wo);
    if (rc) return rc;
    if (!(eps > 0.f)) return fail(CORR_EINVAL, "%s: eps must be positive", fn);
    if ((rc = check_ptr(fn, stats, "stats")) || (rc = check_ptr(fn, scale, "scale")) ||
        (rc = check_ptr(fn, shift, "shift")))
        return rc;
    return hip_status(launch_enc_finalize(static_cast<const float *>(stats), B, C, Ho, Wo, eps, scale, shift,
                                          (hipStream_t)stream),
                      fn);
}

int corr_enc_join(const float *y, const float *scale, const float *shift, int norm_per_batch, const float *skip,
                  int B, int C, int H, int W, float *out, void *stream) {
    static const char *fn = "corr_enc_join";
    g_err[0] = 0;
    int rc = check_enc_planes(fn, B, C, H, W);
    if (rc) return rc;
    if ((rc = check_ptr(fn, y, "y")) || (rc = check_ptr(fn, scale, "scale")) || (rc = check_ptr(fn, shift, "shift")) ||
        (rc = check_ptr(fn, skip, "skip")) || (rc = check_ptr(fn, out, "out")))
        return rc;
    return hip_status(launch_enc_join(y, scale, shift, norm_per_batch != 0, skip, B, C, H, W, out, (hipStream_t)stream),
                      fn);
}

size_t corr_enc_stem_weights_bytes(int cout, int cin) {
    if (!enc_stem_supported(cout, cin)) return 0;
    return enc_stem_weights_bytes(cout);
}

static int check_stem_channels(const char *fn, int cout, int cin) {
    if (cin < 1) return fail(CORR_EINVAL, "%s: cin must be >= 1 (got %d)", fn, cin);
    if (!enc_stem_supported(cout, cin))
        return fail(CORR_EUNSUPPORTED, "%s: built for 1 <= cin <= 16 and 1 <= cout <= 1024 (got cin = %d, cout = %d)",
                    fn, cin, cout);
    return CORR_OK;
}

int corr_enc_stem_pack_weights(const float *w, int cout, int cin, void *packed, void *stream) {
    static const char *fn = "corr_enc_stem_pack_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_stem_channels(fn, cout, cin))) return rc;
    if ((rc = check_ptr(fn, w, "w")) || (rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_enc_stem_pack(w, cout, cin, packed, (hipStream_t)stream), fn);
}

// The checks the stem and the pointwise convolution share, after their channel counts: the
// pointers, the statistics buffer, the pack's alignment, out against in.
static int check_enc_front(const char *fn, const float *in, int cin, int B, int H, int W, int stride,
                           const void *packed, const float *bias, int cout, const float *out, const void *stats,
                           size_t stats_bytes) {
    int rc;
    if ((rc = check_ptr(fn, in, "in")) || (rc = check_ptr(fn, packed, "packed")) || (rc = check_ptr(fn, out, "out")))
        return rc;
    if ((rc = check_opt_ptr(fn, bias, "bias"))) return rc;
    const int Ho = (H - 1) / stride + 1, Wo = (W - 1) / stride + 1;
    if (stats) {
        if ((rc = check_ptr(fn, stats, "stats"))) return rc;
        const size_t need = enc_stats_bytes(B, cout, Ho, Wo);
        if (stats_bytes < need)
            return fail(CORR_EINVAL, "%s: stats of %zu bytes needed, got %zu", fn, need, stats_bytes);
    }
    const long double ib = (long double)B * H * W * sizeof(float) * cin;
    const long double ob = (long double)B * Ho * Wo * sizeof(float) * cout;
    if (ranges_overlap(out, ob, in, ib)) return fail(CORR_EINVAL, "%s: out must not overlap in", fn);
    if ((rc = check_packed(fn, packed))) return rc;
    return CORR_OK;
}

static int enc_stem_forward(const char *fn, const float *in, int cin, int B, int H, int W, const void *packed,
                            const float *bias, int cout, float *out, void *stats, size_t stats_bytes, void *stream,
                            int precision) {
    g_err[0] = 0;
    int rc;
    if ((rc = check_precision(fn, precision))) return rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1)) || (rc = check_pixels(fn, B, H, W))) return rc;
    if ((rc = check_stem_channels(fn, cout, cin))) return rc;
    if ((rc = check_enc_front(fn, in, cin, B, H, W, 2, packed, bias, cout, out, stats, stats_bytes))) return rc;
    return hip_status(launch_enc_stem(in, cin, B, H, W, packed, bias, cout, out, static_cast<float *>(stats),
                                      (hipStream_t)stream, precision),
                      fn);
}

int corr_enc_stem_forward(const float *in, int cin, int B, int H, int W, const void *packed, const float *bias,
                          int cout, float *out, void *stats, size_t stats_bytes, void *stream) {
    return enc_stem_forward("corr_enc_stem_forward", in, cin, B, H, W, packed, bias, cout, out, stats, stats_bytes,
                            stream, CORR_PREC_BF16X6);
}

int corr_enc_stem_forward_prec(const float *in, int cin, int B, int H, int W, const void *packed, const float *bias,
                               int cout, float *out, void *stats, size_t stats_bytes, int precision, void *stream) {
    return enc_stem_forward("corr_enc_stem_forward_prec", in, cin, B, H, W, packed, bias, cout, out, stats,
                            stats_bytes, stream, precision);
}

static int check_pw_channels(const char *fn, int cout, int cin) {
    if (!enc_pw_supported(cout, cin))
        return fail(CORR_EUNSUPPORTED,
                    "%s: built for 1 <= cout <= 1024 and cin a multiple of 32 in 32 .. 1024 (got cout = %d, cin = %d)",
                    fn, cout, cin);
    return CORR_OK;
}

size_t corr_enc_pw_weights_bytes(int cout, int cin) {
    if (!enc_pw_supported(cout, cin)) return 0;
    return enc_pw_weights_bytes(cout, cin);
}

int corr_enc_pw_pack_weights(const float *w, int cout, int cin, void *packed, void *stream) {
    static const char *fn = "corr_enc_pw_pack_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_pw_channels(fn, cout, cin))) return rc;
    if ((rc = check_ptr(fn, w, "w")) || (rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_enc_pw_pack(w, cout, cin, packed, (hipStream_t)stream), fn);
}

static int enc_pw_forward(const char *fn, const float *in, int cin, int B, int H, int W, int stride,
                          const void *packed, const float *bias, int cout, float *out, void *stats,
                          size_t stats_bytes, void *stream, int precision) {
    g_err[0] = 0;
    int rc;
    if ((rc = check_precision(fn, precision))) return rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1)) || (rc = check_pixels(fn, B, H, W))) return rc;
    if (stride != 1 && stride != 2)
        return fail(CORR_EUNSUPPORTED, "%s: built for stride 1 and 2 (got %d)", fn, stride);
    if ((rc = check_pw_channels(fn, cout, cin))) return rc;
    if ((rc = check_enc_front(fn, in, cin, B, H, W, stride, packed, bias, cout, out, stats, stats_bytes))) return rc;
    return hip_status(launch_enc_pw(in, cin, B, H, W, stride, packed, bias, cout, out, static_cast<float *>(stats),
                                    (hipStream_t)stream, precision),
                      fn);
}

int corr_enc_pw_forward(const float *in, int cin, int B, int H, int W, int stride, const void *packed,
                        const float *bias, int cout, float *out, void *stats, size_t stats_bytes, void *stream) {
    return enc_pw_forward("corr_enc_pw_forward", in, cin, B, H, W, stride, packed, bias, cout, out, stats,
                          stats_bytes, stream, CORR_PREC_BF16X6);
}

int corr_enc_pw_forward_prec(const float *in, int cin, int B, int H, int W, int stride, const void *packed,
                             const float *bias, int cout, float *out, void *stats, size_t stats_bytes, int precision,
                             void *stream) {
    return enc_pw_forward("corr_enc_pw_forward_prec", in, cin, B, H, W, stride, packed, bias, cout, out, stats,
                          stats_bytes, stream, precision);
}

int corr_enc_join_affine(const float *y, const float *scale, const float *shift, int norm_per_batch,
                         const float *skip, const float *skip_scale, const float *skip_shift, int skip_per_batch,
                         int skip_relu, int B, int C, int H, int W, float *out, void *stream) {
    static const char *fn = "corr_enc_join_affine";
    g_err[0] = 0;
    int rc = check_enc_planes(fn, B, C, H, W);
    if (rc) return rc;
    if ((rc = check_ptr(fn, y, "y")) || (rc = check_ptr(fn, scale, "scale")) || (rc = check_ptr(fn, shift, "shift")) ||
        (rc = check_ptr(fn, skip, "skip")) || (rc = check_ptr(fn, out, "out")))
        return rc;
    if (!skip_scale != !skip_shift)
        return fail(CORR_EINVAL, "%s: skip_scale and skip_shift must both be given or both be NULL", fn);
    if (skip_scale && ((rc = check_ptr(fn, skip_scale, "skip_scale")) || (rc = check_ptr(fn, skip_shift, "skip_shift"))))
        return rc;
    for (const int f : {norm_per_batch, skip_per_batch, skip_relu})
        if (f != 0 && f != 1)
            return fail(CORR_EINVAL, "%s: norm_per_batch, skip_per_batch and skip_relu must be 0 or 1 (got %d, %d, %d)",
                        fn, norm_per_batch, skip_per_batch, skip_relu);
    return hip_status(launch_enc_join_affine(y, scale, shift, norm_per_batch, skip, skip_scale, skip_shift,
                                             skip_per_batch, skip_relu, B, C, H, W, out, (hipStream_t)stream),
                      fn);
}

int corr_convex_upsample(const float *flow, const float *mask, int N, int h, int w, float *out, void *stream) {
    static const char *fn = "corr_convex_upsample";
    g_err[0] = 0;
    if (N < 1 || h < 1 || w < 1)
        return fail(CORR_EINVAL, "%s: N, h, w must be >= 1 (got %d, %d, %d)", fn, N, h, w);
    int rc;
    if ((rc = check_ptr(fn, flow, "flow")) || (rc = check_ptr(fn, mask, "mask")) || (rc = check_ptr(fn, out, "out")))
        return rc;
    return hip_status(launch_convex_upsample(flow, mask, N, h, w, out, (hipStream_t)stream), fn);
}

size_t corr_mask_upsample_weights_bytes(void) { return mask_upsample_weights_bytes(); }

int corr_mask_upsample_pack_weights(const float *w, void *packed, void *stream) {
    static const char *fn = "corr_mask_upsample_pack_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_ptr(fn, w, "w")) || (rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_mask_upsample_pack(w, packed, (hipStream_t)stream), fn);
}

static int mask_upsample_forward(const char *fn, const float *hidden, int hidden_channels, int hidden_offset,
                                 const float *flow, const void *packed, const float *bias, float mask_scale, int B,
                                 int H, int W, float *out, void *stream, int precision) {
    g_err[0] = 0;
    int rc;
    if ((rc = check_precision(fn, precision))) return rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1))) return rc;
    if ((rc = check_window(fn, "hidden_offset", hidden_offset, 256, "hidden_channels", hidden_channels))) return rc;
    if ((rc = check_ptr(fn, hidden, "hidden")) || (rc = check_ptr(fn, flow, "flow")) ||
        (rc = check_ptr(fn, packed, "packed")) || (rc = check_ptr(fn, bias, "bias")) ||
        (rc = check_ptr(fn, out, "out")))
        return rc;
    if (!(mask_scale - mask_scale == 0.f)) return fail(CORR_EINVAL, "%s: mask_scale must be finite", fn);
    const long double px = (long double)B * H * W * sizeof(float), ob = px * 128;
    if (px * hidden_channels > (long double)(SIZE_MAX / 2) || ob > (long double)(SIZE_MAX / 2))
        return fail(CORR_EINVAL, "%s: B*hidden_channels*H*W too large", fn);
    if (ranges_overlap(out, ob, hidden, px * hidden_channels) || ranges_overlap(out, ob, flow, px * 2))
        return fail(CORR_EINVAL, "%s: out must not overlap hidden or flow", fn);
    if ((rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_mask_upsample(hidden, hidden_channels, hidden_offset, flow, packed, bias, mask_scale, B,
                                           H, W, out, (hipStream_t)stream, precision),
                      fn);
}

int corr_mask_upsample_forward(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                               const void *packed, const float *bias, float mask_scale, int B, int H, int W,
                               float *out, void *stream) {
    return mask_upsample_forward("corr_mask_upsample_forward", hidden, hidden_channels, hidden_offset, flow, packed,
                                 bias, mask_scale, B, H, W, out, stream, CORR_PREC_BF16X6);
}

// include/corr_mi355x_pw_prec.h
int corr_mask_upsample_forward_prec(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                                    const void *packed, const float *bias, float mask_scale, int B, int H, int W,
                                    float *out, int precision, void *stream) {
    return mask_upsample_forward("corr_mask_upsample_forward_prec", hidden, hidden_channels, hidden_offset, flow,
                                 packed, bias, mask_scale, B, H, W, out, stream, precision);
}

size_t corr_flow_enc_weights_bytes(int cout) {
    if (!flow_enc_supported(cout)) return 0;
    return flow_enc_weights_bytes(cout);
}

static int check_flow_enc_channels(const char *fn, int cout) {
    if (!flow_enc_supported(cout))
        return fail(CORR_EUNSUPPORTED, "%s: built for 1 <= cout <= 1024 (got cout = %d)", fn, cout);
    return CORR_OK;
}

int corr_flow_enc_pack_weights(const float *w, int cout, void *packed, void *stream) {
    static const char *fn = "corr_flow_enc_pack_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_flow_enc_channels(fn, cout))) return rc;
    if ((rc = check_ptr(fn, w, "w")) || (rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_flow_enc_pack(w, cout, packed, (hipStream_t)stream), fn);
}

int corr_flow_enc_forward(const float *flow, int B, int H, int W, const void *packed, const float *bias, int cout,
                          int relu, float *out, int out_channels, int out_offset, float *flow_copy,
                          int copy_channels, int copy_offset, void *stream) {
    static const char *fn = "corr_flow_enc_forward";
    g_err[0] = 0;
    int rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1)) || (rc = check_pixels(fn, B, H, W))) return rc;
    if ((rc = check_flow_enc_channels(fn, cout))) return rc;
    if (relu != 0 && relu != 1) return fail(CORR_EINVAL, "%s: relu must be 0 or 1 (got %d)", fn, relu);
    if ((rc = check_window(fn, "out_offset", out_offset, cout, "out_channels", out_channels, "cout"))) return rc;
    if ((rc = check_ptr(fn, flow, "flow")) || (rc = check_ptr(fn, packed, "packed")) ||
        (rc = check_ptr(fn, out, "out")))
        return rc;
    if ((rc = check_opt_ptr(fn, bias, "bias"))) return rc;
    const long double px = (long double)B * H * W * sizeof(float), ob = px * out_channels;
    if (ob > (long double)(SIZE_MAX / 2)) return fail(CORR_EINVAL, "%s: B*out_channels*H*W too large", fn);
    if (ranges_overlap(out, ob, flow, px * 2)) return fail(CORR_EINVAL, "%s: out must not overlap flow", fn);
    if (flow_copy) {
        if ((rc = check_ptr(fn, flow_copy, "flow_copy"))) return rc;
        if ((rc = check_window(fn, "copy_offset", copy_offset, 2, "copy_channels", copy_channels))) return rc;
        const long double cb = px * copy_channels;
        if (cb > (long double)(SIZE_MAX / 2)) return fail(CORR_EINVAL, "%s: B*copy_channels*H*W too large", fn);
        if (ranges_overlap(flow_copy, cb, flow, px * 2))
            return fail(CORR_EINVAL, "%s: flow_copy must not overlap flow", fn);
        // out and flow_copy may be one tensor written through disjoint channel windows, nothing else
        if (ranges_overlap(flow_copy, cb, out, ob)) {
            const bool disjoint = copy_offset + 2 <= out_offset || (long long)out_offset + cout <= copy_offset;
            if (flow_copy != out || copy_channels != out_channels || !disjoint)
                return fail(CORR_EINVAL, "%s: out and flow_copy overlap (one tensor with disjoint channel windows "
                                         "is the only overlap accepted)",
                            fn);
        }
    }
    if ((rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_flow_enc(flow, B, H, W, packed, bias, cout, relu, out, out_channels, out_offset,
                                      flow_copy, copy_channels, copy_offset, (hipStream_t)stream),
                      fn);
}

size_t corr_flow_head_weights_bytes(void) { return flow_head_weights_bytes(); }

int corr_flow_head_pack_weights(const float *w, void *packed, void *stream) {
    static const char *fn = "corr_flow_head_pack_weights";
    g_err[0] = 0;
    int rc;
    if ((rc = check_ptr(fn, w, "w")) || (rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_flow_head_pack(w, packed, (hipStream_t)stream), fn);
}

int corr_flow_head_forward(const float *hidden, int hidden_channels, int hidden_offset, int B, int H, int W,
                           const void *packed, const float *bias, const float *coords_in, const float *coords0,
                           float *delta, float *coords_out, float *flow_out, void *stream) {
    static const char *fn = "corr_flow_head_forward";
    g_err[0] = 0;
    int rc;
    if ((rc = check_dims(fn, B, 1, H, W, 1)) || (rc = check_pixels(fn, B, H, W))) return rc;
    if ((rc = check_window(fn, "hidden_offset", hidden_offset, 256, "hidden_channels", hidden_channels))) return rc;
    if ((rc = check_ptr(fn, hidden, "hidden")) || (rc = check_ptr(fn, packed, "packed")) ||
        (rc = check_ptr(fn, bias, "bias")) || (rc = check_ptr(fn, delta, "delta")))
        return rc;
    if (coords0 && !coords_in) return fail(CORR_EINVAL, "%s: coords0 needs coords_in", fn);
    if (coords_in && ((rc = check_ptr(fn, coords_in, "coords_in")) || (rc = check_ptr(fn, coords_out, "coords_out"))))
        return rc;
    if (coords0 && ((rc = check_ptr(fn, coords0, "coords0")) || (rc = check_ptr(fn, flow_out, "flow_out")))) return rc;
    const long double px = (long double)B * H * W * sizeof(float), hb = px * hidden_channels, cb = px * 2;
    if (hb > (long double)(SIZE_MAX / 2)) return fail(CORR_EINVAL, "%s: B*hidden_channels*H*W too large", fn);
    // the outputs that this call writes, against every input and each other
    const void *outs[3] = {delta, coords_in ? coords_out : nullptr, coords0 ? flow_out : nullptr};
    static const char *names[3] = {"delta", "coords_out", "flow_out"};
    for (int k = 0; k < 3; ++k) {
        if (!outs[k]) continue;
        if (ranges_overlap(outs[k], cb, hidden, hb) || (coords_in && ranges_overlap(outs[k], cb, coords_in, cb)) ||
            (coords0 && ranges_overlap(outs[k], cb, coords0, cb)))
            return fail(CORR_EINVAL, "%s: %s must not overlap hidden, coords_in or coords0 (no in-place update)", fn,
                        names[k]);
        for (int j = 0; j < k; ++j)
            if (outs[j] && ranges_overlap(outs[k], cb, outs[j], cb))
                return fail(CORR_EINVAL, "%s: %s must not overlap %s", fn, names[k], names[j]);
    }
    if ((rc = check_packed(fn, packed))) return rc;
    return hip_status(launch_flow_head(hidden, hidden_channels, hidden_offset, B, H, W, packed, bias, coords_in,
                                       coords0, delta, coords_in ? coords_out : nullptr, coords0 ? flow_out : nullptr,
                                       (hipStream_t)stream),
                      fn);
}

size_t corr_convex_upsample_bwd_workspace(int N, int h, int w) {
    if (N < 1 || h < 1 || w < 1) return 0;
    return convex_upsample_bwd_workspace(N, h, w);
}

int corr_convex_upsample_bwd(const float *flow, const float *mask, const float *grad_out, int N, int h, int w,
                             float *dflow, float *dmask, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_convex_upsample_bwd";
    g_err[0] = 0;
    if (N < 1 || h < 1 || w < 1)
        return fail(CORR_EINVAL, "%s: N, h, w must be >= 1 (got %d, %d, %d)", fn, N, h, w);
    int rc;
    if ((rc = check_ptr(fn, flow, "flow")) || (rc = check_ptr(fn, mask, "mask")) ||
        (rc = check_ptr(fn, grad_out, "grad_out")) || (rc = check_ptr(fn, dflow, "dflow")) ||
        (rc = check_ptr(fn, dmask, "dmask")) || (rc = check_ptr(fn, workspace, "workspace")))
        return rc;
    const size_t need = convex_upsample_bwd_workspace(N, h, w);
    if (workspace_bytes < need)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    return hip_status(launch_convex_upsample_bwd(flow, mask, grad_out, N, h, w, dflow, dmask, workspace,
                                                 (hipStream_t)stream),
                      fn);
}

size_t corr_voxel_grid_workspace(int n_events, int C, int H, int W) {
    if (n_events < 0 || C < 1 || H < 1 || W < 1) return 0;
    return voxel_workspace(n_events, C, H, W);
}

int corr_voxel_grid(const float *x, const float *y, const float *t, const float *p, int n_events, int C, int H,
                    int W, int normalize, float *out, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_voxel_grid";
    g_err[0] = 0;
    if (n_events < 0 || C < 1 || H < 1 || W < 1)
        return fail(CORR_EINVAL, "%s: need n_events >= 0 and C, H, W >= 1 (got %d, %d, %d, %d)", fn, n_events, C,
                    H, W);
    if ((long long)n_events * 4 >= (1ll << 31) || (long long)C * H * W >= (1ll << 31))
        return fail(CORR_EINVAL, "%s: problem too large", fn);
    int rc;
    if ((rc = check_ptr(fn, out, "out"))) return rc;
    if (n_events > 0 && ((rc = check_ptr(fn, x, "x")) || (rc = check_ptr(fn, y, "y")) ||
                         (rc = check_ptr(fn, t, "t")) || (rc = check_ptr(fn, p, "p"))))
        return rc;
    const size_t need = voxel_workspace(n_events, C, H, W);
    if (workspace_bytes < need || !workspace)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    return hip_status(launch_voxel_grid(x, y, t, p, n_events, C, H, W, normalize, out, workspace,
                                        (hipStream_t)stream),
                      fn);
}

size_t corr_voxel_grid_tbilinear_workspace(int n_events, int C, int H, int W) {
    if (n_events < 0 || C < 1 || H < 1 || W < 1) return 0;
    return voxel_tbilinear_workspace(n_events, C, H, W);
}

int corr_voxel_grid_tbilinear(const double *events, int n_events, int C, int H, int W, int normalize, float *out,
                              void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_voxel_grid_tbilinear";
    g_err[0] = 0;
    if (n_events < 0 || C < 1 || H < 1 || W < 1)
        return fail(CORR_EINVAL, "%s: need n_events >= 0 and C, H, W >= 1 (got %d, %d, %d, %d)", fn, n_events, C,
                    H, W);
    if ((long long)n_events * 2 >= (1ll << 31) || (long long)C * H * W >= (1ll << 31))
        return fail(CORR_EINVAL, "%s: problem too large", fn);
    int rc;
    if ((rc = check_ptr(fn, out, "out"))) return rc;
    if (n_events > 0) {
        if ((rc = check_ptr(fn, events, "events"))) return rc;
        if ((uintptr_t)events % 8) return fail(CORR_EINVAL, "%s: events is not 8-byte aligned", fn);
    }
    const size_t need = voxel_tbilinear_workspace(n_events, C, H, W);
    if (workspace_bytes < need || !workspace)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    return hip_status(
        launch_voxel_grid_tbilinear(events, n_events, C, H, W, normalize, out, workspace, (hipStream_t)stream), fn);
}

size_t corr_forward_splat_workspace(int B, int H, int W) {
    if (B < 1 || H < 1 || W < 1) return 0;
    return splat_workspace(B, H, W);
}

int corr_forward_splat(const float *flow, int B, int H, int W, float *out, void *workspace,
                       size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_forward_splat";
    g_err[0] = 0;
    if (B < 1 || H < 1 || W < 1)
        return fail(CORR_EINVAL, "%s: B, H, W must be >= 1 (got %d, %d, %d)", fn, B, H, W);
    if ((long long)H * W * 4 >= (1ll << 31))
        return fail(CORR_EINVAL, "%s: %dx%d is too large", fn, H, W);
    int rc;
    if ((rc = check_ptr(fn, flow, "flow")) || (rc = check_ptr(fn, out, "out"))) return rc;
    const size_t need = splat_workspace(B, H, W);
    if (workspace_bytes < need || !workspace)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes needed, got %zu", fn, need, workspace_bytes);
    return hip_status(launch_forward_splat(flow, B, H, W, out, workspace, (hipStream_t)stream), fn);
}

int corr_build_bwd(const float *grad_c, const float *fmap1, const float *fmap2, int B, int D,
                   int H, int W, float *dfmap1, float *dfmap2, void *workspace,
                   size_t workspace_bytes, void *stream) {
    return corr_build_bwd_rows(grad_c, fmap1, H * W, fmap2, B, D, H, W, dfmap1, dfmap2, workspace,
                               workspace_bytes, stream);
}

}  // extern "C"

// ---- include/corr_mi355x_train.h: the sequence loss, alone and fused with the convex upsampling ----
namespace corr {

static int check_ptr8(const char *fn, const void *p, const char *name) {
    if (!p) return fail(CORR_EINVAL, "%s: %s is NULL", fn, name);
    if ((uintptr_t)p % 8) return fail(CORR_EINVAL, "%s: %s is not 8-byte aligned", fn, name);
    return CORR_OK;
}

static int check_max_flow(const char *fn, float max_flow) {
    if (!(max_flow > 0.0f) || max_flow > 3.402823466e38f)
        return fail(CORR_EINVAL, "%s: max_flow must be finite and positive (got %g)", fn, (double)max_flow);
    return CORR_OK;
}

// The loss frame H x W of N items: sizes, and every tensor of it int-indexable.
static int check_loss_frame(const char *fn, int N, int H, int W) {
    if (N < 1) return fail(CORR_EINVAL, "%s: N must be >= 1 (got %d)", fn, N);
    if (H < 1 || W < 1) return fail(CORR_EINVAL, "%s: H, W must be >= 1 (got %d, %d)", fn, H, W);
    if ((long double)N * 2 * H * W >= (long double)(1LL << 31))
        return fail(CORR_EINVAL, "%s: N*2*H*W too large (2^31 elements or more)", fn);
    return CORR_OK;
}

static int check_upsample_loss(const char *fn, int N, int h, int w, int H, int W, float max_flow) {
    if (N < 1 || h < 1 || w < 1)
        return fail(CORR_EINVAL, "%s: N, h, w must be >= 1 (got %d, %d, %d)", fn, N, h, w);
    if ((long double)N * 576 * h * w >= (long double)(1LL << 31))
        return fail(CORR_EINVAL, "%s: N*576*h*w too large (2^31 elements or more)", fn);
    if (H < 1 || W < 1) return fail(CORR_EINVAL, "%s: H, W must be >= 1 (got %d, %d)", fn, H, W);
    if (H > 8 * h || W > 8 * w)
        return fail(CORR_EINVAL, "%s: H, W must be <= 8h, 8w = %d, %d (got %d, %d)", fn, 8 * h, 8 * w, H, W);
    return check_max_flow(fn, max_flow);
}

static int check_workspace8(const char *fn, const void *workspace, size_t workspace_bytes, size_t need) {
    const int rc = check_ptr8(fn, workspace, "workspace");
    if (rc) return rc;
    if (workspace_bytes < need)
        return fail(CORR_EINVAL, "%s: workspace of %zu bytes, %zu needed", fn, workspace_bytes, need);
    return CORR_OK;
}

}  // namespace corr

extern "C" {

size_t corr_upsample_loss_workspace(int N, int h, int w) {
    if (N < 1 || h < 1 || w < 1) return 0;
    return upsample_loss_workspace(N, h, w);
}

int corr_upsample_loss(const float *flow, const float *mask, const float *gt, const float *valid, int N, int h,
                       int w, int H, int W, float max_flow, int want_metrics, double *out, void *workspace,
                       size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_upsample_loss";
    g_err[0] = 0;
    int rc = check_upsample_loss(fn, N, h, w, H, W, max_flow);
    if (rc) return rc;
    if ((rc = check_ptr(fn, flow, "flow")) || (rc = check_ptr(fn, mask, "mask")) || (rc = check_ptr(fn, gt, "gt")) ||
        (rc = check_ptr(fn, valid, "valid")) || (rc = check_ptr8(fn, out, "out")) ||
        (rc = check_workspace8(fn, workspace, workspace_bytes, upsample_loss_workspace(N, h, w))))
        return rc;
    return hip_status(launch_upsample_loss(flow, mask, gt, valid, N, h, w, H, W, max_flow, want_metrics != 0, out,
                                           workspace, (hipStream_t)stream),
                      fn);
}

int corr_upsample_loss_bwd(const float *flow, const float *mask, const float *gt, const float *valid,
                           const float *scale, int N, int h, int w, int H, int W, float max_flow, float *dflow,
                           float *dmask, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_upsample_loss_bwd";
    g_err[0] = 0;
    int rc = check_upsample_loss(fn, N, h, w, H, W, max_flow);
    if (rc) return rc;
    if ((rc = check_ptr(fn, flow, "flow")) || (rc = check_ptr(fn, mask, "mask")) || (rc = check_ptr(fn, gt, "gt")) ||
        (rc = check_ptr(fn, valid, "valid")) || (rc = check_ptr(fn, scale, "scale")) ||
        (rc = check_ptr(fn, dflow, "dflow")) || (rc = check_ptr(fn, dmask, "dmask")) ||
        (rc = check_workspace8(fn, workspace, workspace_bytes, upsample_loss_workspace(N, h, w))))
        return rc;
    return hip_status(launch_upsample_loss_bwd(flow, mask, gt, valid, scale, N, h, w, H, W, max_flow, dflow, dmask,
                                               workspace, (hipStream_t)stream),
                      fn);
}

size_t corr_sequence_loss_workspace(int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return 0;
    return sequence_loss_workspace(N, H, W);
}

int corr_sequence_loss(const float *pred, const float *gt, const float *valid, int N, int H, int W, float max_flow,
                       int want_metrics, double *out, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_sequence_loss";
    g_err[0] = 0;
    int rc = check_loss_frame(fn, N, H, W);
    if (rc || (rc = check_max_flow(fn, max_flow))) return rc;
    if ((rc = check_ptr(fn, pred, "pred")) || (rc = check_ptr(fn, gt, "gt")) || (rc = check_ptr(fn, valid, "valid")) ||
        (rc = check_ptr8(fn, out, "out")) ||
        (rc = check_workspace8(fn, workspace, workspace_bytes, sequence_loss_workspace(N, H, W))))
        return rc;
    return hip_status(launch_sequence_loss(pred, gt, valid, N, H, W, max_flow, want_metrics != 0, out, workspace,
                                           (hipStream_t)stream),
                      fn);
}

int corr_sequence_loss_bwd(const float *pred, const float *gt, const float *valid, const float *scale, int N, int H,
                           int W, float max_flow, float *dpred, void *stream) {
    static const char *fn = "corr_sequence_loss_bwd";
    g_err[0] = 0;
    int rc = check_loss_frame(fn, N, H, W);
    if (rc || (rc = check_max_flow(fn, max_flow))) return rc;
    if ((rc = check_ptr(fn, pred, "pred")) || (rc = check_ptr(fn, gt, "gt")) || (rc = check_ptr(fn, valid, "valid")) ||
        (rc = check_ptr(fn, scale, "scale")) || (rc = check_ptr(fn, dpred, "dpred")))
        return rc;
    return hip_status(launch_sequence_loss_bwd(pred, gt, valid, scale, N, H, W, max_flow, dpred, (hipStream_t)stream),
                      fn);
}

}  // extern "C"

// ---- include/corr_mi355x_train_head.h: the same loss with the mask head inside the launch ----
namespace corr {

static int check_mask_loss(const char *fn, const float *hidden, int hidden_channels, int hidden_offset,
                           const float *flow, const void *packed, const float *bias, float mask_scale,
                           const float *gt, const float *valid, int N, int h, int w, int H, int W, float max_flow,
                           const void *workspace, size_t workspace_bytes) {
    // N*576*h*w < 2^31: dz, every pixel index and, by H*W <= 64 h*w, gt and valid
    int rc = check_upsample_loss(fn, N, h, w, H, W, max_flow);
    if (rc) return rc;
    if ((rc = check_window(fn, "hidden_offset", hidden_offset, 256, "hidden_channels", hidden_channels))) return rc;
    if ((long double)N * hidden_channels * h * w >= (long double)(1LL << 31))
        return fail(CORR_EINVAL, "%s: N*hidden_channels*h*w too large (2^31 elements or more)", fn);
    if (!(mask_scale - mask_scale == 0.f)) return fail(CORR_EINVAL, "%s: mask_scale must be finite", fn);
    if ((rc = check_ptr(fn, hidden, "hidden")) || (rc = check_ptr(fn, flow, "flow")) ||
        (rc = check_packed(fn, packed)) || (rc = check_ptr(fn, bias, "bias")) || (rc = check_ptr(fn, gt, "gt")) ||
        (rc = check_ptr(fn, valid, "valid")))
        return rc;
    return check_workspace8(fn, workspace, workspace_bytes, mask_upsample_loss_workspace(N, h, w));
}

}  // namespace corr

extern "C" {

size_t corr_mask_upsample_loss_workspace(int N, int h, int w) {
    if (N < 1 || h < 1 || w < 1) return 0;
    return mask_upsample_loss_workspace(N, h, w);
}

int corr_mask_upsample_loss(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                            const void *packed, const float *bias, float mask_scale, const float *gt,
                            const float *valid, int N, int h, int w, int H, int W, float max_flow, int want_metrics,
                            double *out, void *workspace, size_t workspace_bytes, void *stream) {
    static const char *fn = "corr_mask_upsample_loss";
    g_err[0] = 0;
    int rc = check_mask_loss(fn, hidden, hidden_channels, hidden_offset, flow, packed, bias, mask_scale, gt, valid, N,
                             h, w, H, W, max_flow, workspace, workspace_bytes);
    if (rc || (rc = check_ptr8(fn, out, "out"))) return rc;
    return hip_status(launch_mask_upsample_loss(hidden, hidden_channels, hidden_offset, flow, packed, bias, mask_scale,
                                                gt, valid, N, h, w, H, W, max_flow, want_metrics != 0, out, workspace,
                                                (hipStream_t)stream),
                      fn);
}

int corr_mask_upsample_loss_bwd(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                                const void *packed, const float *bias, float mask_scale, const float *gt,
                                const float *valid, const float *scale, int N, int h, int w, int H, int W,
                                float max_flow, float *dflow, float *dz, void *workspace, size_t workspace_bytes,
                                void *stream) {
    static const char *fn = "corr_mask_upsample_loss_bwd";
    g_err[0] = 0;
    int rc = check_mask_loss(fn, hidden, hidden_channels, hidden_offset, flow, packed, bias, mask_scale, gt, valid, N,
                             h, w, H, W, max_flow, workspace, workspace_bytes);
    if (rc || (rc = check_ptr(fn, scale, "scale")) || (rc = check_ptr(fn, dflow, "dflow")) ||
        (rc = check_ptr(fn, dz, "dz")))
        return rc;
    return hip_status(launch_mask_upsample_loss_bwd(hidden, hidden_channels, hidden_offset, flow, packed, bias,
                                                    mask_scale, gt, valid, scale, N, h, w, H, W, max_flow, dflow, dz,
                                                    workspace, (hipStream_t)stream),
                      fn);
}

}  // extern "C"
