// The bf16x6 family's device code: fp32 products on v_mfma_f32_16x16x32_bf16 through the exact
// three-piece split (x = hi + mid + lo), six piece products per fp32 product.  Shared by the
// split build and backward (the split only) and by the convolution kernels (corr_lookup_conv,
// corr_ondemand_conv, corr_gru, corr_conv, corr_mask_upsample, corr_enc_front, corr_flow .hip).
// Internal, not part of the C-ABI.
//
// The reduced modes (corr_gru.hip, corr_conv.hip's update-block and encoder forms,
// corr_enc_front.hip's stem and pointwise kernels, corr_lookup_conv.hip's forward and
// corr_mask_upsample.hip, selected per call by the C-ABI's `precision`)
// keep fewer of split3's pieces per operand, guards included, and multiply
// only the products among the kept ones (products<NP>() below):
//   bf16x6 (NP = 3, the default)  hi, mid, lo   six products:   no narrower than fp32
//   bf16x3 (NP = 2)               hi, mid       three products: operands to 2^-18, the dropped
//                                               wm xm to 2^-16 relative
//   bf16   (NP = 1)               hi            one product:    operands to 2^-9 relative
// The accumulators stay fp32 and the packs are the same in every mode (a reduced mode skips the
// pieces it does not keep), so an infinite operand still splits as (inf, 0, 0) and the non-finite
// pattern stays fp32's.
#pragma once

#include "corr_common.h"

namespace corr {

// ---------------------------------------------------------------------------------------
// The exact three-piece bf16 split (corr_build_bf16.hip's operands, lookup_conv_bwd's).
// ---------------------------------------------------------------------------------------
typedef __bf16 bf16s_pair __attribute__((ext_vector_type(2)));
typedef float bf16s_f32x2 __attribute__((ext_vector_type(2)));

// bf16 round-to-nearest-even of a pair, as fp32 values and as the packed pair.
__device__ __forceinline__ unsigned rn_pair(float a, float b, float &ha, float &hb) {
    const unsigned u = __builtin_bit_cast(unsigned, __builtin_convertvector(bf16s_f32x2{a, b}, bf16s_pair));
    ha = __builtin_bit_cast(float, u << 16);
    hb = __builtin_bit_cast(float, u & 0xffff0000u);
    return u;
}

// Split a pair of fp32 features into packed bf16 (hi, mid, lo) pairs, x = hi + mid + lo exactly.
// Guards: an infinite feature keeps hi = x and mid = lo = 0 (its hi*hi product is x * hi of the
// other operand; its products with the other operand's zero mid / lo pieces are NaN, which the
// consumers' split_sum discards when the hi*hi sum is infinite, corr_common.h); a finite feature
// whose hi rounds up past the bf16 range (|x| within 2^-9 of FLT_MAX) takes the truncated hi
// instead.  NaN propagates through hi.
__device__ __forceinline__ void split3(float a, float b, unsigned &hi, unsigned &mid, unsigned &lo) {
    float ha, hb;
    hi = rn_pair(a, b, ha, hb);
    if (__builtin_expect(__builtin_isinf(ha) | __builtin_isinf(hb), 0)) {
        const unsigned ua = __builtin_bit_cast(unsigned, a), ub = __builtin_bit_cast(unsigned, b);
        if (__builtin_isinf(ha) && !__builtin_isinf(a)) ha = __builtin_bit_cast(float, ua & 0xffff0000u);
        if (__builtin_isinf(hb) && !__builtin_isinf(b)) hb = __builtin_bit_cast(float, ub & 0xffff0000u);
        hi = (__builtin_bit_cast(unsigned, ha) >> 16) | (__builtin_bit_cast(unsigned, hb) & 0xffff0000u);
    }
    float ra = __builtin_isinf(a) ? 0.f : a - ha, rb = __builtin_isinf(b) ? 0.f : b - hb;
    float ma, mb;
    mid = rn_pair(ra, rb, ma, mb);
    float da, db;
    lo = rn_pair(ra - ma, rb - mb, da, db);  // exact: the residuals have <= 8 significant bits
}

// ---------------------------------------------------------------------------------------
// The MFMA and the family's K step.
// ---------------------------------------------------------------------------------------
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                  0, 0, 0);
}

// One K step of the forward kernels: the six piece products of W (wa = hi, mid, lo A fragments)
// and x (xb = hi, mid, lo B fragments), in THE order of the family — every forward kernel's
// arithmetic contract, pinned bit for bit by tests/test_bf16x6_family.py (inputs on which each
// output is one exactly representable product, so every piece product and every pack's pieces
// show in the last bit; its model of this function is tests/_bf16x6.py):
//   acs += wl xh;  acs += wh xl;  acs += wm xm;  acs += wm xh;  acs += wh xm;     acc += wh xh
// The five smaller products go to acs, smallest first, the leading one to acc; split_sum
// (corr_common.h) joins the two at the end.  (The lookup-conv backward's two GEMMs use orders of
// their own, written out where they are.)
__device__ __forceinline__ void six(const u32x4 (&wa)[3], const u32x4 (&xb)[3], f32x4 &acc, f32x4 &acs) {
    acs = mfma_bf16(wa[2], xb[0], acs);
    acs = mfma_bf16(wa[0], xb[2], acs);
    acs = mfma_bf16(wa[1], xb[1], acs);
    acs = mfma_bf16(wa[1], xb[0], acs);
    acs = mfma_bf16(wa[0], xb[1], acs);
    acc = mfma_bf16(wa[0], xb[0], acc);
}

// The K step of a kernel that keeps NP pieces per operand (wa, xb = the first NP of hi, mid, lo).
// NP = 3 is six() itself.  The orders of the reduced modes are part of the same contract (pinned
// by tests/test_precision.py, tests/test_encoder_precision.py and tests/test_pointwise_precision.py):
//   NP = 2 (bf16x3):  acs += wm xh;  acs += wh xm;     acc += wh xh      (six()'s order without
//                     the products that hold a lo piece, and without wm xm)
//   NP = 1 (bf16):    acc += wh xh                                       (acs is not touched: the
//                     kernel's result is acc alone)
template <int NP>
__device__ __forceinline__ void products(const u32x4 (&wa)[NP], const u32x4 (&xb)[NP], f32x4 &acc, f32x4 &acs) {
    static_assert(NP >= 1 && NP <= 3, "one, two or three pieces");
    if constexpr (NP == 3) {
        six(wa, xb, acc, acs);
    } else {
        if constexpr (NP == 2) {
            acs = mfma_bf16(wa[1], xb[0], acs);
            acs = mfma_bf16(wa[0], xb[1], acs);
        }
        acc = mfma_bf16(wa[0], xb[0], acc);
    }
}

// A pack kernel's store of one A fragment: dst = this lane's slot of the hi piece, the mid and lo
// pieces 64 lanes further each.
__device__ __forceinline__ void store_pieces(u32x4 *dst, const unsigned (&h)[4], const unsigned (&m)[4],
                                             const unsigned (&lo)[4]) {
    dst[0] = u32x4{h[0], h[1], h[2], h[3]};
    dst[64] = u32x4{m[0], m[1], m[2], m[3]};
    dst[128] = u32x4{lo[0], lo[1], lo[2], lo[3]};
}

// ---------------------------------------------------------------------------------------
// The tile of corr_conv.hip, corr_enc_front.hip and corr_flow.hip's encoder: a workgroup of 4
// waves owns 4 rows x 16 columns of one batch item's output; wave w owns the row blocks of half
// w & 1 and the tile rows 2 (w >> 1), + 1.  enc_finalize_kernel derives the pixel count of a
// tile's (sum, M2) statistics from these, so every kernel that writes statistics, and
// enc_stats_bytes, take them from here.
// ---------------------------------------------------------------------------------------
constexpr int kConvTW = 16, kConvTH = 4;  // pixel tile (columns x rows)
constexpr int kConvNT = 256;              // threads
constexpr int kConvPad = 64;              // the packs pad the rows to a multiple of this

}  // namespace corr
