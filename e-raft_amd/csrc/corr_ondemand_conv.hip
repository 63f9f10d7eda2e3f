// corr_ondemand_conv.hip — the on-demand window lookup (corr_ondemand.hip) fused with the
// consumer's 1x1 convolution on gfx950: out = relu(convc1(on-demand lookup)) in ONE launch, the
// 324-channel lookup never reaches HBM.  r = 4, L <= 4, O = 256; inference only.
//
// A workgroup of 4 waves owns one 8 x 8 block of queries of one batch item and walks the levels
// l = 0 .. L-1 itself (grid = blocks x B, no level dimension).  Per level it runs the tiled
// lookup's phases A-D (od_tiled_block, corr_ondemand_block.h: the same statements as
// ondemand_lookup_tiled_kernel, the same route choice per (block, level), od_general_query for
// the blocks that are not tiled), whose results go to an LDS tile ct[q][l 81 + i 9 + j] instead
// of global memory: the values entering the convolution are corr_ondemand_lookup's bit for bit.
// Then out[b][o][n] = (relu?)(bias[o] + sum_c W[o][c] ct[n][c]) on v_mfma_f32_16x16x32_bf16 with
// the family's exact three-piece split and six() (corr_bf16x6.h), in lookup_conv_kernel's K
// order: K = L 81 padded with zeros to 352, 11 steps of 32, the two accumulators joined by
// split_sum.  W's pieces are corr_lookup_conv_weights' pack (A fragments, streamed from L2 one K
// step ahead).  Wave w owns output channels [64 w, 64 w + 64).
//
// ct is query-major with a row stride of 356 words (= 36 mod 64 banks): a lane's B fragment —
// query lane & 15, k = 32 kc + 8 (lane >> 4) .. + 7 — is two ds_read_b128 of consecutive words.
// Two forms of the product (kOcPresplit, DESIGN §21's variants table):
//   0  all 64 queries at once (128 accumulator registers); every wave splits the B fragments it
//      reads (each value is split by all four waves), W is streamed once;
//   1  two halves of 32 queries; the workgroup first splits the half once into bf16 pieces
//      x[piece][q][k pair] that alias the lookup's staging (lookup_conv_kernel's layout), W is
//      streamed once per half.
// No atomics, no scratch, no allocation; deterministic (the route is a function of the
// coordinates only, the summation order is fixed).
#include <cmath>

#include "corr_bf16x6.h"
#include "corr_common.h"
#include "corr_ondemand_block.h"

#ifndef CORR_OD_CONV_PRESPLIT
#define CORR_OD_CONV_PRESPLIT 1  // the faster at 160 x 240 with coherent coordinates
#endif

namespace corr {
namespace {

constexpr int kOcPresplit = CORR_OD_CONV_PRESPLIT;
constexpr int kOcO = 256, kOcK = 81, kOcKC = 11, kOcKP = 32 * kOcKC /* 352 >= 4*81 */;
constexpr int kOcCS = kOcKP + 4;      // ct row stride (words): 16-B aligned rows, 36 mod 64 banks
constexpr int kOcXS = kOcKP / 2 + 4;  // piece row stride (k pairs), as lookup_conv_kernel's
constexpr int kOcHQ = kTlQ / 2;       // queries per half (form 1)

struct OcSmem {
    union {
        TlSmem tl;                    // the lookups
        unsigned x[3][kOcHQ][kOcXS];  // form 1: a half's pieces (after the lookups)
    } u;
    float ct[kTlQ][kOcCS];  // the block's lookup [q][l 81 + i 9 + j], zero from L 81 to 352
};
static_assert(sizeof(OcSmem) <= 160 * 1024, "one workgroup per CU: all of it fits in the CU's LDS");

// od_tiled_block's results -> ct (ct = the block's row 0 at this level's first channel).
struct OcStoreCt {
    float *ct;
    __device__ __forceinline__ void general(int t, int, int, int q, float v) const { ct[q * kOcCS + t] = v; }
    __device__ __forceinline__ auto column(int, int, int q, int i) const {
        float *o = ct + q * kOcCS + i * 9;
        return [o](int j, float v) { o[j] = v; };
    }
};

// W's A fragments of K step kc for the wave's four o-tiles.
__device__ __forceinline__ void oc_load_a(const u32x4 *__restrict__ frag, int w, int lane, int kc, u32x4 (&wa)[4][3]) {
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const size_t base = (((size_t)(4 * w + t) * kOcKC + kc) * 3) * 64 + lane;
#pragma unroll
        for (int p = 0; p < 3; ++p) wa[t][p] = frag[base + 64 * p];
    }
}

// C[row = o][col = q] = acc[4 (lane >> 4) + r][lane & 15] of o-tile t and the query tile at q0.
__device__ __forceinline__ void oc_store(const f32x4 &acc, const f32x4 &acs, int o0, int q, int b, int qy0, int qx0,
                                         int H, int W, const float *__restrict__ bias, int relu,
                                         float *__restrict__ out) {
    const int qy = qy0 + (q >> 3), qx = qx0 + (q & 7);
    if (qy >= H || qx >= W) return;  // a partial block's queries outside the image write nothing
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = o0 + r;
        float v = split_sum(acc[r], acs[r]) + bias[o];
        if (relu && v < 0.0f) v = 0.0f;  // torch.relu: a NaN stays a NaN (fmaxf would drop it)
        __builtin_nontemporal_store(v, &out[((size_t)b * kOcO + o) * ((size_t)H * W) + qy * W + qx]);
    }
}

// The wave's 64 x (16 NC) x 352 product: acc / acs [o-tile][query tile] from zero, K steps in
// order, W's fragments one step ahead (two buffers, the loop rolled in pairs of steps so that
// only two are ever live).  load_b(kc, c, xb) gives query tile c's B fragments of step kc.
template <int NC, class LoadB>
__device__ __forceinline__ void oc_product(const u32x4 *__restrict__ frag, int w, int lane, f32x4 (&acc)[4][NC],
                                           f32x4 (&acs)[4][NC], LoadB load_b) {
    static_assert(kOcKC % 2 == 1, "pairs of steps, then the last one from the first buffer");
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[t][c] = acs[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    u32x4 wa0[4][3], wa1[4][3];  // [o-tile][piece]
    auto step = [&](int kc, const u32x4 (&wa)[4][3]) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            u32x4 xb[3];
            load_b(kc, c, xb);
#pragma unroll
            for (int t = 0; t < 4; ++t) six(wa[t], xb, acc[t][c], acs[t][c]);
        }
    };
    oc_load_a(frag, w, lane, 0, wa0);
#pragma unroll 1
    for (int kc = 0; kc + 2 < kOcKC; kc += 2) {
        oc_load_a(frag, w, lane, kc + 1, wa1);
        step(kc, wa0);
        oc_load_a(frag, w, lane, kc + 2, wa0);
        step(kc + 1, wa1);
    }
    step(kOcKC - 1, wa0);
}

__global__ __launch_bounds__(256) void ondemand_lookup_conv_kernel(OdArgs a, int general,
                                                                    const u32x4 *__restrict__ frag,
                                                                    const float *__restrict__ bias, int relu,
                                                                    float *__restrict__ out) {
    __shared__ OcSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int W = a.W, H = a.H;
    const int bw8 = (W + 7) >> 3, bh8 = (H + 7) >> 3;
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x / (bw8 * bh8));
    const int blk = blockIdx.x - b * bw8 * bh8;
    const int qy0 = (blk / bw8) * 8, qx0 = (blk % bw8) * 8;
    const int KC = a.L * kOcK, KZ = kOcKP - KC;
    // the K padding: zero for every query (the pack's zeros times a stale NaN would be NaN); the
    // rows of queries outside the image stay unwritten — a column of the product reaches only
    // its own query's outputs, which are not stored
    for (int idx = tid; idx < kTlQ * KZ; idx += 256) {
        const int q = idx / KZ, k = KC + (idx - q * KZ);
        sm.ct[q][k] = 0.f;
    }
    // ---- the lookups, level by level -> ct ----
#pragma unroll 1
    for (int l = 0; l < a.L; ++l) {
        const OdLevel lv = od_level(a, b, l);
        od_tiled_block(sm.u.tl, a, lv, b, qy0, qx0, general != 0, OcStoreCt{&sm.ct[0][l * kOcK]});
    }
    __syncthreads();  // ct complete; the staging is free
    // ---- 256 x 64 x 352 product: wave w owns output channels [64 w, 64 w + 64) ----
    const int fr = lane & 15, kg = lane >> 4;  // B fragment: query fr of the tile, k = 8 kg .. + 7 of the step
    if constexpr (!kOcPresplit) {
        f32x4 acc[4][4], acs[4][4];  // [o-tile][query tile]
        oc_product<4>(frag, w, lane, acc, acs, [&](int kc, int c, u32x4 (&xb)[3]) {
            const float *src = &sm.ct[16 * c + fr][32 * kc + 8 * kg];
            const f32x4 y0 = *reinterpret_cast<const f32x4 *>(src);
            const f32x4 y1 = *reinterpret_cast<const f32x4 *>(src + 4);
            unsigned h[4], m[4], lo[4];
            split3(y0[0], y0[1], h[0], m[0], lo[0]);
            split3(y0[2], y0[3], h[1], m[1], lo[1]);
            split3(y1[0], y1[1], h[2], m[2], lo[2]);
            split3(y1[2], y1[3], h[3], m[3], lo[3]);
            xb[0] = u32x4{h[0], h[1], h[2], h[3]};
            xb[1] = u32x4{m[0], m[1], m[2], m[3]};
            xb[2] = u32x4{lo[0], lo[1], lo[2], lo[3]};
        });
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                oc_store(acc[t][c], acs[t][c], 64 * w + 16 * t + 4 * kg, 16 * c + fr, b, qy0, qx0, H, W, bias, relu,
                         out);
    } else {
#pragma unroll 1
        for (int hq = 0; hq < 2; ++hq) {
            if (hq) __syncthreads();  // the first half's MFMAs have read x
            // ---- the half's pieces x[piece][q][k pair]: lanes along k (conflict-free both ways) ----
            for (int idx = tid; idx < kOcHQ * (kOcKP / 2); idx += 256) {
                const int q = idx / (kOcKP / 2), kp = idx - q * (kOcKP / 2);
                const float *src = &sm.ct[kOcHQ * hq + q][2 * kp];
                unsigned h, m, lo;
                split3(src[0], src[1], h, m, lo);
                sm.u.x[0][q][kp] = h;
                sm.u.x[1][q][kp] = m;
                sm.u.x[2][q][kp] = lo;
            }
            __syncthreads();
            f32x4 acc[4][2], acs[4][2];
            oc_product<2>(frag, w, lane, acc, acs, [&](int kc, int c, u32x4 (&xb)[3]) {
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    xb[p] = *reinterpret_cast<const u32x4 *>(&sm.u.x[p][16 * c + fr][16 * kc + 4 * kg]);
            });
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    oc_store(acc[t][c], acs[t][c], 64 * w + 16 * t + 4 * kg, kOcHQ * hq + 16 * c + fr, b, qy0, qx0, H, W,
                             bias, relu, out);
        }
    }
}

}  // namespace

hipError_t launch_ondemand_lookup_conv(const void *ws, const float *coords, int B, int D, int H, int W, int levels,
                                       int radius, int flags, const void *packed, const float *bias, int relu,
                                       float *out, hipStream_t s) {
    if (radius != 4 || levels < 1 || levels > 4) return hipErrorInvalidValue;  // E-RAFT: r = 4, L <= 4
    const OdLayout lay = ondemand_offsets(B, D, H, W, levels);
    const float *base = (const float *)ws;
    OdArgs a{};
    a.F1 = (const f32x4 *)(base + lay.f1);
    for (int l = 0; l < levels; ++l) a.P[l] = (const f32x4 *)(base + lay.p[l]);
    a.coords = coords, a.out = nullptr;
    a.B = B, a.N = H * W, a.H = H, a.W = W, a.L = levels, a.D4 = padded_d(D) / 4, a.S = 2 * radius + 1;
    a.sqrtD = std::sqrt((float)D);
    const unsigned nblk = (unsigned)(((W + 7) / 8) * ((H + 7) / 8));
    hipLaunchKernelGGL(ondemand_lookup_conv_kernel, dim3(nblk * (unsigned)B), dim3(256), 0, s, a,
                       (flags & CORR_ONDEMAND_GENERAL) ? 1 : 0, static_cast<const u32x4 *>(packed), bias, relu, out);
    return hipGetLastError();
}

}  // namespace corr
