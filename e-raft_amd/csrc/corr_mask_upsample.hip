// corr_mask_upsample.hip — the update block's mask head (the 256 -> 576 1x1 convolution mask[2]
// and its 0.25, model/update.py:99-107) fused with E-RAFT's convex upsampling (model/eraft.py:75-86)
// on gfx950, inference only: the 576-channel mask is never stored.
//
//   logit[k][i][j] = mask_scale * (bias[64k + 8i + j] + sum_c W[64k + 8i + j][c] hidden[n][off + c][y][x])
//   p = softmax over the 9 taps k (max-subtracted, tap order k = 0..8, as corr_convex_upsample)
//   out[n][ch][8y + i][8x + j] = sum_k p[k] * 8 flow[n][ch][y + k/3 - 1][x + k%3 - 1]   (0 outside the map)
//
// The logits are the implicit GEMM [576 x 256] x [256 x pixels] on the 16x16x32 bf16 MFMA with
// the build's exact three-piece split (x = hi + mid + lo, six products per fp32 product in
// the family's order (corr_bf16x6.h), two accumulators joined by split_sum: no narrower than fp32,
// no scales), K in ascending steps of 32 channels.
//
// Tap ownership: the 576 rows are 9 taps x 64 sub-pixels, so a wave that owns the nine 16-row
// blocks 64k + 16q .. + 15 (k = 0..8) of one sub-pixel range q holds, lane by lane, all nine
// logits of its (pixel, sub-pixel) pairs in accumulator registers: the softmax and the convex
// combination are a register-only epilogue (no LDS, no cross-lane traffic).  In the 16x16
// accumulator layout C[row = 4 (lane >> 4) + r][col = lane & 15] a lane's four rows are the
// sub-pixels 16q + 4g + r (g = lane >> 4), i.e. i = 2q + (g >> 1) and j = 4 (g & 1) + r: four
// consecutive j of one i, one 16-byte store per channel, and the 16 columns of a block are 16
// consecutive coarse pixels of a row, a contiguous 512-byte piece of an output row.
//
// Workgroup = 4 waves (wave = q) x kMuNP column blocks of 16 pixels (consecutive in the order
// batch item, row, block of the row; a partial block's pixels past W are computed from the
// clamped pixel W - 1 and neither stored nor used).  The blocks' 256 channels are loaded once,
// split and kept in LDS as bf16 pieces [piece][pixel][channel pair] for the workgroup's waves.
// The weights are pre-split once (mask_pack_kernel) into A-fragment order
// [q][K step][tap][piece][lane] (884736 bytes): a wave streams its quarter front to back from L2,
// kMuAhead steps ahead in a ring of registers.  The flow neighbours are loaded unconditionally from
// clamped addresses inside the pixel's own map and zeroed afterwards.  No atomics, no scratch,
// no workspace.
//
// Non-finite inputs give fp32's pattern (corr_conv.hip's note applies).
//
// `precision` (CORR_PREC_*) selects the kernel's NP: the reduced modes stage, fetch and multiply
// only the first two pieces (bf16x3, three products) or the first one (bf16, one product, one
// accumulator) of both operands, from the same pack (corr_bf16x6.h).  The softmax, the
// combination, the flow loads and the stores are the same in every mode.
#include "corr_bf16x6.h"
#include "corr_common.h"

namespace corr {
namespace {

constexpr int kMuK = 256;                 // input channels
constexpr int kMuTaps = 9;
constexpr int kMuKS = kMuK / 32;          // K steps
constexpr int kMuSteps = kMuKS * kMuTaps; // A fragments (of three pieces) a wave streams
constexpr int kMuNT = 256;                // threads: wave = sub-pixel range q
constexpr int kMuXS = kMuK / 2 + 4;       // words per LDS pixel: 128 channel pairs + pad (16-B rows)
// (DESIGN §17 has the variants measured: 1 block per workgroup, a 9-slot ring, 1 wave per SIMD)
constexpr int kMuNP = 2;                  // 16-pixel column blocks per workgroup
constexpr int kMuRing = 3;                // weight ring slots; divides the 9 steps of a K step
constexpr int kMuAhead = kMuRing - 1;     // steps the weight fragments run ahead
constexpr int kMuWaves = 2;               // waves per SIMD the kernel is compiled for (<= 256 registers)
constexpr int kMuPX = 16 * kMuNP;                 // pixels per workgroup
constexpr int kMuNLD = (kMuK / 2) * kMuPX / kMuNT;  // staging passes per thread
static_assert(kMuTaps % kMuRing == 0, "ring slots are compile-time");
static_assert(kMuNT % kMuPX == 0 && (kMuK / 2) % (kMuNT / kMuPX) == 0, "a thread stages one pixel");

// w [576][256] fp32 -> pieces [4 q][8 K steps][9 taps][hi, mid, lo][64 lanes] in the 16x16x32
// A-fragment order: lane = 16 kg + r holds W[64 tap + 16 q + r][32 step + 8 kg + j], j < 8.  One
// block per (step, 9 q + tap).
__global__ __launch_bounds__(64) void mask_pack_kernel(const float *__restrict__ w, u32x4 *__restrict__ frag) {
    const int ks = blockIdx.x, q = blockIdx.y / kMuTaps, k = blockIdx.y % kMuTaps, lane = threadIdx.x;
    const float *src = w + (size_t)(64 * k + 16 * q + (lane & 15)) * kMuK + 32 * ks + 8 * (lane >> 4);
    unsigned h[4], m[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split3(src[2 * j], src[2 * j + 1], h[j], m[j], lo[j]);
    u32x4 *dst = frag + ((size_t)(q * kMuKS + ks) * kMuTaps + k) * 3 * 64 + lane;
    store_pieces(dst, h, m, lo);
}

struct MaskUpArgs {
    const float *hidden;  // [B][hc][H][W]; channels off .. off + 255 are read
    const float *flow;    // [B][2][H][W]
    const float *bias;    // [576]
    const u32x4 *frag;    // the pack
    float *out;           // [B][2][8H][8W]
    float scale;
    int hc, off, H, W, nxb, tiles, vec;  // nxb blocks per row, tiles = B H nxb, vec: out is 16-B aligned
};

// NP: the pieces kept per operand (3 = bf16x6, 2 = bf16x3, 1 = bf16; products<NP>, corr_bf16x6.h).
// The pack is the same for every NP: a reduced mode skips the 1-KB runs of the pieces it drops.
template <int NP>
__global__ __launch_bounds__(kMuNT, kMuWaves) void mask_upsample_kernel(MaskUpArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned xs[NP][kMuPX][kMuXS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int H = g.H, W = g.W;
    const size_t HW = (size_t)H * W;

    // ---- A fragments: step s = 9 (K step) + tap of this wave's quarter of the pack ----
    const u32x4 *fq = g.frag + (size_t)q * kMuSteps * 3 * 64 + lane;
    auto load_a = [&](u32x4 (&wa)[NP], int s) {
        s = s < kMuSteps ? s : kMuSteps - 1;  // the last steps re-read the last fragment
#pragma unroll
        for (int p = 0; p < NP; ++p) wa[p] = fq[(size_t)(s * 3 + p) * 64];
    };
    u32x4 wa[kMuRing][NP];
#pragma unroll
    for (int s = 0; s < kMuAhead; ++s) load_a(wa[s], s);

    // ---- staging: this thread's pixel is px, its channel pairs cp0 + (kMuNT / kMuPX) i.  A block
    // past the last one re-reads the last block, a pixel past W the pixel W - 1: every address is
    // inside this launch's hidden, and what comes of them is never stored. ----
    {
        const int px = tid % kMuPX, cp0 = tid / kMuPX;
        int t = (int)blockIdx.x * kMuNP + (px >> 4);
        t = t < g.tiles ? t : g.tiles - 1;
        const int xb = t % g.nxb, ny = t / g.nxb, y = ny % H, n = ny / H;
        const int x = min(16 * xb + (px & 15), W - 1);
        const float *src = g.hidden + ((size_t)n * g.hc + g.off) * HW + (size_t)y * W + x;
        float v[kMuNLD][2];
#pragma unroll
        for (int i = 0; i < kMuNLD; ++i) {
            const size_t c = (size_t)(2 * (cp0 + (kMuNT / kMuPX) * i));
            v[i][0] = src[c * HW];
            v[i][1] = src[(c + 1) * HW];
        }
#pragma unroll
        for (int i = 0; i < kMuNLD; ++i) {
            unsigned hi, mid, lo;
            split3(v[i][0], v[i][1], hi, mid, lo);
            const int cp = cp0 + (kMuNT / kMuPX) * i;
            xs[0][px][cp] = hi;
            if constexpr (NP > 1) xs[1][px][cp] = mid;
            if constexpr (NP > 2) xs[2][px][cp] = lo;
        }
    }
    __syncthreads();

    // ---- the logits: acc[k][p] (hi * hi) and acs[k][p] (the five smaller products) ----
    const int fr = lane & 15, gq = lane >> 4, fk = 4 * gq;  // B fragment: pixel fr, channel pairs fk .. fk + 3
    f32x4 acc[kMuTaps][kMuNP], acs[kMuTaps][kMuNP];
#pragma unroll
    for (int k = 0; k < kMuTaps; ++k)
#pragma unroll
        for (int p = 0; p < kMuNP; ++p) acc[k][p] = acs[k][p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < kMuKS; ++ks) {
        u32x4 xb[kMuNP][NP];
#pragma unroll
        for (int p = 0; p < kMuNP; ++p)
#pragma unroll
            for (int c = 0; c < NP; ++c)
                xb[p][c] = *reinterpret_cast<const u32x4 *>(&xs[c][16 * p + fr][16 * ks + fk]);
#pragma unroll
        for (int k = 0; k < kMuTaps; ++k) {
            load_a(wa[(k + kMuAhead) % kMuRing], ks * kMuTaps + k + kMuAhead);
#pragma unroll
            for (int p = 0; p < kMuNP; ++p) products<NP>(wa[k % kMuRing], xb[p], acc[k][p], acs[k][p]);
        }
    }

    // ---- epilogue: lane (gq, fr) holds the nine logits of pixel fr at sub-pixels i, j0 .. j0 + 3 ----
    const int i = 2 * q + (gq >> 1), j0 = 4 * (gq & 1);
    float bs[kMuTaps][4];
#pragma unroll
    for (int k = 0; k < kMuTaps; ++k)
#pragma unroll
        for (int r = 0; r < 4; ++r) bs[k][r] = g.bias[64 * k + 8 * i + j0 + r];
#pragma unroll
    for (int p = 0; p < kMuNP; ++p) {
        const int t = (int)blockIdx.x * kMuNP + p;
        const bool live = t < g.tiles;
        const int tc = live ? t : g.tiles - 1;
        const int xb = tc % g.nxb, ny = tc / g.nxb, y = ny % H, n = ny / H;
        const int x = 16 * xb + fr, xc = min(x, W - 1);
        // (every load is unconditional, from an address inside this batch item's map; the zero of
        // a neighbour outside the map is applied afterwards)
        const float *f0 = g.flow + (size_t)n * 2 * HW, *f1 = f0 + HW;
        float u0[kMuTaps], u1[kMuTaps];
#pragma unroll
        for (int k = 0; k < kMuTaps; ++k) {
            const int yy = y + k / 3 - 1, xx = xc + k % 3 - 1;
            const size_t o = (size_t)min(max(yy, 0), H - 1) * W + min(max(xx, 0), W - 1);
            u0[k] = f0[o];
            u1[k] = f1[o];
        }
#pragma unroll
        for (int k = 0; k < kMuTaps; ++k) {
            const int yy = y + k / 3 - 1, xx = xc + k % 3 - 1;
            const bool in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
            u0[k] = in ? 8.0f * u0[k] : 0.0f;
            u1[k] = in ? 8.0f * u1[k] : 0.0f;
        }
        float a0[4], a1[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float lg[kMuTaps];
#pragma unroll
            for (int k = 0; k < kMuTaps; ++k)
                lg[k] = g.scale * (bs[k][r] + (NP == 1 ? acc[k][p][r] : split_sum(acc[k][p][r], acs[k][p][r])));
            float mx = lg[0];
#pragma unroll
            for (int k = 1; k < kMuTaps; ++k) mx = fmaxf(mx, lg[k]);
            float e[kMuTaps], s = 0.0f;
#pragma unroll
            for (int k = 0; k < kMuTaps; ++k) {
                e[k] = expf(lg[k] - mx);
                s += e[k];
            }
            a0[r] = a1[r] = 0.0f;
#pragma unroll
            for (int k = 0; k < kMuTaps; ++k) {
                const float pk = e[k] / s;
                a0[r] += pk * u0[k];
                a1[r] += pk * u1[k];
            }
        }
        if (!live || x >= W) continue;
        const size_t W8 = (size_t)8 * W, H8 = (size_t)8 * H;
        float *o0 = g.out + ((size_t)n * 2 * H8 + 8 * y + i) * W8 + 8 * (size_t)x + j0, *o1 = o0 + H8 * W8;
        if (g.vec) {  // uniform
            *reinterpret_cast<f32x4 *>(o0) = f32x4{a0[0], a0[1], a0[2], a0[3]};
            *reinterpret_cast<f32x4 *>(o1) = f32x4{a1[0], a1[1], a1[2], a1[3]};
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                o0[r] = a0[r];
                o1[r] = a1[r];
            }
        }
    }
}

}  // namespace

size_t mask_upsample_weights_bytes() { return (size_t)4 * kMuSteps * 3 * 64 * sizeof(u32x4); }

hipError_t launch_mask_upsample_pack(const float *w, void *packed, hipStream_t s) {
    hipLaunchKernelGGL(mask_pack_kernel, dim3(kMuKS, 4 * kMuTaps), dim3(64), 0, s, w, static_cast<u32x4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_mask_upsample(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                                const void *packed, const float *bias, float mask_scale, int B, int H, int W,
                                float *out, hipStream_t s, int precision) {
    if (!precision_supported(precision)) return hipErrorInvalidValue;
    MaskUpArgs g{};
    g.hidden = hidden, g.flow = flow, g.bias = bias, g.frag = static_cast<const u32x4 *>(packed), g.out = out;
    g.scale = mask_scale, g.hc = hidden_channels, g.off = hidden_offset, g.H = H, g.W = W;
    g.nxb = (W + 15) / 16;
    g.tiles = B * H * g.nxb;  // <= B H W < 2^31
    g.vec = (uintptr_t)out % 16 == 0;  // (8W floats per output row: every row then is 16-B aligned)
    const dim3 grid((unsigned)((g.tiles + kMuNP - 1) / kMuNP)), block(kMuNT);
    switch (precision) {
        case 1: hipLaunchKernelGGL(mask_upsample_kernel<2>, grid, block, 0, s, g); break;
        case 2: hipLaunchKernelGGL(mask_upsample_kernel<1>, grid, block, 0, s, g); break;
        default: hipLaunchKernelGGL(mask_upsample_kernel<3>, grid, block, 0, s, g);
    }
    return hipGetLastError();
}

}  // namespace corr
