// corr_conv.hip — a 3x3 convolution (padding 1, stride 1) with bias and an optional ReLU on
// gfx950, inference only: the update block's convc2, convf2, conv and the two heads' first
// convolutions (model/update.py:63-107); and its forms for the encoders' residual stages.
//
//   out[b][out_offset + o][y][x] = act(bias[o] + sum_c sum_ky sum_kx w[o][c][ky][kx] in[b][c][y+ky-1][x+kx-1])
//
// o < cout, zero outside the map, act = identity or ReLU.  `in` is the channel-wise concatenation
// of in_a (ca channels) and in_b (cb channels, may be absent) and is never materialised: a
// 32-channel chunk comes from one pointer or the other (ca and cb are multiples of 32, the
// boundary is anywhere).  `out` has out_channels channels of which only out_offset .. + cout - 1
// are written, so a producer writes straight into the buffer its consumer reads (no cat).
//
// The arithmetic is corr_gru.hip's: the implicit GEMM
//   out[o][pixel] = sum_chunk sum_tap sum_{c in chunk} W[o][c][tap] * in[c][pixel + tap offset]
// with K = 9 cin in steps of 32 channels (channel chunk outer, tap inner, ky major and kx minor: a
// fixed order), on the 16x16x32 bf16 MFMA with the build's exact three-piece split (x = hi +
// mid + lo, six products per fp32 product in the family's order, corr_bf16x6.h, two accumulators
// joined by split_sum: no narrower than fp32, no scales).
//
// Workgroup = 4 waves = 32 output rows x one tile of 4 rows x 16 columns of one batch item's
// map; wave w owns rows 16 (w & 1) .. + 16 and tile rows 2 (w >> 1), + 1 (one 16x16 output tile
// by two pixel tiles, 4 accumulators; the GRU kernel's 64 rows per workgroup measured slower
// here: at DSEC they leave most CUs one workgroup or none).  Per channel chunk the
// workgroup stages the tile plus its 1-pixel halo on all four sides (6 x 18 positions; zero
// outside the map, so a halo never reads the neighbouring row, map or batch item) from fp32
// global memory through split3 into LDS as bf16 pieces [piece][position][channel pair]; 108
// positions x 16 channel pairs are 6.75 passes of 256 threads, so the seventh pass is guarded
// (only wave 3 sits it out: the guard is wave-uniform).  The next chunk's values are loaded into registers two chunks ahead.  The B
// fragment of tap (ky, kx) is the same LDS tile read at the position offset 18 ky + kx.  The
// weights are pre-split once (conv_pack_kernel) into A-fragment order
// [16-row block][chunk][tap][piece][lane], rows padded with zeros to a multiple of 64 (padding
// rows are computed and never stored), and streamed from L2 kConvAhead K steps ahead in a ring.
// No atomics, no scratch, nothing allocated.
//
// The same kernel is a template <STRIDE, NORM_IN, STATS> for the encoders' residual stages
// (model/extractor.py:7-52; launch_enc_conv): stride 2 (a 9 x 33 window, staged by
// another thread-to-word map), a per-channel affine + ReLU applied while staging (the norm of the
// producing convolution, "norm on load"), and per-tile (sum, M2) statistics of the output for that
// norm, merged by enc_finalize_kernel; enc_join_kernel is the block's normalise + add + ReLU.
// <1, false, false> is the kernel described above, unchanged in its arithmetic.
//
// Non-finite inputs give fp32's pattern (an infinite operand splits as (inf, 0, 0) and split_sum
// keeps the infinite leading sum; tests/test_bf16x6_family.py); finite inputs give finite outputs.
//
// `precision` (CORR_PREC_*) selects NP, for the update block's form <1, false, false> and for the
// encoder forms alike: the reduced modes stage, fetch and multiply only the first two pieces
// (bf16x3, three products) or the first one (bf16, one product, one accumulator) of both operands,
// from the same pack (corr_bf16x6.h).  The on-load norm is applied before the
// split and the statistics are those of the launch's own output, in every mode.
#include <type_traits>

#include "corr_bf16x6.h"
#include "corr_common.h"

namespace corr {
namespace {

// (the pixel tile kConvTW x kConvTH, kConvNT threads and the packs' row padding kConvPad are the
// family's: corr_bf16x6.h)
// The staged window of a 4 x 16 output tile at stride S: S (t - 1) + 3 positions a side.
template <int S>
struct ConvGeo {
    static constexpr int PW = kConvTW * S + 3 - S;             // staged positions per row: 18 / 33
    static constexpr int PH = kConvTH * S + 3 - S;             // staged rows: 6 / 9
    static constexpr int NPOS = PW * PH;                       // 108 / 297
    static constexpr int Stage = NPOS * 16;                    // staged words per piece and chunk: 1728 / 4752
    // Staging passes per thread.  Stride 1: word idx = tid + 256 i of the chunk's Stage words, 7
    // passes, the last guarded.  Stride 2: a wave owns 4 channel pairs and a lane the positions
    // lane + 64 i, i < NPP = 5 (the last guarded), so only NPP positions' bookkeeping is live and
    // the channel pair is wave-uniform: 19 passes of the stride-1 scheme would hold 4 registers of
    // it each.
    static constexpr int NPP = S == 1 ? 0 : (NPOS + 63) / 64;
    static constexpr int NLD = S == 1 ? (Stage + 256 - 1) / 256 : 4 * NPP;
    static constexpr int Ahead = S == 1 ? 2 : 1;               // chunks the activation registers run ahead
};
constexpr int kConvT = 1;                      // 16-row blocks per wave (2 measured slower)
constexpr int kConvOB = 32 * kConvT;           // output rows per workgroup
constexpr int kConvXS = 16 + 4;                // words per LDS position: 16 channel pairs + pad (16-B rows)
constexpr int kConvTaps = 9;
// Waves per SIMD the kernel is compiled for, by the pieces it keeps (2: <= 256 registers; 3: <= 168).
// One piece needs 144 registers; two pieces need 186 and spill at 168.  The encoder
// forms take the third wave where the resource report shows that they fit.
constexpr int conv_waves(int np, int stride = 1) { return np == 1 && stride == 1 ? 3 : 2; }
constexpr int kConvRing = 6;                   // weight ring slots; divides the 18 K steps of a chunk pair
constexpr int kConvAhead = 5;                  // K steps the weight fragments run ahead (< kConvRing)
constexpr int kConvMaxCin = 1024;              // conv_supported's bound (the norm-on-load table in LDS)
static_assert((2 * kConvTaps) % kConvRing == 0 && kConvAhead < kConvRing, "ring slots are compile-time");
static_assert(kConvNT == 256 && ConvGeo<1>::Stage - (ConvGeo<1>::NLD - 1) * kConvNT > 0 &&
                  (ConvGeo<1>::Stage - (ConvGeo<1>::NLD - 1) * kConvNT) % 64 == 0,
              "the guard of the last staging pass is wave-uniform at stride 1");

// w [cout][cin][3][3] fp32 -> pieces [rows/16 blocks][cin/32 chunks][9 taps][hi, mid, lo][64 lanes]
// in the 16x16x32 A-fragment order: lane = 16 kg + r holds W[16 ob + r][32 chunk + 8 kg + j][tap],
// j < 8; rows >= cout are zero.  One block per (chunk, ob).
__global__ __launch_bounds__(64) void conv_pack_kernel(const float *__restrict__ w, int cout, int cin,
                                                       u32x4 *__restrict__ frag) {
    const int ch = blockIdx.x, ob = blockIdx.y, lane = threadIdx.x;
    const int row = 16 * ob + (lane & 15), c0 = 32 * ch + 8 * (lane >> 4);
    const bool live = row < cout;
    const float *src = w + ((size_t)(live ? row : 0) * cin + c0) * kConvTaps;
    const int NC = cin / 32;
#pragma unroll
    for (int t = 0; t < kConvTaps; ++t) {
        unsigned h[4], m[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float a = src[(2 * j) * kConvTaps + t], b = src[(2 * j + 1) * kConvTaps + t];
            split3(live ? a : 0.f, live ? b : 0.f, h[j], m[j], lo[j]);
        }
        u32x4 *dst = frag + ((((size_t)ob * NC + ch) * kConvTaps + t) * 3) * 64 + lane;
        store_pieces(dst, h, m, lo);
    }
}

struct ConvArgs {
    const float *a;      // channels < ca of the input
    const float *b;      // the other cb channels (unused when cb == 0)
    const float *bias;   // [cout], or null for no bias
    const u32x4 *frag;   // the pack
    float *out;          // [B][oc][Ho][Wo]; channels off .. off + cout - 1 are written
    const float *scale;  // NORM_IN: [B][cin] (nb = 1) or [cin] (nb = 0)
    const float *shift;
    float *stats;        // STATS: [B][cout][tiles][2]
    int B, ca, cb, H, W, cout, relu, oc, off, tx, ty, nb;
};

// STRIDE 1 or 2 (padding 1, Ho = (H - 1) / STRIDE + 1; tx, ty tile the output).  NORM_IN: a staged
// value is relu(in * scale[c] + shift[c]) (two fp32 ops, each rounded), and the zero of a position
// outside the map is applied after it: the padding is zero in the normalised domain.  STATS: no
// ReLU, and the workgroup leaves (sum, M2 about the tile's own mean) of its valid pixels per
// output channel (header: corr_enc_conv_forward).
// NP: the pieces kept per operand (3 = bf16x6, 2 = bf16x3, 1 = bf16: products<NP>, corr_bf16x6.h).
// The pack is the same for every NP: a reduced mode skips the 1-KB runs of the pieces it drops.
template <int STRIDE, bool NORM_IN, bool STATS, int NP = 3>
__global__ __launch_bounds__(kConvNT, conv_waves(NP, STRIDE)) void conv_kernel(ConvArgs g) {
    using G = ConvGeo<STRIDE>;
    constexpr int kConvPW = G::PW, kConvNPOS = G::NPOS, kConvStage = G::Stage, kConvNLD = G::NLD;
    __shared__ __attribute__((aligned(16))) unsigned xs[NP][kConvNPOS][kConvXS];
    __shared__ float nrm[NORM_IN ? 2 * kConvMaxCin : 1];  // scale | shift of this batch item's channels
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = g.H, W = g.W;
    const int Ho = STRIDE == 1 ? H : (H - 1) / STRIDE + 1, Wo = STRIDE == 1 ? W : (W - 1) / STRIDE + 1;
    const size_t HW = (size_t)H * W;
    const int tiles = g.tx * g.ty;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int y0 = (tl / g.tx) * kConvTH, x0 = (tl % g.tx) * kConvTW;
    const int NC = (g.ca + g.cb) / 32, NS = NC * kConvTaps;

    if constexpr (NORM_IN) {
        const int cin = g.ca + g.cb;
        const size_t base = g.nb ? (size_t)b * cin : 0;
        for (int c = tid; c < cin; c += kConvNT) {
            nrm[c] = g.scale[base + c];
            nrm[kConvMaxCin + c] = g.shift[base + c];
        }
        __syncthreads();
    }

    // ---- staging: pass i of this thread is channel pair kp[i] at position ps[i] (stride 2: pass
    // 5 k + i is channel pair 4 w + k at position ps[i]) ----
    constexpr int kConvNB = STRIDE == 1 ? kConvNLD : G::NPP;  // passes with bookkeeping of their own
    int ps[kConvNB];
    [[maybe_unused]] int kp[STRIDE == 1 ? kConvNLD : 1];
    long off[kConvNB];   // float offset inside a batch item's chunk (0 for a position outside the map)
    unsigned inmap = 0;  // bit i: pass i's position is inside the map (else its values are zero)
    static_assert(kConvNB <= 32, "one inmap bit per pass");
    [[maybe_unused]] const int wu = __builtin_amdgcn_readfirstlane(w);
#pragma unroll
    for (int i = 0; i < kConvNB; ++i) {
        bool live;
        long plane = 0;
        if constexpr (STRIDE == 1) {
            const int idx = tid + kConvNT * i;
            live = idx < kConvStage;  // false only in the last pass
            kp[i] = live ? idx / kConvNPOS : 0;
            ps[i] = live ? idx - kp[i] * kConvNPOS : 0;
            plane = (long)(2 * kp[i]) * (long)HW;
        } else {
            live = lane + 64 * i < kConvNPOS;  // false only in the last pass
            ps[i] = live ? lane + 64 * i : 0;
        }
        const int y = STRIDE * y0 + ps[i] / kConvPW - 1, x = STRIDE * x0 + ps[i] % kConvPW - 1;
        const bool in = live && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        off[i] = in ? plane + (long)y * W + x : 0;
        inmap |= (unsigned)in << i;
    }
    // (every load is unconditional, from a valid address, and the zero of a position outside the
    // map is applied at the split: a select on the loaded value would wait for it right here)
    auto load_chunk = [&](int ch, float (&v)[kConvNLD][2]) {
        const int c0 = 32 * ch;
        const float *src = c0 < g.ca ? g.a + ((size_t)b * g.ca + c0) * HW : g.b + ((size_t)b * g.cb + (c0 - g.ca)) * HW;
        if constexpr (STRIDE == 1) {
#pragma unroll
            for (int i = 0; i < kConvNLD; ++i) {
                v[i][0] = src[off[i]];
                v[i][1] = src[off[i] + HW];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float *sk = src + (size_t)(2 * (4 * wu + k)) * HW;
#pragma unroll
                for (int i = 0; i < G::NPP; ++i) {
                    v[G::NPP * k + i][0] = sk[off[i]];
                    v[G::NPP * k + i][1] = sk[off[i] + HW];
                }
            }
        }
    };

    // ---- A fragments: row blocks ob0 .. ob0 + kConvT - 1 of the pack, K step s = 9 chunk + tap ----
    const int ob0 = (int)blockIdx.y * (kConvOB / 16) + kConvT * (w & 1);
    auto load_a = [&](u32x4 (&wa)[kConvT][NP], int s) {
        s = s < NS ? s : NS - 1;  // the last steps re-read the last fragment
#pragma unroll
        for (int t = 0; t < kConvT; ++t) {
            const size_t base = ((size_t)(ob0 + t) * NS + s) * 3 * 64 + lane;
#pragma unroll
            for (int p = 0; p < NP; ++p) wa[t][p] = g.frag[base + 64 * p];
        }
    };

    const int fr = lane & 15, fk = 4 * (lane >> 4);  // B fragment: column fr, channel pairs fk .. fk + 3
    const int j0 = 2 * (w >> 1);                     // this wave's tile rows j0, j0 + 1
    f32x4 acc[kConvT][2], acs[kConvT][2];
#pragma unroll
    for (int t = 0; t < kConvT; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[t][c] = acs[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The weights run kConvAhead K steps ahead of the products in a ring (step s lives in slot
    // s % kConvRing; a pair of chunks is 18 steps, so the slot of (chunk parity, tap) is a
    // constant), the activations two chunks ahead in two register sets: at DSEC a CU holds one or
    // two workgroups, too few to hide an L2 round trip per step.  (Stride 2 stages 2.75 times as
    // many values per chunk and keeps one set, one chunk ahead.)
    u32x4 wa[kConvRing][kConvT][NP];
    float va[kConvNLD][2];
    [[maybe_unused]] float vb[G::Ahead == 2 ? kConvNLD : 1][2];
    load_chunk(0, va);
    if constexpr (G::Ahead == 2) load_chunk(NC > 1 ? 1 : 0, vb);
#pragma unroll
    for (int s = 0; s < kConvAhead; ++s) load_a(wa[s], s);
    auto chunk = [&](int ch, auto par, float (&v)[kConvNLD][2]) {
        constexpr int S0 = decltype(par)::value * kConvTaps;  // this chunk's first step, mod the ring
#pragma unroll
        for (int i = 0; i < kConvNLD; ++i) {
            unsigned hi, mid, lo;
            const int ib = STRIDE == 1 ? i : i % (G::NPP ? G::NPP : 1);  // this pass's bookkeeping
            const int kpi = STRIDE == 1 ? kp[STRIDE == 1 ? i : 0] : 4 * wu + i / (G::NPP ? G::NPP : 1);
            const bool in = (inmap >> ib) & 1;
            float p = v[i][0], q = v[i][1];
            if constexpr (NORM_IN) {
                const int c = 32 * ch + 2 * kpi;
                p = p * nrm[c] + nrm[kConvMaxCin + c];
                q = q * nrm[c + 1] + nrm[kConvMaxCin + c + 1];
                p = p < 0.f ? 0.f : p;
                q = q < 0.f ? 0.f : q;
            }
            split3(in ? p : 0.f, in ? q : 0.f, hi, mid, lo);
            if (STRIDE == 1 ? i + 1 < kConvNLD || tid + kConvNT * i < kConvStage
                            : ib + 1 < G::NPP || lane + 64 * ib < kConvNPOS) {
                xs[0][ps[ib]][kpi] = hi;
                if constexpr (NP > 1) xs[1][ps[ib]][kpi] = mid;
                if constexpr (NP > 2) xs[2][ps[ib]][kpi] = lo;
            }
        }
        __syncthreads();
        load_chunk(ch + G::Ahead < NC ? ch + G::Ahead : NC - 1, v);  // (past the end: a harmless re-read)
#pragma unroll
        for (int tap = 0; tap < kConvTaps; ++tap) {
            load_a(wa[(S0 + tap + kConvAhead) % kConvRing], ch * kConvTaps + tap + kConvAhead);
            const int tp = (tap / 3) * kConvPW + tap % 3;
            u32x4 xb[2][NP];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    xb[c][p] = *reinterpret_cast<const u32x4 *>(
                        &xs[p][STRIDE * ((j0 + c) * kConvPW + fr) + tp][fk]);
#pragma unroll
            for (int t = 0; t < kConvT; ++t)
#pragma unroll
                for (int c = 0; c < 2; ++c) products<NP>(wa[(S0 + tap) % kConvRing][t], xb[c], acc[t][c], acs[t][c]);
        }
        __syncthreads();
    };
    int ch = 0;
#pragma unroll 1
    for (; ch + 1 < NC; ch += 2) {
        chunk(ch, std::integral_constant<int, 0>{}, va);
        if constexpr (G::Ahead == 2)
            chunk(ch + 1, std::integral_constant<int, 1>{}, vb);
        else
            chunk(ch + 1, std::integral_constant<int, 1>{}, va);
    }
    if (ch < NC) chunk(ch, std::integral_constant<int, 0>{}, va);

    // ---- epilogue: C[row = 4 (lane >> 4) + r][col = lane & 15] ----
    const size_t HWo = (size_t)Ho * Wo;
    const int x = x0 + fr;
    if constexpr (!STATS) {
        if (x >= Wo) return;
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const int y = y0 + j0 + c;
            if (y >= Ho) continue;
            const size_t n = (size_t)y * Wo + x;
#pragma unroll
            for (int t = 0; t < kConvT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = (int)blockIdx.y * kConvOB + 16 * kConvT * (w & 1) + 16 * t + 4 * (lane >> 4) + r;
                    if (row >= g.cout) continue;  // a padding row of the pack
                    float v = NP == 1 ? acc[t][c][r] : split_sum(acc[t][c][r], acs[t][c][r]);
                    if (g.bias) v = v + g.bias[row];
                    if (g.relu) v = v < 0.f ? 0.f : v;
                    g.out[((size_t)b * g.oc + g.off + row) * HWo + n] = v;
                }
        }
    } else {
        // A copy of front_epilogue<1, true> (corr_enc_front.hip, where it is described) that writes
        // the channel window; kept in step with it by hand, see there.
        static_assert(kConvT == 1, "the statistics epilogue is written for one row block per wave");
        float *red = reinterpret_cast<float *>(&xs[0][0][0]);  // [half][32 rows][sum, M2]; the tile is consumed
        const int nx = min(kConvTW, Wo - x0);
        const bool ok[2] = {x < Wo && y0 + j0 < Ho, x < Wo && y0 + j0 + 1 < Ho};
        const int nyw = max(0, min(2, Ho - (y0 + j0)));
        const float nw = (float)(nx * nyw);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lrow = 16 * (w & 1) + 4 * (lane >> 4) + r, row = (int)blockIdx.y * kConvOB + lrow;
            const bool live = row < g.cout;
            const float bs = g.bias && live ? g.bias[row] : 0.f;
            float v[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                v[c] = (NP == 1 ? acc[0][c][r] : split_sum(acc[0][c][r], acs[0][c][r])) + bs;
                if (ok[c] && live)
                    g.out[((size_t)b * g.oc + g.off + row) * HWo + (size_t)(y0 + j0 + c) * Wo + x] = v[c];
            }
            float s = (ok[0] ? v[0] : 0.f) + (ok[1] ? v[1] : 0.f);
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) s = s + __shfl_xor(s, m);
            const float mean = nyw > 0 ? s / nw : 0.f;
            const float d0 = ok[0] ? v[0] - mean : 0.f, d1 = ok[1] ? v[1] - mean : 0.f;
            float q = d0 * d0 + d1 * d1;
#pragma unroll
            for (int m = 1; m < 16; m <<= 1) q = q + __shfl_xor(q, m);
            if (fr == 0) {
                red[((w >> 1) * kConvOB + lrow) * 2] = s;
                red[((w >> 1) * kConvOB + lrow) * 2 + 1] = q;
            }
        }
        __syncthreads();
        const int row = (int)blockIdx.y * kConvOB + tid;
        if (tid < kConvOB && row < g.cout) {
            const float na = (float)(nx * min(2, Ho - y0)), nb = (float)(nx * max(0, min(2, Ho - y0 - 2)));
            const float sa = red[tid * 2], qa = red[tid * 2 + 1];
            const float sb = red[(kConvOB + tid) * 2], qb = red[(kConvOB + tid) * 2 + 1];
            float sum = sa, m2 = qa;
            if (nb > 0.f) {
                const float d = sb / nb - sa / na;
                sum = sa + sb;
                m2 = (qa + qb) + (d * d) * (na * nb / (na + nb));
            }
            float *st = g.stats + (((size_t)b * g.cout + row) * tiles + tl) * 2;
            st[0] = sum;
            st[1] = m2;
        }
    }
}

// One wave per (b, c): lane l merges tiles l per, .. in ascending order, then the lanes are merged
// pairwise in ascending order (Chan et al., fp64).  The pixel count of a tile is its geometry's.
struct Moments {
    double n, mean, m2;
};
__device__ __forceinline__ Moments merge(Moments a, Moments b) {
    if (b.n == 0.0) return a;
    if (a.n == 0.0) return b;
    const double n = a.n + b.n, d = b.mean - a.mean;
    return Moments{n, a.mean + d * (b.n / n), a.m2 + b.m2 + d * d * (a.n * b.n / n)};
}

__global__ __launch_bounds__(256) void enc_finalize_kernel(const float *__restrict__ stats, int BC, int Ho, int Wo,
                                                           int tx, int ty, float eps, float *__restrict__ scale,
                                                           float *__restrict__ shift) {
    const int lane = threadIdx.x & 63, bc = (int)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (bc >= BC) return;  // wave-uniform
    const int tiles = tx * ty, per = (tiles + 63) / 64;
    const float *st = stats + (size_t)bc * tiles * 2;
    Moments m{0.0, 0.0, 0.0};
    for (int t = lane * per; t < min(tiles, (lane + 1) * per); ++t) {
        const int tyi = t / tx, txi = t - tyi * tx;
        const double n = (double)(min(kConvTH, Ho - tyi * kConvTH) * min(kConvTW, Wo - txi * kConvTW));
        m = merge(m, Moments{n, (double)st[2 * t] / n, (double)st[2 * t + 1]});
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const Moments u{__shfl_down(m.n, o), __shfl_down(m.mean, o), __shfl_down(m.m2, o)};
        if ((lane & (2 * o - 1)) == 0) m = merge(m, u);
    }
    if (lane == 0) {
        const float sc = (float)(1.0 / sqrt(m.m2 / m.n + (double)eps));
        scale[bc] = sc;
        shift[bc] = (float)(-m.mean * (double)sc);
    }
}

// out = relu(skip + relu(y * scale + shift)); one plane (b, c) per blockIdx.x.  Each element is
// read and written by the same thread, so out may be y.
__global__ __launch_bounds__(256) void enc_join_kernel(const float *y, const float *__restrict__ scale,
                                                       const float *__restrict__ shift, int nb, const float *skip,
                                                       int C, size_t HW, float *out) {
    const int bc = blockIdx.x, k = nb ? bc : bc % C;
    const float sc = scale[k], sh = shift[k];
    const size_t base = (size_t)bc * HW;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.y * 256) {
        float v = y[base + i] * sc + sh;
        v = v < 0.f ? 0.f : v;
        v = skip[base + i] + v;
        out[base + i] = v < 0.f ? 0.f : v;
    }
}

constexpr int conv_rows(int cout) { return (cout + kConvPad - 1) / kConvPad * kConvPad; }

template <int STRIDE, bool NORM_IN, bool STATS, int NP = 3>
hipError_t launch_conv(const ConvArgs &g, hipStream_t s) {
    const dim3 grid((unsigned)g.B * g.tx * g.ty, conv_rows(g.cout) / kConvOB);
    hipLaunchKernelGGL((conv_kernel<STRIDE, NORM_IN, STATS, NP>), grid, dim3(kConvNT), 0, s, g);
    return hipGetLastError();
}

}  // namespace

bool conv_supported(int cout, int ca, int cb) {
    return cout >= 1 && cout <= 1024 && ca >= 32 && cb >= 0 && ca % 32 == 0 && cb % 32 == 0 && (long)ca + cb <= 1024;
}

size_t conv_weights_bytes(int cout, int cin) {
    return (size_t)(conv_rows(cout) / 16) * (cin / 32) * kConvTaps * 3 * 64 * sizeof(u32x4);
}

hipError_t launch_conv_pack(const float *w, int cout, int cin, void *packed, hipStream_t s) {
    if (!conv_supported(cout, cin, 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(conv_pack_kernel, dim3(cin / 32, conv_rows(cout) / 16), dim3(64), 0, s, w, cout, cin,
                       static_cast<u32x4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_conv_forward(const float *in_a, int ca, const float *in_b, int cb, int B, int H, int W,
                               const void *packed, const float *bias, int cout, int relu, float *out,
                               int out_channels, int out_offset, hipStream_t s, int precision) {
    if (!conv_supported(cout, ca, cb) || !precision_supported(precision)) return hipErrorInvalidValue;
    ConvArgs g{};
    g.a = in_a, g.b = cb > 0 ? in_b : in_a, g.bias = bias;
    g.frag = static_cast<const u32x4 *>(packed);
    g.out = out;
    g.B = B, g.ca = ca, g.cb = cb, g.H = H, g.W = W, g.cout = cout, g.relu = relu;
    g.oc = out_channels, g.off = out_offset;
    g.tx = (W + kConvTW - 1) / kConvTW, g.ty = (H + kConvTH - 1) / kConvTH;
    switch (precision) {
        case 1: return launch_conv<1, false, false, 2>(g, s);
        case 2: return launch_conv<1, false, false, 1>(g, s);
        default: return launch_conv<1, false, false>(g, s);
    }
}

static int enc_out(int n, int stride) { return (n - 1) / stride + 1; }

size_t enc_stats_bytes(int B, int cout, int Ho, int Wo) {
    return (size_t)B * cout * ((Ho + kConvTH - 1) / kConvTH) * ((Wo + kConvTW - 1) / kConvTW) * 2 * sizeof(float);
}

// The eight encoder forms at NP pieces: sel = 4 (stride 2) | 2 (norm on load) | 1 (statistics).
template <int NP>
static hipError_t launch_enc_form(int sel, const ConvArgs &g, hipStream_t s) {
    switch (sel) {
        case 0: return launch_conv<1, false, false, NP>(g, s);
        case 1: return launch_conv<1, false, true, NP>(g, s);
        case 2: return launch_conv<1, true, false, NP>(g, s);
        case 3: return launch_conv<1, true, true, NP>(g, s);
        case 4: return launch_conv<2, false, false, NP>(g, s);
        case 5: return launch_conv<2, false, true, NP>(g, s);
        case 6: return launch_conv<2, true, false, NP>(g, s);
        default: return launch_conv<2, true, true, NP>(g, s);
    }
}

hipError_t launch_enc_conv(const float *in, int cin, int B, int H, int W, int stride, const float *scale,
                           const float *shift, int norm_per_batch, const void *packed, const float *bias, int cout,
                           float *out, float *stats, hipStream_t s, int precision) {
    if (!conv_supported(cout, cin, 0) || (stride != 1 && stride != 2) || !precision_supported(precision))
        return hipErrorInvalidValue;
    const int Ho = enc_out(H, stride), Wo = enc_out(W, stride);
    ConvArgs g{};
    g.a = g.b = in, g.bias = bias;
    g.frag = static_cast<const u32x4 *>(packed);
    g.out = out, g.scale = scale, g.shift = shift, g.stats = stats;
    g.B = B, g.ca = cin, g.cb = 0, g.H = H, g.W = W, g.cout = cout, g.relu = 0, g.oc = cout, g.off = 0;
    g.tx = (Wo + kConvTW - 1) / kConvTW, g.ty = (Ho + kConvTH - 1) / kConvTH, g.nb = norm_per_batch;
    const int sel = (stride == 2 ? 4 : 0) | (scale ? 2 : 0) | (stats ? 1 : 0);
    switch (precision) {
        case 1: return launch_enc_form<2>(sel, g, s);
        case 2: return launch_enc_form<1>(sel, g, s);
        default: return launch_enc_form<3>(sel, g, s);
    }
}

hipError_t launch_enc_finalize(const float *stats, int B, int C, int Ho, int Wo, float eps, float *scale,
                               float *shift, hipStream_t s) {
    const int BC = B * C;
    hipLaunchKernelGGL(enc_finalize_kernel, dim3((BC + 3) / 4), dim3(256), 0, s, stats, BC, Ho, Wo,
                       (Wo + kConvTW - 1) / kConvTW, (Ho + kConvTH - 1) / kConvTH, eps, scale, shift);
    return hipGetLastError();
}

hipError_t launch_enc_join(const float *y, const float *scale, const float *shift, int norm_per_batch,
                           const float *skip, int B, int C, int H, int W, float *out, hipStream_t s) {
    const size_t HW = (size_t)H * W;
    const unsigned gy = (unsigned)((HW + 1023) / 1024 < 4096 ? (HW + 1023) / 1024 : 4096);
    hipLaunchKernelGGL(enc_join_kernel, dim3((unsigned)(B * C), gy), dim3(256), 0, s, y, scale, shift, norm_per_batch,
                       skip, C, HW, out);
    return hipGetLastError();
}

}  // namespace corr

