// corr_enc_front.hip — what BasicEncoder runs around its residual stages (model/extractor.py:
// 137-189), on gfx950, inference only: the 7x7 stride-2 stem, the 1x1 convolutions (the strided
// blocks' projections at stride 2, the head at stride 1), and the join that normalises its skip.
//
//   stem:  out[b][o][y][x] = bias[o] + sum_c sum_ky sum_kx w[o][c][ky][kx] in[b][c][2y+ky-3][2x+kx-3]
//   pw:    out[b][o][y][x] = bias[o] + sum_c w[o][c] in[b][c][s y][s x],  s = 1 or 2
//   join:  out = relu(s(skip) + relu(y * scale + shift)),  s(v) = v * skip_scale + skip_shift [, relu]
//
// The arithmetic is corr_conv.hip's: an implicit GEMM on the 16x16x32 bf16 MFMA with the build's
// exact three-piece split (x = hi + mid + lo, six products per fp32 product in the family's
// order (corr_bf16x6.h), two accumulators joined by split_sum), and so are the workgroup's shape
// (4 waves, one tile of 4 rows x 16 columns of one batch item's output; wave w owns the row blocks
// of half w & 1 and the tile rows 2 (w >> 1), + 1) and the optional per-tile (sum, M2) statistics,
// which corr_enc_norm_finalize merges unchanged.
//
// Stem.  K is tap-major: tap = 7 ky + kx ascending, the cin <= 16 channels of a tap padded to 16,
// so one 32-wide K step is two taps and the 49 taps are 25 steps (the 50th tap's weights are
// zero).  The workgroup stages the tile's 13 x 37 input window once (8 channel pairs a position,
// zero outside the map and for the channels >= cin, which are never read: their loads are clamped
// to the last channel the tensor has) through split3 into LDS, then every K step reads its B
// fragment at the two taps' position offsets.  A wave owns two 16-row blocks (64 output rows a
// workgroup: the model's 64 channels stage each window once).  The weights are pre-split into
// A-fragment order [16-row block][step][piece][lane] and run two steps ahead in registers.
//
// Pointwise.  K = cin in ascending 32-channel chunks.  Per chunk the workgroup stages its 64 output
// pixels' input positions (s y, s x): at stride 2 only even rows and columns are ever read.  There
// is no padding, so nothing is zeroed: a pixel past the map's edge re-reads the last one and is
// neither stored nor counted.  The pack is conv_pack_kernel's with one tap.
//
// Every load is unconditional, from an address clamped into the same map; a zero is applied to
// the loaded value afterwards.  No atomics, no scratch, nothing allocated.
#include "corr_bf16x6.h"
#include "corr_common.h"

namespace corr {
namespace {

constexpr int kTW = kConvTW, kTH = kConvTH, kNT = kConvNT, kPad = kConvPad;  // the family's tile (corr_bf16x6.h)
constexpr int kStemT = 2;          // 16-row blocks per wave: 64 output rows per workgroup
constexpr int kStemK = 7, kStemTaps = 49, kStemSteps = 25, kStemMaxCin = 16;
constexpr int kStemPW = kTW * 2 + kStemK - 2;   // staged positions per row: 37
constexpr int kStemPH = kTH * 2 + kStemK - 2;   // staged rows: 13
constexpr int kStemNPOS = kStemPW * kStemPH;    // 481
constexpr int kStemXS = 8;                      // words per LDS position: 8 channel pairs
constexpr int kStemWords = kStemNPOS * kStemXS; // staged words per piece
constexpr int kStemNLD = (kStemWords + kNT - 1) / kNT;  // staging passes per thread: 16, the last guarded
constexpr int kPwT = 1;            // 32 output rows per workgroup
constexpr int kPwXS = 16 + 4;      // words per LDS position: 16 channel pairs + pad (16-B rows)
// Waves per SIMD the pointwise and the stem kernel are compiled for, by the pieces they keep
// (DESIGN §30 has the resource report behind each value).  1 asks for nothing, as before: the
// pointwise kernel reaches 6 / 7 / 8 waves on its own (64 / 56 / 40 registers), and the stem's
// three-piece form stays the parent's (152 + 48 registers, 46 KB of LDS: 2 waves).  The stem's
// reduced forms fit one more wave each without a spill: 134 registers and 31 KB (3), 114 and 15 KB (4).
constexpr int front_waves(int np) { return 1; }
constexpr int stem_waves(int np) { return np == 1 ? 4 : np == 2 ? 3 : 1; }

struct FrontArgs {
    const float *in;
    const float *bias;   // [cout], or null for no bias
    const u32x4 *frag;   // the pack
    float *out;          // [B][cout][Ho][Wo]
    float *stats;        // STATS: [B][cout][tiles][2]
    int B, cin, H, W, Ho, Wo, cout, tx, ty;
};

// C[row = 4 (lane >> 4) + r][col = lane & 15] of row block t, tile row j0 + c: + bias, store, and
// (STATS) the tile's (sum, M2 about its own mean) per output row: a butterfly over the 16 lanes of
// a row group per wave (every lane ends with the same bits: each level adds the same two values in
// either order), the squared deviations from that half's mean likewise; the two halves of the tile
// (waves w and w + 2) meet in LDS and thread `row` merges them, upper half first (Chan et al.).
// Every lane stays to the end (the reductions and the barrier need all of them); a pixel past Ho /
// Wo is neither stored nor counted.
// This is the statistics epilogue's one description; conv_kernel's STATS branch (corr_conv.hip) is
// a copy of it for T = 1 that writes a channel window.  The two stay separate because either one
// compiled from a shared function came out as different machine code; a change to
// one is a change to both, and enc_finalize_kernel reads what both write.
// NP: the pieces the kernel kept; a one-piece kernel (bf16) has no acs and its result is acc alone.
template <int T, bool STATS, int NP = 3>
__device__ __forceinline__ void front_epilogue(const FrontArgs &g, const f32x4 (&acc)[T][2], const f32x4 (&acs)[T][2],
                                               int b, int tl, int y0, int x0, float *red) {
    constexpr int R = 32 * T;  // output rows per workgroup
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int fr = lane & 15, j0 = 2 * (w >> 1), x = x0 + fr;
    const int Ho = g.Ho, Wo = g.Wo;
    const size_t HWo = (size_t)Ho * Wo;
    const bool ok[2] = {x < Wo && y0 + j0 < Ho, x < Wo && y0 + j0 + 1 < Ho};
    const int nx = min(kTW, Wo - x0);
    const int nyw = max(0, min(2, Ho - (y0 + j0)));
    const float nw = (float)(nx * nyw);
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int lrow = 16 * (T * (w & 1) + t) + 4 * (lane >> 4) + r, row = (int)blockIdx.y * R + lrow;
            const bool live = row < g.cout;  // else a padding row of the pack
            const float bs = g.bias && live ? g.bias[row] : 0.f;
            float v[2];
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                v[c] = (NP == 1 ? acc[t][c][r] : split_sum(acc[t][c][r], acs[t][c][r])) + bs;
                if (ok[c] && live) g.out[((size_t)b * g.cout + row) * HWo + (size_t)(y0 + j0 + c) * Wo + x] = v[c];
            }
            if constexpr (STATS) {
                float s = (ok[0] ? v[0] : 0.f) + (ok[1] ? v[1] : 0.f);
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) s = s + __shfl_xor(s, m);
                const float mean = nyw > 0 ? s / nw : 0.f;
                const float d0 = ok[0] ? v[0] - mean : 0.f, d1 = ok[1] ? v[1] - mean : 0.f;
                float q = d0 * d0 + d1 * d1;
#pragma unroll
                for (int m = 1; m < 16; m <<= 1) q = q + __shfl_xor(q, m);
                if (fr == 0) {
                    red[((w >> 1) * R + lrow) * 2] = s;
                    red[((w >> 1) * R + lrow) * 2 + 1] = q;
                }
            }
        }
    if constexpr (STATS) {
        __syncthreads();
        const int row = (int)blockIdx.y * R + tid;
        if (tid < R && row < g.cout) {
            const float na = (float)(nx * min(2, Ho - y0)), nb = (float)(nx * max(0, min(2, Ho - y0 - 2)));
            const float sa = red[tid * 2], qa = red[tid * 2 + 1];
            const float sb = red[(R + tid) * 2], qb = red[(R + tid) * 2 + 1];
            float sum = sa, m2 = qa;
            if (nb > 0.f) {
                const float d = sb / nb - sa / na;
                sum = sa + sb;
                m2 = (qa + qb) + (d * d) * (na * nb / (na + nb));
            }
            float *st = g.stats + (((size_t)b * g.cout + row) * (g.tx * g.ty) + tl) * 2;
            st[0] = sum;
            st[1] = m2;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// stem
// ---------------------------------------------------------------------------------------------
// w [cout][cin][7][7] fp32 -> pieces [rows/16 blocks][25 steps][hi, mid, lo][64 lanes] in the
// 16x16x32 A-fragment order: lane = 16 kg + r holds W[16 ob + r][8 (kg & 1) + j][tap 2 s + (kg >> 1)],
// j < 8; rows >= cout, channels >= cin and tap 49 are zero.  One block per (step, ob).
__global__ __launch_bounds__(64) void stem_pack_kernel(const float *__restrict__ w, int cout, int cin,
                                                       u32x4 *__restrict__ frag) {
    const int s = blockIdx.x, ob = blockIdx.y, lane = threadIdx.x;
    const int row = 16 * ob + (lane & 15), kg = lane >> 4, tap = 2 * s + (kg >> 1), c0 = 8 * (kg & 1);
    const bool live = row < cout && tap < kStemTaps;
    const float *src = w + (size_t)(live ? row : 0) * cin * kStemTaps + (live ? tap : 0);
    unsigned h[4], m[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int ca = c0 + 2 * j, cb = ca + 1;
        const float a = src[(size_t)min(ca, cin - 1) * kStemTaps], b = src[(size_t)min(cb, cin - 1) * kStemTaps];
        split3(live && ca < cin ? a : 0.f, live && cb < cin ? b : 0.f, h[j], m[j], lo[j]);
    }
    u32x4 *dst = frag + (((size_t)ob * kStemSteps + s) * 3) * 64 + lane;
    store_pieces(dst, h, m, lo);
}

constexpr int stem_tap_offset(int tap) {  // the window offset of a tap (the zero 50th tap reads the 49th's)
    const int t = tap < kStemTaps ? tap : kStemTaps - 1;
    return (t / kStemK) * kStemPW + t % kStemK;
}

// NP: the pieces kept per operand (3 = bf16x6, 2 = bf16x3, 1 = bf16: products<NP>, corr_bf16x6.h);
// a reduced mode stages and fetches only those, from the same pack.
template <bool STATS, int NP = 3>
__global__ __launch_bounds__(kNT, stem_waves(NP)) void stem_kernel(FrontArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned xs[NP][kStemNPOS][kStemXS];
    __shared__ float red[STATS ? 2 * 32 * kStemT * 2 : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = g.H, W = g.W, cin = g.cin;
    const size_t HW = (size_t)H * W;
    const int tiles = g.tx * g.ty;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int y0 = (tl / g.tx) * kTH, x0 = (tl % g.tx) * kTW;

    // ---- A fragments of row blocks ob0, ob0 + 1, two steps ahead ----
    const int ob0 = (int)blockIdx.y * (2 * kStemT) + kStemT * (w & 1);
    auto load_a = [&](u32x4 (&wa)[kStemT][NP], int s) {
#pragma unroll
        for (int t = 0; t < kStemT; ++t) {
            const size_t base = ((size_t)(ob0 + t) * kStemSteps + s) * 3 * 64 + lane;
#pragma unroll
            for (int p = 0; p < NP; ++p) wa[t][p] = g.frag[base + 64 * p];
        }
    };
    u32x4 wa[3][kStemT][NP];
    load_a(wa[0], 0);
    load_a(wa[1], 1);

    // ---- staging: pass i of this thread is word idx = tid + 256 i = channel pair idx / 481 at
    // window position idx % 481 ----
    {
        const float *src = g.in + (size_t)b * cin * HW;
        float v[kStemNLD][2];
        unsigned in_a = 0, in_b = 0;  // bit i: pass i's first / second value is a real one (else zero)
#pragma unroll
        for (int i = 0; i < kStemNLD; ++i) {
            const int idx = tid + kNT * i;
            const bool live = idx < kStemWords;  // false only in the last pass
            const int kp = live ? idx / kStemNPOS : 0, ps = live ? idx - kp * kStemNPOS : 0;
            const int y = 2 * y0 + ps / kStemPW - 3, x = 2 * x0 + ps % kStemPW - 3;
            const bool in = live && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
            const size_t off = in ? (size_t)y * W + x : 0;
            v[i][0] = src[(size_t)min(2 * kp, cin - 1) * HW + off];
            v[i][1] = src[(size_t)min(2 * kp + 1, cin - 1) * HW + off];
            in_a |= (unsigned)(in && 2 * kp < cin) << i;
            in_b |= (unsigned)(in && 2 * kp + 1 < cin) << i;
        }
#pragma unroll
        for (int i = 0; i < kStemNLD; ++i) {
            const int idx = tid + kNT * i;
            const int kp = idx / kStemNPOS, ps = idx - kp * kStemNPOS;
            unsigned hi, mid, lo;
            split3((in_a >> i) & 1 ? v[i][0] : 0.f, (in_b >> i) & 1 ? v[i][1] : 0.f, hi, mid, lo);
            if (i + 1 < kStemNLD || idx < kStemWords) {
                xs[0][ps][kp] = hi;
                if constexpr (NP > 1) xs[1][ps][kp] = mid;
                if constexpr (NP > 2) xs[2][ps][kp] = lo;
            }
        }
    }
    __syncthreads();

    // ---- K loop: lane = 16 kg + fr reads tap 2 s + (kg >> 1), channel pairs 4 (kg & 1) .. + 3 of
    // output column fr ----
    const int fr = lane & 15, kg = lane >> 4, j0 = 2 * (w >> 1);
    const bool odd = kg >> 1;
    const unsigned *xb0 = &xs[0][(2 * j0) * kStemPW + 2 * fr][4 * (kg & 1)];
    f32x4 acc[kStemT][2], acs[kStemT][2];
#pragma unroll
    for (int t = 0; t < kStemT; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[t][c] = acs[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kStemSteps; ++s) {
        if (s + 2 < kStemSteps) load_a(wa[(s + 2) % 3], s + 2);
        const int tp = odd ? stem_tap_offset(2 * s + 1) : stem_tap_offset(2 * s);
        u32x4 xb[2][NP];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int p = 0; p < NP; ++p)
                xb[c][p] = *reinterpret_cast<const u32x4 *>(xb0 + (p * kStemNPOS + 2 * c * kStemPW + tp) * kStemXS);
#pragma unroll
        for (int t = 0; t < kStemT; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) products<NP>(wa[s % 3][t], xb[c], acc[t][c], acs[t][c]);
    }
    front_epilogue<kStemT, STATS, NP>(g, acc, acs, b, tl, y0, x0, red);
}

// ---------------------------------------------------------------------------------------------
// pointwise
// ---------------------------------------------------------------------------------------------
// w [cout][cin] fp32 -> pieces [rows/16 blocks][cin/32 chunks][hi, mid, lo][64 lanes]: lane =
// 16 kg + r holds W[16 ob + r][32 chunk + 8 kg + j], j < 8; rows >= cout are zero.
__global__ __launch_bounds__(64) void pw_pack_kernel(const float *__restrict__ w, int cout, int cin,
                                                     u32x4 *__restrict__ frag) {
    const int ch = blockIdx.x, ob = blockIdx.y, lane = threadIdx.x;
    const int row = 16 * ob + (lane & 15), c0 = 32 * ch + 8 * (lane >> 4);
    const bool live = row < cout;
    const float *src = w + (size_t)(live ? row : 0) * cin + c0;
    unsigned h[4], m[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split3(live ? src[2 * j] : 0.f, live ? src[2 * j + 1] : 0.f, h[j], m[j], lo[j]);
    u32x4 *dst = frag + (((size_t)ob * (cin / 32) + ch) * 3) * 64 + lane;
    store_pieces(dst, h, m, lo);
}

template <int S, bool STATS, int NP = 3>
__global__ __launch_bounds__(kNT, front_waves(NP)) void pw_kernel(FrontArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned xs[NP][kTH * kTW][kPwXS];
    __shared__ float red[STATS ? 2 * 32 * kPwT * 2 : 1];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const size_t HW = (size_t)g.H * g.W;
    const int tiles = g.tx * g.ty;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int y0 = (tl / g.tx) * kTH, x0 = (tl % g.tx) * kTW;
    const int NC = g.cin / 32;
    const int wu = __builtin_amdgcn_readfirstlane(w);

    // staging: lane = the tile's pixel 16 j + fr, pass i = channel pair wu + 4 i.  A pixel past the
    // output's edge reads the last one inside (an even position at stride 2).
    const int py = min(y0 + (lane >> 4), g.Ho - 1), px = min(x0 + (lane & 15), g.Wo - 1);
    const float *src = g.in + (size_t)b * g.cin * HW + (size_t)(S * py) * g.W + S * px;
    auto load_chunk = [&](int ch, float (&v)[4][2]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float *p = src + (size_t)(32 * ch + 2 * (wu + 4 * i)) * HW;
            v[i][0] = p[0];
            v[i][1] = p[HW];
        }
    };
    const int ob0 = (int)blockIdx.y * (2 * kPwT) + kPwT * (w & 1);
    auto load_a = [&](u32x4 (&wa)[kPwT][NP], int ch) {
#pragma unroll
        for (int t = 0; t < kPwT; ++t) {
            const size_t base = ((size_t)(ob0 + t) * NC + ch) * 3 * 64 + lane;
#pragma unroll
            for (int p = 0; p < NP; ++p) wa[t][p] = g.frag[base + 64 * p];
        }
    };

    const int fr = lane & 15, fk = 4 * (lane >> 4), j0 = 2 * (w >> 1);
    f32x4 acc[kPwT][2], acs[kPwT][2];
#pragma unroll
    for (int t = 0; t < kPwT; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[t][c] = acs[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    float va[4][2];
    u32x4 wn[kPwT][NP];
    load_chunk(0, va);
    load_a(wn, 0);
#pragma unroll 1
    for (int ch = 0; ch < NC; ++ch) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            unsigned hi, mid, lo;
            split3(va[i][0], va[i][1], hi, mid, lo);
            xs[0][lane][wu + 4 * i] = hi;
            if constexpr (NP > 1) xs[1][lane][wu + 4 * i] = mid;
            if constexpr (NP > 2) xs[2][lane][wu + 4 * i] = lo;
        }
        u32x4 wa[kPwT][NP];
#pragma unroll
        for (int t = 0; t < kPwT; ++t)
#pragma unroll
            for (int p = 0; p < NP; ++p) wa[t][p] = wn[t][p];
        __syncthreads();
        const int nx = ch + 1 < NC ? ch + 1 : NC - 1;  // (past the end: a harmless re-read)
        load_chunk(nx, va);
        load_a(wn, nx);
        u32x4 xb[2][NP];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int p = 0; p < NP; ++p) xb[c][p] = *reinterpret_cast<const u32x4 *>(&xs[p][(j0 + c) * kTW + fr][fk]);
#pragma unroll
        for (int t = 0; t < kPwT; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) products<NP>(wa[t], xb[c], acc[t][c], acs[t][c]);
        __syncthreads();
    }
    front_epilogue<kPwT, STATS, NP>(g, acc, acs, b, tl, y0, x0, red);
}

// ---------------------------------------------------------------------------------------------
// join
// ---------------------------------------------------------------------------------------------
// out = relu(s(skip) + relu(y * scale + shift)), s(v) = v * kscale + kshift [then relu]; one plane
// (b, c) per blockIdx.x.  Each element is read and written by the same thread, so out may be y.
template <bool SKIP_AFFINE>
__global__ __launch_bounds__(256) void join_affine_kernel(const float *y, const float *__restrict__ scale,
                                                          const float *__restrict__ shift, int nb, const float *skip,
                                                          const float *__restrict__ kscale,
                                                          const float *__restrict__ kshift, int knb, int krelu, int C,
                                                          size_t HW, float *out) {
    const int bc = blockIdx.x, k = nb ? bc : bc % C;
    const float sc = scale[k], sh = shift[k];
    float ksc = 1.f, ksh = 0.f;
    if constexpr (SKIP_AFFINE) {
        const int kk = knb ? bc : bc % C;
        ksc = kscale[kk], ksh = kshift[kk];
    }
    const size_t base = (size_t)bc * HW;
    for (size_t i = (size_t)blockIdx.y * 256 + threadIdx.x; i < HW; i += (size_t)gridDim.y * 256) {
        float v = y[base + i] * sc + sh;
        v = v < 0.f ? 0.f : v;
        float u = skip[base + i];
        if constexpr (SKIP_AFFINE) u = u * ksc + ksh;
        if (krelu) u = u < 0.f ? 0.f : u;
        v = u + v;
        out[base + i] = v < 0.f ? 0.f : v;
    }
}

constexpr int front_rows(int cout) { return (cout + kPad - 1) / kPad * kPad; }

FrontArgs front_args(const float *in, int cin, int B, int H, int W, int stride, const void *packed, const float *bias,
                     int cout, float *out, float *stats) {
    FrontArgs g{};
    g.in = in, g.bias = bias, g.frag = static_cast<const u32x4 *>(packed), g.out = out, g.stats = stats;
    g.B = B, g.cin = cin, g.H = H, g.W = W, g.cout = cout;
    g.Ho = (H - 1) / stride + 1, g.Wo = (W - 1) / stride + 1;
    g.tx = (g.Wo + kTW - 1) / kTW, g.ty = (g.Ho + kTH - 1) / kTH;
    return g;
}

}  // namespace

bool enc_stem_supported(int cout, int cin) { return cout >= 1 && cout <= 1024 && cin >= 1 && cin <= kStemMaxCin; }

size_t enc_stem_weights_bytes(int cout) {
    return (size_t)(front_rows(cout) / 16) * kStemSteps * 3 * 64 * sizeof(u32x4);
}

hipError_t launch_enc_stem_pack(const float *w, int cout, int cin, void *packed, hipStream_t s) {
    if (!enc_stem_supported(cout, cin)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(stem_pack_kernel, dim3(kStemSteps, front_rows(cout) / 16), dim3(64), 0, s, w, cout, cin,
                       static_cast<u32x4 *>(packed));
    return hipGetLastError();
}

namespace {
template <int NP>
void launch_stem_np(const FrontArgs &g, dim3 grid, hipStream_t s) {
    if (g.stats)
        hipLaunchKernelGGL((stem_kernel<true, NP>), grid, dim3(kNT), 0, s, g);
    else
        hipLaunchKernelGGL((stem_kernel<false, NP>), grid, dim3(kNT), 0, s, g);
}

template <int NP>
void launch_pw_np(const FrontArgs &g, int stride, dim3 grid, hipStream_t s) {
    switch ((stride == 2 ? 2 : 0) | (g.stats ? 1 : 0)) {
        case 0: hipLaunchKernelGGL((pw_kernel<1, false, NP>), grid, dim3(kNT), 0, s, g); break;
        case 1: hipLaunchKernelGGL((pw_kernel<1, true, NP>), grid, dim3(kNT), 0, s, g); break;
        case 2: hipLaunchKernelGGL((pw_kernel<2, false, NP>), grid, dim3(kNT), 0, s, g); break;
        default: hipLaunchKernelGGL((pw_kernel<2, true, NP>), grid, dim3(kNT), 0, s, g); break;
    }
}
}  // namespace

hipError_t launch_enc_stem(const float *in, int cin, int B, int H, int W, const void *packed, const float *bias,
                           int cout, float *out, float *stats, hipStream_t s, int precision) {
    if (!enc_stem_supported(cout, cin) || !precision_supported(precision)) return hipErrorInvalidValue;
    const FrontArgs g = front_args(in, cin, B, H, W, 2, packed, bias, cout, out, stats);
    const dim3 grid((unsigned)B * g.tx * g.ty, (cout + 32 * kStemT - 1) / (32 * kStemT));
    switch (precision) {
        case 1: launch_stem_np<2>(g, grid, s); break;
        case 2: launch_stem_np<1>(g, grid, s); break;
        default: launch_stem_np<3>(g, grid, s); break;
    }
    return hipGetLastError();
}

bool enc_pw_supported(int cout, int cin) {
    return cout >= 1 && cout <= 1024 && cin >= 32 && cin <= 1024 && cin % 32 == 0;
}

size_t enc_pw_weights_bytes(int cout, int cin) {
    return (size_t)(front_rows(cout) / 16) * (cin / 32) * 3 * 64 * sizeof(u32x4);
}

hipError_t launch_enc_pw_pack(const float *w, int cout, int cin, void *packed, hipStream_t s) {
    if (!enc_pw_supported(cout, cin)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(pw_pack_kernel, dim3(cin / 32, front_rows(cout) / 16), dim3(64), 0, s, w, cout, cin,
                       static_cast<u32x4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_enc_pw(const float *in, int cin, int B, int H, int W, int stride, const void *packed,
                         const float *bias, int cout, float *out, float *stats, hipStream_t s, int precision) {
    if (!enc_pw_supported(cout, cin) || (stride != 1 && stride != 2) || !precision_supported(precision))
        return hipErrorInvalidValue;
    const FrontArgs g = front_args(in, cin, B, H, W, stride, packed, bias, cout, out, stats);
    const dim3 grid((unsigned)B * g.tx * g.ty, (cout + 32 * kPwT - 1) / (32 * kPwT));
    switch (precision) {
        case 1: launch_pw_np<2>(g, stride, grid, s); break;
        case 2: launch_pw_np<1>(g, stride, grid, s); break;
        default: launch_pw_np<3>(g, stride, grid, s); break;
    }
    return hipGetLastError();
}

hipError_t launch_enc_join_affine(const float *y, const float *scale, const float *shift, int norm_per_batch,
                                  const float *skip, const float *skip_scale, const float *skip_shift,
                                  int skip_per_batch, int skip_relu, int B, int C, int H, int W, float *out,
                                  hipStream_t s) {
    const size_t HW = (size_t)H * W;
    const unsigned gy = (unsigned)((HW + 1023) / 1024 < 4096 ? (HW + 1023) / 1024 : 4096);
    const dim3 grid((unsigned)(B * C), gy);
    if (skip_scale)
        hipLaunchKernelGGL(join_affine_kernel<true>, grid, dim3(256), 0, s, y, scale, shift, norm_per_batch, skip,
                           skip_scale, skip_shift, skip_per_batch, skip_relu, C, HW, out);
    else
        hipLaunchKernelGGL(join_affine_kernel<false>, grid, dim3(256), 0, s, y, scale, shift, norm_per_batch, skip,
                           skip_scale, skip_shift, skip_per_batch, skip_relu, C, HW, out);
    return hipGetLastError();
}

}  // namespace corr
