// corr_conv.hip — a 3x3 convolution (padding 1, stride 1) with bias and an optional ReLU on
// gfx950, inference only: the update block's convc2, convf2, conv and the two heads' first
// convolutions (model/update.py:63-107).
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
// fixed order), on v_mfma_f32_16x16x32_bf16 with the build's exact three-piece split (x = hi +
// mid + lo, six products per fp32 product in lookup_conv_kernel's order, two accumulators joined
// by split_sum: no narrower than fp32, no scales).
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
// Non-finite inputs are not parity-checked (an infinite activation meets the zero mid / lo
// pieces of the weights); finite inputs give finite outputs.
#include <type_traits>

#include "corr_build_common.h"
#include "corr_common.h"

namespace corr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kConvTW = 16, kConvTH = 4;       // pixel tile (columns x rows)
constexpr int kConvPW = kConvTW + 2;           // staged positions per row
constexpr int kConvPH = kConvTH + 2;           // staged rows
constexpr int kConvNPOS = kConvPW * kConvPH;   // 108
constexpr int kConvT = 1;                      // 16-row blocks per wave (2 measured slower)
constexpr int kConvOB = 32 * kConvT;           // output rows per workgroup
constexpr int kConvPad = 64;                   // the pack pads the rows to a multiple of this
constexpr int kConvNT = 256;                   // threads
constexpr int kConvXS = 16 + 4;                // words per LDS position: 16 channel pairs + pad (16-B rows)
constexpr int kConvTaps = 9;
constexpr int kConvWaves = 2;                  // waves per SIMD the kernel is compiled for (<= 256 registers)
constexpr int kConvRing = 6;                   // weight ring slots; divides the 18 K steps of a chunk pair
constexpr int kConvAhead = 5;                  // K steps the weight fragments run ahead (< kConvRing)
constexpr int kConvStage = kConvNPOS * 16;     // staged words per piece and chunk: 1728
constexpr int kConvNLD = (kConvStage + kConvNT - 1) / kConvNT;  // staging passes per thread: 7, the last guarded
static_assert((2 * kConvTaps) % kConvRing == 0 && kConvAhead < kConvRing, "ring slots are compile-time");
static_assert(kConvStage - (kConvNLD - 1) * kConvNT > 0 && (kConvStage - (kConvNLD - 1) * kConvNT) % 64 == 0,
              "the guard of the last staging pass is wave-uniform");

__device__ __forceinline__ f32x4 mfma_bf16(u32x4 a, u32x4 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c,
                                                  0, 0, 0);
}

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
        dst[0] = u32x4{h[0], h[1], h[2], h[3]};
        dst[64] = u32x4{m[0], m[1], m[2], m[3]};
        dst[128] = u32x4{lo[0], lo[1], lo[2], lo[3]};
    }
}

struct ConvArgs {
    const float *a;     // channels < ca of the input
    const float *b;     // the other cb channels (unused when cb == 0)
    const float *bias;  // [cout], or null for no bias
    const u32x4 *frag;  // the pack
    float *out;         // [B][oc][H][W]; channels off .. off + cout - 1 are written
    int B, ca, cb, H, W, cout, relu, oc, off, tx, ty;
};

__global__ __launch_bounds__(kConvNT, kConvWaves) void conv_kernel(ConvArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned xs[3][kConvNPOS][kConvXS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = g.H, W = g.W;
    const size_t HW = (size_t)H * W;
    const int tiles = g.tx * g.ty;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int y0 = (tl / g.tx) * kConvTH, x0 = (tl % g.tx) * kConvTW;
    const int NC = (g.ca + g.cb) / 32, NS = NC * kConvTaps;

    // ---- staging: pass i of this thread is channel pair kp[i] at position ps[i] ----
    int ps[kConvNLD], kp[kConvNLD];
    long off[kConvNLD];  // float offset inside a batch item's chunk (0 for a position outside the map)
    unsigned inmap = 0;  // bit i: pass i's position is inside the map (else its values are zero)
#pragma unroll
    for (int i = 0; i < kConvNLD; ++i) {
        const int idx = tid + kConvNT * i;
        const bool live = idx < kConvStage;  // false only in the last pass (wave 3)
        kp[i] = live ? idx / kConvNPOS : 0;
        ps[i] = live ? idx - kp[i] * kConvNPOS : 0;
        const int y = y0 + ps[i] / kConvPW - 1, x = x0 + ps[i] % kConvPW - 1;
        const bool in = live && (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        off[i] = in ? (long)(2 * kp[i]) * (long)HW + (long)y * W + x : 0;
        inmap |= (unsigned)in << i;
    }
    // (every load is unconditional, from a valid address, and the zero of a position outside the
    // map is applied at the split: a select on the loaded value would wait for it right here)
    auto load_chunk = [&](int ch, float (&v)[kConvNLD][2]) {
        const int c0 = 32 * ch;
        const float *src = c0 < g.ca ? g.a + ((size_t)b * g.ca + c0) * HW : g.b + ((size_t)b * g.cb + (c0 - g.ca)) * HW;
#pragma unroll
        for (int i = 0; i < kConvNLD; ++i) {
            v[i][0] = src[off[i]];
            v[i][1] = src[off[i] + HW];
        }
    };

    // ---- A fragments: row blocks ob0 .. ob0 + kConvT - 1 of the pack, K step s = 9 chunk + tap ----
    const int ob0 = (int)blockIdx.y * (kConvOB / 16) + kConvT * (w & 1);
    auto load_a = [&](u32x4 (&wa)[kConvT][3], int s) {
        s = s < NS ? s : NS - 1;  // the last steps re-read the last fragment
#pragma unroll
        for (int t = 0; t < kConvT; ++t) {
            const size_t base = ((size_t)(ob0 + t) * NS + s) * 3 * 64 + lane;
#pragma unroll
            for (int p = 0; p < 3; ++p) wa[t][p] = g.frag[base + 64 * p];
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
    // two workgroups, too few to hide an L2 round trip per step.
    u32x4 wa[kConvRing][kConvT][3];
    float va[kConvNLD][2], vb[kConvNLD][2];
    load_chunk(0, va);
    load_chunk(NC > 1 ? 1 : 0, vb);
#pragma unroll
    for (int s = 0; s < kConvAhead; ++s) load_a(wa[s], s);
    auto chunk = [&](int ch, auto par, float (&v)[kConvNLD][2]) {
        constexpr int S0 = decltype(par)::value * kConvTaps;  // this chunk's first step, mod the ring
#pragma unroll
        for (int i = 0; i < kConvNLD; ++i) {
            unsigned hi, mid, lo;
            const bool in = (inmap >> i) & 1;
            split3(in ? v[i][0] : 0.f, in ? v[i][1] : 0.f, hi, mid, lo);
            if (i + 1 < kConvNLD || tid + kConvNT * i < kConvStage) {
                xs[0][ps[i]][kp[i]] = hi;
                xs[1][ps[i]][kp[i]] = mid;
                xs[2][ps[i]][kp[i]] = lo;
            }
        }
        __syncthreads();
        load_chunk(ch + 2 < NC ? ch + 2 : NC - 1, v);  // (past the end: a harmless re-read)
#pragma unroll
        for (int tap = 0; tap < kConvTaps; ++tap) {
            load_a(wa[(S0 + tap + kConvAhead) % kConvRing], ch * kConvTaps + tap + kConvAhead);
            const int tp = (tap / 3) * kConvPW + tap % 3;
            u32x4 xb[2][3];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int p = 0; p < 3; ++p)
                    xb[c][p] = *reinterpret_cast<const u32x4 *>(&xs[p][(j0 + c) * kConvPW + fr + tp][fk]);
#pragma unroll
            for (int t = 0; t < kConvT; ++t) {
                const u32x4 wh = wa[(S0 + tap) % kConvRing][t][0], wm = wa[(S0 + tap) % kConvRing][t][1],
                            wl = wa[(S0 + tap) % kConvRing][t][2];
#pragma unroll
                for (int c = 0; c < 2; ++c) {
                    acs[t][c] = mfma_bf16(wl, xb[c][0], acs[t][c]);
                    acs[t][c] = mfma_bf16(wh, xb[c][2], acs[t][c]);
                    acs[t][c] = mfma_bf16(wm, xb[c][1], acs[t][c]);
                    acs[t][c] = mfma_bf16(wm, xb[c][0], acs[t][c]);
                    acs[t][c] = mfma_bf16(wh, xb[c][1], acs[t][c]);
                    acc[t][c] = mfma_bf16(wh, xb[c][0], acc[t][c]);
                }
            }
        }
        __syncthreads();
    };
    int ch = 0;
#pragma unroll 1
    for (; ch + 1 < NC; ch += 2) {
        chunk(ch, std::integral_constant<int, 0>{}, va);
        chunk(ch + 1, std::integral_constant<int, 1>{}, vb);
    }
    if (ch < NC) chunk(ch, std::integral_constant<int, 0>{}, va);

    // ---- epilogue: C[row = 4 (lane >> 4) + r][col = lane & 15] ----
    const int x = x0 + fr;
    if (x >= W) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int y = y0 + j0 + c;
        if (y >= H) continue;
        const size_t n = (size_t)y * W + x;
#pragma unroll
        for (int t = 0; t < kConvT; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (int)blockIdx.y * kConvOB + 16 * kConvT * (w & 1) + 16 * t + 4 * (lane >> 4) + r;
                if (row >= g.cout) continue;  // a padding row of the pack
                float v = split_sum(acc[t][c][r], acs[t][c][r]);
                if (g.bias) v = v + g.bias[row];
                if (g.relu) v = v < 0.f ? 0.f : v;
                g.out[((size_t)b * g.oc + g.off + row) * HW + n] = v;
            }
    }
}

constexpr int conv_rows(int cout) { return (cout + kConvPad - 1) / kConvPad * kConvPad; }

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
                               int out_channels, int out_offset, hipStream_t s) {
    if (!conv_supported(cout, ca, cb)) return hipErrorInvalidValue;
    ConvArgs g{};
    g.a = in_a, g.b = cb > 0 ? in_b : in_a, g.bias = bias;
    g.frag = static_cast<const u32x4 *>(packed);
    g.out = out;
    g.B = B, g.ca = ca, g.cb = cb, g.H = H, g.W = W, g.cout = cout, g.relu = relu;
    g.oc = out_channels, g.off = out_offset;
    g.tx = (W + kConvTW - 1) / kConvTW, g.ty = (H + kConvTH - 1) / kConvTH;
    const dim3 grid((unsigned)B * g.tx * g.ty, conv_rows(cout) / kConvOB);
    hipLaunchKernelGGL(conv_kernel, grid, dim3(kConvNT), 0, s, g);
    return hipGetLastError();
}

}  // namespace corr
