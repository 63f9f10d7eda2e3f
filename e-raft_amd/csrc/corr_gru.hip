// corr_gru.hip — one half step of the update block's SepConvGRU (model/update.py:45-60) on
// gfx950, inference only.
//
//   z  = sigmoid(bz + convz([h, x]))        r = sigmoid(br + convr([h, x]))
//   q  = tanh(bq + convq([r*h, x]))         h' = (1 - z) * h + z * q
//
// dir 0: the 1x5 convolutions (padding (0,2)); dir 1: the 5x1 ones (padding (2,0)).  q's
// convolution reads r*h at neighbouring pixels, so a half step is two launches of one kernel:
//   gates:      rows = convz, convr stacked (256); epilogue writes z and r*h [B][128][H][W]
//               (r itself is never stored);
//   candidate:  rows = convq over [r*h, x] (128); epilogue reads z and h at its own pixels and
//               writes h'.
// Both are the implicit GEMM
//   out[o][pixel] = sum_chunk sum_tap sum_{c in chunk} W[o][c][tap] * in[c][pixel + (tap - 2) step]
// with K = 5 C in steps of 32 channels (channel chunk outer, tap inner: a fixed order), on
// the 16x16x32 bf16 MFMA with the build's exact three-piece split (x = hi + mid + lo, six
// products per fp32 product in the family's order, corr_bf16x6.h, two accumulators joined by
// split_sum: no narrower than fp32, no scales).
//
// Workgroup = 4 waves = 64 output rows x one tile of 4 rows x 16 columns of one batch item's
// map; wave w owns rows 32 (w & 1) .. + 32 and tile rows 2 (w >> 1), + 1 (two 16x16 output tiles
// by two pixel tiles, 8 accumulators).  Per channel chunk the workgroup stages the tile plus
// its 2-pixel halo along dir (4 x 20 positions for dir 0, 8 x 16 for dir 1; zero outside the
// map, so a halo never reads the neighbouring row or batch item) from fp32 global memory —
// channels below 128 from the h (or r*h) pointer, the rest from x, so there is no cat — through
// split3 into LDS as bf16 pieces [piece][position][channel pair]; the next chunk's values are
// loaded into registers two chunks ahead.  The B fragment of tap t is the
// same LDS tile read at a position offset (t for dir 0, 16 t for dir 1).  The weights are
// pre-split once (gru_pack_kernel) into A-fragment order [16-row block][chunk][tap][piece][lane]
// and streamed from L2 four K steps ahead.  No atomics, no scratch, nothing allocated.
//
// Non-finite inputs give fp32's pattern (an infinite operand splits as (inf, 0, 0) and split_sum
// keeps the infinite leading sum; tests/test_bf16x6_family.py); finite inputs give finite outputs.
//
// `precision` (CORR_PREC_*) selects the kernel's NP: the reduced modes stage, fetch and multiply
// only the first two pieces (bf16x3, three products) or the first one (bf16, one product, one
// accumulator) of both operands, from the same pack (corr_bf16x6.h).
#include <cmath>

#include "corr_bf16x6.h"
#include "corr_build_common.h"  // align256
#include "corr_common.h"

namespace corr {
namespace {

constexpr int kGruH = 128;                  // hidden channels
constexpr int kGruTW = 16, kGruTH = 4;      // pixel tile (columns x rows)
constexpr int kGruOB = 64;                  // output rows per workgroup
constexpr int kGruNT = 256;                 // threads
constexpr int kGruXS = 16 + 4;              // words per LDS position: 16 channel pairs + pad (16-B rows)
constexpr int kGruTaps = 5;
// Waves per SIMD the kernel is compiled for, by the pieces it keeps (2: <= 256 registers; 3: <= 168).
// One piece needs 132 .. 152 registers; two pieces need 208 .. 224 and spill at 168.
constexpr int gru_waves(int np) { return np == 1 ? 3 : 2; }
constexpr int kGruAhead = 4;                // K steps the weight fragments run ahead (< kGruTaps)
constexpr int kGruBlocks = 3 * kGruH / 16;  // 16-row blocks of the pack: z, r, q

template <int DIR>
struct GruTile {
    static constexpr int PW = kGruTW + (DIR == 0 ? 4 : 0);  // staged positions per row
    static constexpr int PH = kGruTH + (DIR == 1 ? 4 : 0);  // staged rows
    static constexpr int NPOS = PW * PH;                    // 80 / 128
    static constexpr int TSTEP = DIR == 0 ? 1 : PW;         // positions per tap
    static constexpr int NLD = NPOS * 16 / kGruNT;          // channel pairs staged per thread: 5 / 8
    static_assert(NPOS * 16 % kGruNT == 0, "whole staging passes");
};

// wz, wr, wq [128][C][5] fp32 -> pieces [24 row blocks][C/32 chunks][5 taps][hi, mid, lo][64 lanes]
// in the 16x16x32 A-fragment order: lane = 16 kg + r holds W[16 ob + r][32 chunk + 8 kg + j][tap],
// j < 8, of the stacked rows (z: 0..127, r: 128..255, q: 256..383).  One block per (chunk, ob).
__global__ __launch_bounds__(64) void gru_pack_kernel(const float *__restrict__ wz, const float *__restrict__ wr,
                                                      const float *__restrict__ wq, int C,
                                                      u32x4 *__restrict__ frag) {
    const int ch = blockIdx.x, ob = blockIdx.y, lane = threadIdx.x;
    const int row = 16 * ob + (lane & 15), c0 = 32 * ch + 8 * (lane >> 4);
    const float *w = row < kGruH ? wz : row < 2 * kGruH ? wr : wq;
    const float *src = w + ((size_t)(row & (kGruH - 1)) * C + c0) * kGruTaps;
    const int NC = C / 32;
#pragma unroll
    for (int t = 0; t < kGruTaps; ++t) {
        unsigned h[4], m[4], lo[4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
            split3(src[(2 * j) * kGruTaps + t], src[(2 * j + 1) * kGruTaps + t], h[j], m[j], lo[j]);
        u32x4 *dst = frag + ((((size_t)ob * NC + ch) * kGruTaps + t) * 3) * 64 + lane;
        store_pieces(dst, h, m, lo);
    }
}

struct GruArgs {
    const float *a;     // channels < 128 of the convolution's input: h (gates), r*h (candidate)
    const float *x;     // the other `input` channels
    const float *h;     // the state, read by both epilogues
    const float *b0;    // bz (gates) / bq (candidate)
    const float *b1;    // br (gates)
    const u32x4 *frag;  // the pack
    float *z;           // gates: written; candidate: read
    float *rh;          // gates: written
    float *hout;        // candidate: written
    int B, input, H, W, tx, ty;
};

// NP: the pieces kept per operand (3 = bf16x6, 2 = bf16x3, 1 = bf16; products<NP>, corr_bf16x6.h).
// The pack is the same for every NP: a reduced mode skips the 1-KB runs of the pieces it drops.
template <bool GATES, int DIR, int NP>
__global__ __launch_bounds__(kGruNT, gru_waves(NP)) void gru_kernel(GruArgs g) {
    using T = GruTile<DIR>;
    __shared__ __attribute__((aligned(16))) unsigned xs[NP][T::NPOS][kGruXS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = g.H, W = g.W;
    const size_t HW = (size_t)H * W;
    const int tiles = g.tx * g.ty;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int y0 = (tl / g.tx) * kGruTH, x0 = (tl % g.tx) * kGruTW;
    const int NC = (kGruH + g.input) / 32, NS = NC * kGruTaps;

    // ---- staging: pass i of this thread is channel pair kp[i] at position ps[i] ----
    int ps[T::NLD], kp[T::NLD];
    long off[T::NLD];   // float offset inside a batch item's chunk (0 for a position outside the map)
    unsigned inmap = 0;  // bit i: pass i's position is inside the map (else its values are zero)
#pragma unroll
    for (int i = 0; i < T::NLD; ++i) {
        const int idx = tid + kGruNT * i;
        kp[i] = idx / T::NPOS;
        ps[i] = idx - kp[i] * T::NPOS;
        const int y = y0 + ps[i] / T::PW - (DIR == 1 ? 2 : 0), x = x0 + ps[i] % T::PW - (DIR == 0 ? 2 : 0);
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        off[i] = in ? (long)(2 * kp[i]) * (long)HW + (long)y * W + x : 0;
        inmap |= (unsigned)in << i;
    }
    // (every load is unconditional, from a valid address, and the zero of a position outside the
    // map is applied at the split: a select on the loaded value would wait for it right here)
    auto load_chunk = [&](int ch, float (&v)[T::NLD][2]) {
        const int c0 = 32 * ch;
        const float *src = c0 < kGruH ? g.a + ((size_t)b * kGruH + c0) * HW
                                      : g.x + ((size_t)b * g.input + (c0 - kGruH)) * HW;
#pragma unroll
        for (int i = 0; i < T::NLD; ++i) {
            v[i][0] = src[off[i]];
            v[i][1] = src[off[i] + HW];
        }
    };

    // ---- A fragments: row blocks ob0, ob0 + 1 of the pack, K step s = 5 chunk + tap ----
    const int ob0 = (GATES ? 0 : 2 * kGruH / 16) + (int)blockIdx.y * (kGruOB / 16) + 2 * (w & 1);
    auto load_a = [&](u32x4 (&wa)[2][NP], int s) {
        s = s < NS ? s : NS - 1;  // the last steps re-read the last fragment
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const size_t base = ((size_t)(ob0 + t) * NS + s) * 3 * 64 + lane;
#pragma unroll
            for (int p = 0; p < NP; ++p) wa[t][p] = g.frag[base + 64 * p];
        }
    };

    const int fr = lane & 15, fk = 4 * (lane >> 4);  // B fragment: column fr, channel pairs fk .. fk + 3
    const int j0 = 2 * (w >> 1);                     // this wave's tile rows j0, j0 + 1
    f32x4 acc[2][2], acs[2][2];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[t][c] = acs[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
    // The weights run kGruAhead K steps ahead of the products in a ring of one slot per tap (step
    // s = 5 chunk + tap lives in slot tap), the activations two chunks ahead in two register
    // sets: at DSEC a CU holds one or two workgroups, too few to hide an L2 round trip per step.
    u32x4 wa[kGruTaps][2][NP];
    float va[T::NLD][2], vb[T::NLD][2];
    load_chunk(0, va);
    load_chunk(NC > 1 ? 1 : 0, vb);
#pragma unroll
    for (int s = 0; s < kGruAhead; ++s) load_a(wa[s], s);
    auto chunk = [&](int ch, float (&v)[T::NLD][2]) {
#pragma unroll
        for (int i = 0; i < T::NLD; ++i) {
            unsigned hi, mid, lo;
            const bool in = (inmap >> i) & 1;
            split3(in ? v[i][0] : 0.f, in ? v[i][1] : 0.f, hi, mid, lo);
            xs[0][ps[i]][kp[i]] = hi;
            if constexpr (NP > 1) xs[1][ps[i]][kp[i]] = mid;
            if constexpr (NP > 2) xs[2][ps[i]][kp[i]] = lo;
        }
        __syncthreads();
        load_chunk(ch + 2 < NC ? ch + 2 : NC - 1, v);  // (past the end: a harmless re-read)
#pragma unroll
        for (int tap = 0; tap < kGruTaps; ++tap) {
            load_a(wa[(tap + kGruAhead) % kGruTaps], ch * kGruTaps + tap + kGruAhead);
            u32x4 xb[2][NP];
#pragma unroll
            for (int c = 0; c < 2; ++c)
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    xb[c][p] = *reinterpret_cast<const u32x4 *>(&xs[p][(j0 + c) * T::PW + fr + tap * T::TSTEP][fk]);
#pragma unroll
            for (int t = 0; t < 2; ++t)
#pragma unroll
                for (int c = 0; c < 2; ++c) products<NP>(wa[tap][t], xb[c], acc[t][c], acs[t][c]);
        }
        __syncthreads();
    };
    int ch = 0;
#pragma unroll 1
    for (; ch + 1 < NC; ch += 2) {
        chunk(ch, va);
        chunk(ch + 1, vb);
    }
    if (ch < NC) chunk(ch, va);

    // ---- epilogue: C[row = 4 (lane >> 4) + r][col = lane & 15] ----
    const int x = x0 + fr;
    if (x >= W) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int y = y0 + j0 + c;
        if (y >= H) continue;
        const size_t n = (size_t)y * W + x;
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = (int)blockIdx.y * kGruOB + 32 * (w & 1) + 16 * t + 4 * (lane >> 4) + r;
                const int o = row & (kGruH - 1);
                const size_t at = ((size_t)b * kGruH + o) * HW + n;
                const float s = NP == 1 ? acc[t][c][r] : split_sum(acc[t][c][r], acs[t][c][r]);
                if constexpr (GATES) {
                    if (row < kGruH) {
                        g.z[at] = 1.0f / (1.0f + expf(-(s + g.b0[o])));
                    } else {
                        const float rr = 1.0f / (1.0f + expf(-(s + g.b1[o])));
                        g.rh[at] = rr * g.h[at];
                    }
                } else {
                    const float q = tanhf(s + g.b0[o]);
                    const float z = g.z[at];
                    g.hout[at] = (1.0f - z) * g.h[at] + z * q;
                }
            }
    }
}

template <bool GATES, int NP>
void launch_gru(const GruArgs &g, int dir, hipStream_t s) {
    const dim3 grid((unsigned)g.B * g.tx * g.ty, (GATES ? 2 : 1) * kGruH / kGruOB);
    if (dir == 0) hipLaunchKernelGGL((gru_kernel<GATES, 0, NP>), grid, dim3(kGruNT), 0, s, g);
    else hipLaunchKernelGGL((gru_kernel<GATES, 1, NP>), grid, dim3(kGruNT), 0, s, g);
}

template <int NP>
hipError_t launch_gru_pair(GruArgs &g, int dir, const float *bq, hipStream_t s) {
    launch_gru<true, NP>(g, dir, s);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    g.a = g.rh, g.b0 = bq, g.b1 = nullptr;
    launch_gru<false, NP>(g, dir, s);
    return hipGetLastError();
}

}  // namespace

bool gru_supported(int hidden, int input) {
    return hidden == kGruH && input >= 0 && (hidden + input) % 32 == 0 && hidden + input <= 1024;
}

size_t gru_weights_bytes(int hidden, int input) {
    return (size_t)kGruBlocks * ((hidden + input) / 32) * kGruTaps * 3 * 64 * sizeof(u32x4);
}

// z, then r*h: [B][hidden][H][W] fp32 each, each rounded up to 256 bytes.
size_t gru_workspace(int B, int hidden, int H, int W) {
    return 2 * align256((size_t)B * hidden * H * W * sizeof(float));
}

hipError_t launch_gru_pack(const float *wz, const float *wr, const float *wq, int hidden, int input, void *packed,
                           hipStream_t s) {
    if (!gru_supported(hidden, input)) return hipErrorInvalidValue;
    const int C = hidden + input;
    hipLaunchKernelGGL(gru_pack_kernel, dim3(C / 32, kGruBlocks), dim3(64), 0, s, wz, wr, wq, C,
                       static_cast<u32x4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_gru_half_step(const float *h, const float *x, int B, int hidden, int input, int H, int W, int dir,
                                const void *packed, const float *bz, const float *br, const float *bq, void *ws,
                                float *h_out, hipStream_t s, int precision) {
    if (!gru_supported(hidden, input) || (dir != 0 && dir != 1) || !precision_supported(precision))
        return hipErrorInvalidValue;
    GruArgs g{};
    g.x = x;
    g.h = h;
    g.frag = static_cast<const u32x4 *>(packed);
    g.z = static_cast<float *>(ws);
    g.rh = reinterpret_cast<float *>(static_cast<char *>(ws) + gru_workspace(B, hidden, H, W) / 2);
    g.hout = h_out;
    g.B = B, g.input = input, g.H = H, g.W = W;
    g.tx = (W + kGruTW - 1) / kGruTW, g.ty = (H + kGruTH - 1) / kGruTH;
    g.a = h, g.b0 = bz, g.b1 = br;
    switch (precision) {
        case 1: return launch_gru_pair<2>(g, dir, bq, s);
        case 2: return launch_gru_pair<1>(g, dir, bq, s);
        default: return launch_gru_pair<3>(g, dir, bq, s);
    }
}

}  // namespace corr
