// corr_flow.hip — the two ends of the update block that touch the flow (model/update.py:63-82 and
// 20-31), on gfx950, inference only: the motion encoder's 7x7 convolution of the 2-channel flow
// (convf1) and the flow head's 3x3 convolution from 256 to 2 channels (flow_head.conv2) with the
// coordinate update that follows it in the refinement loop (model/eraft.py:128-134).
//
//   enc:   out[b][oo + o][y][x] = act(bias[o] + sum_tap sum_c w[o][c][tap] flow[b][c][y + ky - 3][x + kx - 3])
//          copy[b][co + c][y][x] = flow[b][c][y][x]                      (optional, bit for bit)
//   head:  delta[b][o][y][x] = bias[o] + sum_tap (sum_c w[o][c][tap] hidden[b][off + c][y + ky - 1][x + kx - 1])
//          coords_out = coords_in + delta;  flow_out = coords_out - coords0   (optional)
//
// The arithmetic is corr_conv.hip's: the 16x16x32 bf16 MFMA with the build's exact three-piece split
// (x = hi + mid + lo, six products per fp32 product in the family's order (corr_bf16x6.h), two accumulators
// joined by split_sum), every following fp32 operation rounded once.
//
// Encoder.  K = 98 is tap-major, tap = 7 ky + kx ascending with the two channels of a tap adjacent
// (k = 2 tap + c), padded with zero weights to 128: four K steps of 16 taps.  The workgroup is
// corr_enc_front.hip's stem at stride 1: 4 waves, a tile of 4 rows x 16 columns of one batch item,
// wave w owning the two 16-row blocks of half w & 1 (64 output rows a workgroup) and the tile rows
// 2 (w >> 1), + 1.  The tile's 10 x 22 window is staged once through split3 into LDS, one word (a
// channel pair) per position and piece; a lane's B fragment of a step is the four words of its four
// taps.  The padded taps 49 .. 63 re-read tap 48's position against zero weights.
//
// Head.  Two output rows would leave 14 of an MFMA tile's 16 rows idle, so the convolution is taken
// apart: P[o][tap][pixel] = sum_c w[o][c][tap] hidden[c][pixel] is a 1x1 product over K = 256 in
// ascending 32-channel steps (row block o, row = tap: 9 of 16 rows live), evaluated on the tile
// plus its 1-pixel halo; a pixel outside the map gets P = 0 (the zero padding).  The nine taps of
// an output are then added from LDS in ascending tap order, then the bias: this is NOT
// corr_conv_forward's order (chunk outer, tap inner in one accumulator).  A workgroup owns 2 rows
// x 14 columns of output; its halo is 4 rows of 16 pixels, one row per wave, and a lane loads and
// splits its pixel's channels straight from global memory (no wave shares another's pixels, so the
// activations do not pass through LDS).
//
// Every load is unconditional, from an address clamped into the same map; a zero is applied to
// the loaded value (or the product) afterwards.  No atomics, no scratch, nothing allocated.
// Non-finite inputs: the head gives fp32's pattern (corr_conv.hip's note applies); the encoder is
// not parity-checked on them.
#include "corr_bf16x6.h"
#include "corr_common.h"

namespace corr {
namespace {

constexpr int kTW = kConvTW, kTH = kConvTH, kNT = kConvNT, kPad = kConvPad;  // the family's tile (corr_bf16x6.h)
constexpr int kFeT = 2;            // 16-row blocks per wave: 64 output rows per workgroup
constexpr int kFeK = 7, kFeTaps = 49, kFeSteps = 4, kFeStepTaps = 16;
constexpr int kFePW = kTW + kFeK - 1;   // staged positions per row: 22
constexpr int kFePH = kTH + kFeK - 1;   // staged rows: 10
constexpr int kFeNPOS = kFePW * kFePH;  // 220: one staging pass
static_assert(kFeNPOS <= kNT && 2 * kTH * kTW <= kNT, "one pass stages the window and copies the tile");

constexpr int kFhC = 256, kFhKS = kFhC / 32, kFhTaps = 9;
constexpr int kFhTW = 14, kFhTH = 2;   // output tile; with its halo kFhTH + 2 rows of 16 pixels
constexpr int kFhNB = kFhTH + 2;       // 16-pixel blocks (halo rows) per workgroup
static_assert(2 * kFhTH * kFhTW <= kNT, "one thread per output value");

// ---------------------------------------------------------------------------------------------
// encoder: 7x7, 2 -> cout
// ---------------------------------------------------------------------------------------------
// w [cout][2][7][7] fp32 -> pieces [rows/16 blocks][4 steps][hi, mid, lo][64 lanes] in the 16x16x32
// A-fragment order: lane = 16 kg + r holds, in word j < 4, the channel pair (0, 1) of
// W[16 ob + r][.][tap 16 s + 4 kg + j]; rows >= cout and taps >= 49 are zero.  One block per
// (step, ob).
__global__ __launch_bounds__(64) void flow_enc_pack_kernel(const float *__restrict__ w, int cout,
                                                           u32x4 *__restrict__ frag) {
    const int s = blockIdx.x, ob = blockIdx.y, lane = threadIdx.x;
    const int row = 16 * ob + (lane & 15), kg = lane >> 4;
    unsigned h[4], m[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int tap = kFeStepTaps * s + 4 * kg + j;
        const bool live = row < cout && tap < kFeTaps;
        const float *src = w + (size_t)(live ? row : 0) * 2 * kFeTaps + (live ? tap : 0);
        const float a = src[0], b = src[kFeTaps];
        split3(live ? a : 0.f, live ? b : 0.f, h[j], m[j], lo[j]);
    }
    u32x4 *dst = frag + (((size_t)ob * kFeSteps + s) * 3) * 64 + lane;
    store_pieces(dst, h, m, lo);
}

struct FlowEncArgs {
    const float *flow;   // [B][2][H][W]
    const float *bias;   // [cout], or null for no bias
    const u32x4 *frag;   // the pack
    float *out;          // [B][oc][H][W]; channels oo .. oo + cout - 1 are written
    float *copy;         // null, or [B][cc][H][W]; channels co, co + 1 receive the flow
    int H, W, cout, oc, oo, cc, co, tx, ty, relu;
};

__global__ __launch_bounds__(kNT) void flow_enc_kernel(FlowEncArgs g) {
    __shared__ unsigned xs[3][kFeNPOS];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = g.H, W = g.W;
    const size_t HW = (size_t)H * W;
    const int tiles = g.tx * g.ty;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int y0 = (tl / g.tx) * kTH, x0 = (tl % g.tx) * kTW;
    const float *src = g.flow + (size_t)b * 2 * HW;

    // ---- staging: thread = window position (the threads past the window re-read the last one) ----
    {
        const int ps = min(tid, kFeNPOS - 1);
        const int y = y0 + ps / kFePW - 3, x = x0 + ps % kFePW - 3;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        const size_t off = (size_t)min(max(y, 0), H - 1) * W + min(max(x, 0), W - 1);
        const float a = src[off], c = src[HW + off];
        unsigned hi, mid, lo;
        split3(in ? a : 0.f, in ? c : 0.f, hi, mid, lo);
        if (tid < kFeNPOS) {
            xs[0][ps] = hi;
            xs[1][ps] = mid;
            xs[2][ps] = lo;
        }
    }
    // ---- the pass-through: the first row group's workgroup copies its tile's flow (waves 0, 1) ----
    if (g.copy && blockIdx.y == 0 && tid < 2 * kTH * kTW) {
        const int c = tid >> 6, y = y0 + (lane >> 4), x = x0 + (lane & 15);
        const size_t off = (size_t)min(y, H - 1) * W + min(x, W - 1);
        const float v = src[(size_t)c * HW + off];
        if (y < H && x < W) g.copy[((size_t)b * g.cc + g.co + c) * HW + off] = v;
    }
    __syncthreads();

    // ---- K loop: lane = 16 kg + fr reads taps 16 s + 4 kg .. + 3 of output column fr ----
    const int fr = lane & 15, kg = lane >> 4, j0 = 2 * (w >> 1);
    const int ob0 = (int)blockIdx.y * (2 * kFeT) + kFeT * (w & 1);
    f32x4 acc[kFeT][2], acs[kFeT][2];
#pragma unroll
    for (int t = 0; t < kFeT; ++t)
#pragma unroll
        for (int c = 0; c < 2; ++c) acc[t][c] = acs[t][c] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < kFeSteps; ++s) {
        u32x4 wa[kFeT][3];
#pragma unroll
        for (int t = 0; t < kFeT; ++t)
#pragma unroll
            for (int p = 0; p < 3; ++p) wa[t][p] = g.frag[(((size_t)(ob0 + t) * kFeSteps + s) * 3 + p) * 64 + lane];
        int toff[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int tap = min(kFeStepTaps * s + 4 * kg + j, kFeTaps - 1);
            toff[j] = (tap / kFeK) * kFePW + tap % kFeK;
        }
        u32x4 xb[2][3];
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int p = 0; p < 3; ++p) {
                const unsigned *q = &xs[p][(j0 + c) * kFePW + fr];
                xb[c][p] = u32x4{q[toff[0]], q[toff[1]], q[toff[2]], q[toff[3]]};
            }
#pragma unroll
        for (int t = 0; t < kFeT; ++t)
#pragma unroll
            for (int c = 0; c < 2; ++c) six(wa[t], xb[c], acc[t][c], acs[t][c]);
    }

    // ---- epilogue: C[row = 4 (lane >> 4) + r][col = lane & 15] of row block t, tile row j0 + c ----
    const int x = x0 + fr;
#pragma unroll
    for (int t = 0; t < kFeT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = (int)blockIdx.y * (32 * kFeT) + 16 * (kFeT * (w & 1) + t) + 4 * kg + r;
            const bool live = row < g.cout;  // else a padding row of the pack
            const float bs = g.bias && live ? g.bias[row] : 0.f;
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const int y = y0 + j0 + c;
                float v = split_sum(acc[t][c][r], acs[t][c][r]) + bs;
                if (g.relu) v = v < 0.f ? 0.f : v;
                if (live && x < W && y < H) g.out[((size_t)b * g.oc + g.oo + row) * HW + (size_t)y * W + x] = v;
            }
        }
}

// ---------------------------------------------------------------------------------------------
// head: 3x3, 256 -> 2, + the coordinate update
// ---------------------------------------------------------------------------------------------
// w [2][256][3][3] fp32 -> pieces [2 o][8 K steps][hi, mid, lo][64 lanes] in the 16x16x32 A-fragment
// order: lane = 16 kg + r holds W[o][32 step + 8 kg + j][tap r], j < 8; rows r >= 9 are zero.  One
// block per (step, o).
__global__ __launch_bounds__(64) void flow_head_pack_kernel(const float *__restrict__ w, u32x4 *__restrict__ frag) {
    const int ks = blockIdx.x, o = blockIdx.y, lane = threadIdx.x;
    const int tap = lane & 15, c0 = 32 * ks + 8 * (lane >> 4);
    const bool live = tap < kFhTaps;
    const float *src = w + ((size_t)o * kFhC + c0) * kFhTaps + (live ? tap : 0);
    unsigned h[4], m[4], lo[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float a = src[(2 * j) * kFhTaps], b = src[(2 * j + 1) * kFhTaps];
        split3(live ? a : 0.f, live ? b : 0.f, h[j], m[j], lo[j]);
    }
    u32x4 *dst = frag + (((size_t)o * kFhKS + ks) * 3) * 64 + lane;
    store_pieces(dst, h, m, lo);
}

struct FlowHeadArgs {
    const float *hidden;     // [B][hc][H][W]; channels off .. off + 255 are read
    const float *bias;       // [2]
    const u32x4 *frag;       // the pack
    const float *coords_in;  // null, or [B][2][H][W]
    const float *coords0;    // null, or [B][2][H][W]
    float *delta, *coords_out, *flow_out;  // [B][2][H][W] each
    int hc, off, H, W, tx, ty;
};

__global__ __launch_bounds__(kNT) void flow_head_kernel(FlowHeadArgs g) {
    __shared__ float P[2][kFhTaps][kFhNB][16];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int H = g.H, W = g.W;
    const size_t HW = (size_t)H * W;
    const int tiles = g.tx * g.ty;
    const int b = blockIdx.x / tiles, tl = blockIdx.x - b * tiles;
    const int y0 = (tl / g.tx) * kFhTH, x0 = (tl % g.tx) * kFhTW;
    const int fr = lane & 15, kg = lane >> 4;

    // ---- P of halo row blk: lane = 16 kg + fr holds channels 32 ks + 8 kg .. + 7 of pixel fr ----
    for (int blk = w; blk < kFhNB; blk += kNT / 64) {
        const int y = y0 - 1 + blk, x = x0 - 1 + fr;
        const bool in = (unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W;
        const float *src = g.hidden + ((size_t)b * g.hc + g.off + 8 * kg) * HW + (size_t)min(max(y, 0), H - 1) * W +
                           min(max(x, 0), W - 1);
        float v[kFhKS][8];
#pragma unroll
        for (int ks = 0; ks < kFhKS; ++ks)
#pragma unroll
            for (int j = 0; j < 8; ++j) v[ks][j] = src[(size_t)(32 * ks + j) * HW];
        f32x4 acc[2], acs[2];
        acc[0] = acc[1] = acs[0] = acs[1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ks = 0; ks < kFhKS; ++ks) {
            unsigned h[4], m[4], lo[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) split3(v[ks][2 * j], v[ks][2 * j + 1], h[j], m[j], lo[j]);
            const u32x4 xb[3] = {u32x4{h[0], h[1], h[2], h[3]}, u32x4{m[0], m[1], m[2], m[3]},
                                 u32x4{lo[0], lo[1], lo[2], lo[3]}};
#pragma unroll
            for (int o = 0; o < 2; ++o) {
                u32x4 wa[3];
#pragma unroll
                for (int p = 0; p < 3; ++p) wa[p] = g.frag[(((size_t)o * kFhKS + ks) * 3 + p) * 64 + lane];
                six(wa, xb, acc[o], acs[o]);
            }
        }
        // C[row = 4 kg + r][col = fr]: row = tap.  A pixel outside the map contributes zero.
#pragma unroll
        for (int o = 0; o < 2; ++o)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tap = 4 * kg + r;
                if (tap < kFhTaps) P[o][tap][blk][fr] = in ? split_sum(acc[o][r], acs[o][r]) : 0.f;
            }
    }
    __syncthreads();

    // ---- shift and add: thread = (o, tile pixel); taps ascending, then the bias ----
    if (tid < 2 * kFhTH * kFhTW) {
        const int o = tid / (kFhTH * kFhTW), p = tid - o * (kFhTH * kFhTW);
        const int ty = p / kFhTW, tx = p - ty * kFhTW, y = y0 + ty, x = x0 + tx;
        if (y < H && x < W) {
            float s = P[o][0][ty][tx];
#pragma unroll
            for (int tap = 1; tap < kFhTaps; ++tap) s = s + P[o][tap][ty + tap / 3][tx + tap % 3];
            const float d = s + g.bias[o];
            const size_t i = ((size_t)b * 2 + o) * HW + (size_t)y * W + x;
            g.delta[i] = d;
            if (g.coords_in) {
                const float c = g.coords_in[i] + d;
                g.coords_out[i] = c;
                if (g.coords0) g.flow_out[i] = c - g.coords0[i];
            }
        }
    }
}

constexpr int flow_rows(int cout) { return (cout + kPad - 1) / kPad * kPad; }

}  // namespace

bool flow_enc_supported(int cout) { return cout >= 1 && cout <= 1024; }

size_t flow_enc_weights_bytes(int cout) { return (size_t)(flow_rows(cout) / 16) * kFeSteps * 3 * 64 * sizeof(u32x4); }

hipError_t launch_flow_enc_pack(const float *w, int cout, void *packed, hipStream_t s) {
    if (!flow_enc_supported(cout)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(flow_enc_pack_kernel, dim3(kFeSteps, flow_rows(cout) / 16), dim3(64), 0, s, w, cout,
                       static_cast<u32x4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_flow_enc(const float *flow, int B, int H, int W, const void *packed, const float *bias, int cout,
                           int relu, float *out, int out_channels, int out_offset, float *flow_copy,
                           int copy_channels, int copy_offset, hipStream_t s) {
    if (!flow_enc_supported(cout)) return hipErrorInvalidValue;
    FlowEncArgs g{};
    g.flow = flow, g.bias = bias, g.frag = static_cast<const u32x4 *>(packed), g.out = out, g.copy = flow_copy;
    g.H = H, g.W = W, g.cout = cout, g.oc = out_channels, g.oo = out_offset, g.cc = copy_channels, g.co = copy_offset;
    g.tx = (W + kTW - 1) / kTW, g.ty = (H + kTH - 1) / kTH, g.relu = relu;
    const dim3 grid((unsigned)B * g.tx * g.ty, (cout + 32 * kFeT - 1) / (32 * kFeT));
    hipLaunchKernelGGL(flow_enc_kernel, grid, dim3(kNT), 0, s, g);
    return hipGetLastError();
}

size_t flow_head_weights_bytes() { return (size_t)2 * kFhKS * 3 * 64 * sizeof(u32x4); }

hipError_t launch_flow_head_pack(const float *w, void *packed, hipStream_t s) {
    hipLaunchKernelGGL(flow_head_pack_kernel, dim3(kFhKS, 2), dim3(64), 0, s, w, static_cast<u32x4 *>(packed));
    return hipGetLastError();
}

hipError_t launch_flow_head(const float *hidden, int hidden_channels, int hidden_offset, int B, int H, int W,
                            const void *packed, const float *bias, const float *coords_in, const float *coords0,
                            float *delta, float *coords_out, float *flow_out, hipStream_t s) {
    FlowHeadArgs g{};
    g.hidden = hidden, g.bias = bias, g.frag = static_cast<const u32x4 *>(packed);
    g.coords_in = coords_in, g.coords0 = coords_in ? coords0 : nullptr;
    g.delta = delta, g.coords_out = coords_out, g.flow_out = flow_out;
    g.hc = hidden_channels, g.off = hidden_offset, g.H = H, g.W = W;
    g.tx = (W + kFhTW - 1) / kFhTW, g.ty = (H + kFhTH - 1) / kFhTH;
    hipLaunchKernelGGL(flow_head_kernel, dim3((unsigned)B * g.tx * g.ty), dim3(kNT), 0, s, g);
    return hipGetLastError();
}

}  // namespace corr
