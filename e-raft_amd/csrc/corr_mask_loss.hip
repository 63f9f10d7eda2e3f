// corr_mask_loss.hip — the training tail with the mask head inside it: the update block's mask head
// (mask[2], 256 -> 576 1x1, and its 0.25), the convex upsampling and the sequence loss in one launch
// per direction on gfx950, so the 576-channel mask is neither stored nor saved for backward.
//
//   z[64k + 8i + j] = bias + sum_c W[64k + 8i + j][c] hidden[n][off + c][y][x]        (bf16x6)
//   p = softmax over the 9 taps of mask_scale z;  pred_c = sum_k p_k u_kc,  u_kc = 8 flow_c at tap k
//   forward : the six fp64 words of include/corr_mi355x_train.h over the cropped prediction
//   backward: G_c = scale v sign(pred_c - gt_c);  dv_k = G_0 u_k0 + G_1 u_k1
//             dz_k = mask_scale p_k (dv_k - sum_k' p_k' dv_k'),   S_kc = sum_{i,j} p_k G_c
//             (launch_convex_upsample_bwd_flow turns the 18 S planes into dflow)
//
// Both kernels are mask_upsample_kernel (corr_mask_upsample.hip) up to its store: the same
// staging, LDS layout, weight ring over the same pack, MFMA loop and softmax / combination, op
// for op, so a sub-pixel's prediction carries the bits corr_mask_upsample_forward stores.  A lane
// (wave q, lane group gq, column fr) holds, per 16-pixel block, the nine logits of pixel fr at
// sub-pixels i = 2q + (gq >> 1), j = 4 (gq & 1) .. + 3.  The loss lives on H x W with the pad
// (8h - H, 8w - W) at the top and left: sub-pixel (8y + i, 8x + j) is pixel (8y + i - pad_h,
// 8x + j - pad_w); the crop can cut between a lane's four j, so gt / valid are read per element
// from clamped addresses and the term is predicated.
//
// Forward reduction (corr_loss_math.h): a thread's 2 blocks x 4 sub-pixels x 2 channels = 16 L1
// terms in fp32, then fp64 in a fixed order; one LossPartial per workgroup, summed by
// launch_loss_finalize.  Backward: a coarse pixel's 64 sub-pixels sit in 4 waves x 4 lane groups
// x 4 registers; S is summed over the registers in order, over the lane groups by two xor swaps
// and over the waves in wave order through LDS (the staging buffer, free by then).  No atomics,
// no arrival counters: two runs agree bit for bit.  dW, dbias and dhidden are not formed here
// (DESIGN §32): dz goes to memory once and the caller's convolution backward takes it.
#include <algorithm>

#include "corr_bf16x6.h"
#include "corr_common.h"
#include "corr_loss_math.h"

namespace corr {
namespace {

// (mask_upsample_kernel's constants: the two kernels read one pack and must tile alike)
constexpr int kMlK = 256;
constexpr int kMlTaps = 9;
constexpr int kMlKS = kMlK / 32;
constexpr int kMlSteps = kMlKS * kMlTaps;
constexpr int kMlNT = 256;
constexpr int kMlXS = kMlK / 2 + 4;
constexpr int kMlNP = 2;
constexpr int kMlRing = 3;
constexpr int kMlAhead = kMlRing - 1;
constexpr int kMlWaves = 2;
constexpr int kMlPX = 16 * kMlNP;
constexpr int kMlNLD = (kMlK / 2) * kMlPX / kMlNT;
static_assert(kMlTaps % kMlRing == 0, "ring slots are compile-time");
static_assert(kMlNT % kMlPX == 0 && (kMlK / 2) % (kMlNT / kMlPX) == 0, "a thread stages one pixel");
static_assert(4 * 18 * kMlPX <= 3 * kMlPX * kMlXS, "the S partials fit in the staging buffer");

enum { kFwd = 0, kFwdMetrics = 1, kBwd = 2 };

struct MaskLossArgs {
    const float *hidden;  // [N][hc][h][w]; channels off .. off + 255 are read
    const float *flow;    // [N][2][h][w]
    const float *bias;    // [576]
    const u32x4 *frag;    // mask_pack_kernel's pack
    const float *gt;      // [N][2][H][W]
    const float *valid;   // [N][H][W]
    const float *scale;   // backward: one float
    LossPartial *part;    // forward: one per workgroup
    float *dz;            // backward: [N][576][h][w]
    float *S;             // backward: [N][2][9][h][w]
    float mscale, max_flow;
    int hc, off, h, w, H, W, nxb, tiles, vec;  // nxb blocks per row, tiles = N h nxb, vec: 16-byte dz stores
};

template <int MODE>
__global__ __launch_bounds__(kMlNT, kMlWaves) void mask_loss_kernel(MaskLossArgs g) {
    __shared__ __attribute__((aligned(16))) unsigned xs[3][kMlPX][kMlXS];
    const int tid = threadIdx.x, lane = tid & 63;
    const int q = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = g.h, w = g.w;
    const size_t plane = (size_t)h * w;

    // ---- A fragments: step s = 9 (K step) + tap of this wave's quarter of the pack ----
    const u32x4 *fq = g.frag + (size_t)q * kMlSteps * 3 * 64 + lane;
    auto load_a = [&](u32x4 (&wa)[3], int s) {
        s = s < kMlSteps ? s : kMlSteps - 1;  // the last steps re-read the last fragment
#pragma unroll
        for (int p = 0; p < 3; ++p) wa[p] = fq[(size_t)(s * 3 + p) * 64];
    };
    u32x4 wa[kMlRing][3];
#pragma unroll
    for (int s = 0; s < kMlAhead; ++s) load_a(wa[s], s);

    // ---- staging: a block past the last one re-reads the last block, a pixel past w the pixel
    // w - 1: every address is inside this launch's hidden, and what comes of them is never used ----
    {
        const int px = tid % kMlPX, cp0 = tid / kMlPX;
        int t = (int)blockIdx.x * kMlNP + (px >> 4);
        t = t < g.tiles ? t : g.tiles - 1;
        const int xb = t % g.nxb, ny = t / g.nxb, y = ny % h, n = ny / h;
        const int x = min(16 * xb + (px & 15), w - 1);
        const float *src = g.hidden + ((size_t)n * g.hc + g.off) * plane + (size_t)y * w + x;
        float v[kMlNLD][2];
#pragma unroll
        for (int i = 0; i < kMlNLD; ++i) {
            const size_t c = (size_t)(2 * (cp0 + (kMlNT / kMlPX) * i));
            v[i][0] = src[c * plane];
            v[i][1] = src[(c + 1) * plane];
        }
#pragma unroll
        for (int i = 0; i < kMlNLD; ++i) {
            unsigned hi, mid, lo;
            split3(v[i][0], v[i][1], hi, mid, lo);
            const int cp = cp0 + (kMlNT / kMlPX) * i;
            xs[0][px][cp] = hi;
            xs[1][px][cp] = mid;
            xs[2][px][cp] = lo;
        }
    }
    __syncthreads();

    // ---- the logits: acc[k][p] (hi * hi) and acs[k][p] (the five smaller products) ----
    const int fr = lane & 15, gq = lane >> 4, fk = 4 * gq;
    f32x4 acc[kMlTaps][kMlNP], acs[kMlTaps][kMlNP];
#pragma unroll
    for (int k = 0; k < kMlTaps; ++k)
#pragma unroll
        for (int p = 0; p < kMlNP; ++p) acc[k][p] = acs[k][p] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int ks = 0; ks < kMlKS; ++ks) {
        u32x4 xb[kMlNP][3];
#pragma unroll
        for (int p = 0; p < kMlNP; ++p)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                xb[p][c] = *reinterpret_cast<const u32x4 *>(&xs[c][16 * p + fr][16 * ks + fk]);
#pragma unroll
        for (int k = 0; k < kMlTaps; ++k) {
            load_a(wa[(k + kMlAhead) % kMlRing], ks * kMlTaps + k + kMlAhead);
#pragma unroll
            for (int p = 0; p < kMlNP; ++p) six(wa[k % kMlRing], xb[p], acc[k][p], acs[k][p]);
        }
    }

    // ---- epilogue: lane (gq, fr) holds the nine logits of pixel fr at sub-pixels i, j0 .. j0 + 3 ----
    const int i = 2 * q + (gq >> 1), j0 = 4 * (gq & 1);
    const int H = g.H, W = g.W, pad_h = 8 * h - H, pad_w = 8 * w - W;
    const size_t HW = (size_t)H * W;
    float *red = reinterpret_cast<float *>(&xs[0][0][0]);  // backward: [wave][18 planes][pixel]
    float scale = 0.0f;
    if (MODE == kBwd) {
        scale = *g.scale;
        __syncthreads();  // every wave has read its last B fragments: xs becomes red
    }
    LossAcc la;
#pragma unroll
    for (int p = 0; p < kMlNP; ++p) {
        const int t = (int)blockIdx.x * kMlNP + p;
        const bool live = t < g.tiles;
        const int tc = live ? t : g.tiles - 1;
        const int xb = tc % g.nxb, ny = tc / g.nxb, y = ny % h, n = ny / h;
        const int x = 16 * xb + fr, xc = min(x, w - 1);
        const bool own = live && x < w;
        // (every load is unconditional, from an address inside this batch item's maps; the zero of
        // a neighbour outside the map and the crop are applied afterwards)
        const float *f0 = g.flow + (size_t)n * 2 * plane, *f1 = f0 + plane;
        float u0[kMlTaps], u1[kMlTaps];
#pragma unroll
        for (int k = 0; k < kMlTaps; ++k) {
            const int yy = y + k / 3 - 1, xx = xc + k % 3 - 1;
            const size_t o = (size_t)min(max(yy, 0), h - 1) * w + min(max(xx, 0), w - 1);
            u0[k] = f0[o];
            u1[k] = f1[o];
        }
#pragma unroll
        for (int k = 0; k < kMlTaps; ++k) {
            const int yy = y + k / 3 - 1, xx = xc + k % 3 - 1;
            const bool in = (unsigned)yy < (unsigned)h && (unsigned)xx < (unsigned)w;
            u0[k] = in ? 8.0f * u0[k] : 0.0f;
            u1[k] = in ? 8.0f * u1[k] : 0.0f;
        }
        const int Y = 8 * y + i - pad_h, X0 = 8 * xc + j0 - pad_w;  // Y < H, X0 + r < W
        const size_t row = (size_t)max(Y, 0) * W;
        const float *g0p = g.gt + (size_t)n * 2 * HW + row, *vp = g.valid + (size_t)n * HW + row;
        float t0[4], t1[4], vl[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int X = max(X0 + r, 0);
            t0[r] = g0p[X];
            t1[r] = g0p[HW + X];
            vl[r] = vp[X];
        }
        float s0[kMlTaps], s1[kMlTaps];
#pragma unroll
        for (int k = 0; k < kMlTaps; ++k) s0[k] = s1[k] = 0.0f;
        float dzv[MODE == kBwd ? kMlTaps : 1][4];  // backward: dz of channel 64 k + 8 i + j0 + r at pixel fr
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float lg[kMlTaps];
#pragma unroll
            for (int k = 0; k < kMlTaps; ++k)
                lg[k] = g.mscale * (g.bias[64 * k + 8 * i + j0 + r] + split_sum(acc[k][p][r], acs[k][p][r]));
            float mx = lg[0];
#pragma unroll
            for (int k = 1; k < kMlTaps; ++k) mx = fmaxf(mx, lg[k]);
            float e[kMlTaps], s = 0.0f;
#pragma unroll
            for (int k = 0; k < kMlTaps; ++k) {
                e[k] = expf(lg[k] - mx);
                s += e[k];
            }
            float pk[kMlTaps], a0 = 0.0f, a1 = 0.0f;
#pragma unroll
            for (int k = 0; k < kMlTaps; ++k) {
                pk[k] = e[k] / s;
                a0 += pk[k] * u0[k];
                a1 += pk[k] * u1[k];
            }
            const bool keep = own && Y >= 0 && X0 + r >= 0;
            if (MODE != kBwd) {
                if (keep) loss_term<MODE == kFwdMetrics>(la, a0, a1, t0[r], t1[r], vl[r], g.max_flow);
            } else {
                const float sv = scale * loss_valid(vl[r], t0[r], t1[r], g.max_flow);
                const float g0 = sv * loss_sign(a0 - t0[r]), g1 = sv * loss_sign(a1 - t1[r]);
                float dv[kMlTaps], pdv = 0.0f;
#pragma unroll
                for (int k = 0; k < kMlTaps; ++k) {
                    dv[k] = g0 * u0[k] + g1 * u1[k];
                    pdv += pk[k] * dv[k];
                }
#pragma unroll
                for (int k = 0; k < kMlTaps; ++k) {
                    dzv[k][r] = keep ? g.mscale * (pk[k] * (dv[k] - pdv)) : 0.0f;
                    s0[k] += keep ? pk[k] * g0 : 0.0f;
                    s1[k] += keep ? pk[k] * g1 : 0.0f;
                }
            }
        }
        if (MODE == kBwd) {
            float *dzp = g.dz + ((size_t)n * 576 + 8 * i + j0) * plane + (size_t)y * w;
            if (g.vec) {  // uniform: w % 4 == 0 and dz 16-byte aligned
                // 4 x 4 transposes among the lanes fr = 4 a + b of a quad (swaps over fr ^ 1, then fr ^ 2):
                // the lane then holds channel j0 + b at the pixels 4 a .. 4 a + 3, one 16-byte store per tap
                const bool o1 = fr & 1, o2 = fr & 2;
                const int x4 = 16 * xb + (fr & 12);
#pragma unroll
                for (int k = 0; k < kMlTaps; ++k) {
                    float v0 = dzv[k][0], v1 = dzv[k][1], v2 = dzv[k][2], v3 = dzv[k][3];
                    const float a1 = __shfl_xor(o1 ? v0 : v1, 1), b1 = __shfl_xor(o1 ? v2 : v3, 1);
                    v0 = o1 ? a1 : v0, v1 = o1 ? v1 : a1, v2 = o1 ? b1 : v2, v3 = o1 ? v3 : b1;
                    const float a2 = __shfl_xor(o2 ? v0 : v2, 2), b2 = __shfl_xor(o2 ? v1 : v3, 2);
                    v0 = o2 ? a2 : v0, v1 = o2 ? b2 : v1, v2 = o2 ? v2 : a2, v3 = o2 ? v3 : b2;
                    if (live && x4 < w)
                        *reinterpret_cast<f32x4 *>(dzp + ((size_t)64 * k + (fr & 3)) * plane + x4) = f32x4{v0, v1, v2, v3};
                }
            } else if (own) {
#pragma unroll
                for (int k = 0; k < kMlTaps; ++k)
#pragma unroll
                    for (int r = 0; r < 4; ++r) dzp[((size_t)64 * k + r) * plane + x] = dzv[k][r];
            }
#pragma unroll
            for (int k = 0; k < kMlTaps; ++k) {
                s0[k] += __shfl_xor(s0[k], 16);
                s1[k] += __shfl_xor(s1[k], 16);
                s0[k] += __shfl_xor(s0[k], 32);
                s1[k] += __shfl_xor(s1[k], 32);
            }
            if (gq == 0) {
#pragma unroll
                for (int k = 0; k < kMlTaps; ++k) {
                    red[(q * 18 + k) * kMlPX + 16 * p + fr] = s0[k];
                    red[(q * 18 + 9 + k) * kMlPX + 16 * p + fr] = s1[k];
                }
            }
        }
    }
    if (MODE != kBwd) {
        loss_block_reduce<kMlNT / 64>(la, g.part + blockIdx.x);
    } else {
        __syncthreads();
        // 18 planes x 32 pixels, each summed over the 4 waves in order
        for (int id = tid; id < 18 * kMlPX; id += kMlNT) {
            const int pl = id / kMlPX, px = id % kMlPX;
            float a = 0.0f;
#pragma unroll
            for (int v = 0; v < kMlNT / 64; ++v) a += red[(v * 18 + pl) * kMlPX + px];
            const int t = (int)blockIdx.x * kMlNP + (px >> 4);
            if (t >= g.tiles) continue;
            const int xb = t % g.nxb, ny = t / g.nxb, y = ny % h, n = ny / h;
            const int x = 16 * xb + (px & 15);
            if (x < w) g.S[((size_t)n * 18 + pl) * plane + (size_t)y * w + x] = a;
        }
    }
}

MaskLossArgs make_args(const float *hidden, int hc, int off, const float *flow, const void *packed,
                       const float *bias, float mask_scale, const float *gt, const float *valid, int N, int h, int w,
                       int H, int W, float max_flow) {
    MaskLossArgs g{};
    g.hidden = hidden, g.flow = flow, g.bias = bias, g.frag = static_cast<const u32x4 *>(packed);
    g.gt = gt, g.valid = valid, g.mscale = mask_scale, g.max_flow = max_flow;
    g.hc = hc, g.off = off, g.h = h, g.w = w, g.H = H, g.W = W;
    g.nxb = (w + 15) / 16;
    g.tiles = N * h * g.nxb;  // <= N h w < 2^31
    return g;
}

size_t workgroups(int N, int h, int w) { return ((size_t)N * h * ((w + 15) / 16) + kMlNP - 1) / kMlNP; }

}  // namespace

// The backward's 18 S planes or the forward's per-workgroup partials, whichever is larger.
size_t mask_upsample_loss_workspace(int N, int h, int w) {
    return std::max(convex_upsample_bwd_workspace(N, h, w), workgroups(N, h, w) * sizeof(LossPartial));
}

hipError_t launch_mask_upsample_loss(const float *hidden, int hidden_channels, int hidden_offset, const float *flow,
                                     const void *packed, const float *bias, float mask_scale, const float *gt,
                                     const float *valid, int N, int h, int w, int H, int W, float max_flow,
                                     bool metrics, double *out, void *ws, hipStream_t s) {
    MaskLossArgs g = make_args(hidden, hidden_channels, hidden_offset, flow, packed, bias, mask_scale, gt, valid, N,
                               h, w, H, W, max_flow);
    g.part = static_cast<LossPartial *>(ws);
    const size_t blocks = workgroups(N, h, w);
    if (metrics)
        hipLaunchKernelGGL(mask_loss_kernel<kFwdMetrics>, dim3((unsigned)blocks), dim3(kMlNT), 0, s, g);
    else
        hipLaunchKernelGGL(mask_loss_kernel<kFwd>, dim3((unsigned)blocks), dim3(kMlNT), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_loss_finalize(ws, blocks, out, s);
}

hipError_t launch_mask_upsample_loss_bwd(const float *hidden, int hidden_channels, int hidden_offset,
                                         const float *flow, const void *packed, const float *bias, float mask_scale,
                                         const float *gt, const float *valid, const float *scale, int N, int h,
                                         int w, int H, int W, float max_flow, float *dflow, float *dz, void *ws,
                                         hipStream_t s) {
    MaskLossArgs g = make_args(hidden, hidden_channels, hidden_offset, flow, packed, bias, mask_scale, gt, valid, N,
                               h, w, H, W, max_flow);
    g.scale = scale, g.dz = dz, g.S = static_cast<float *>(ws);
    g.vec = w % 4 == 0 && (uintptr_t)dz % 16 == 0;  // (every channel's every row then is 16-byte aligned)
    hipLaunchKernelGGL(mask_loss_kernel<kBwd>, dim3((unsigned)workgroups(N, h, w)), dim3(kMlNT), 0, s, g);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_convex_upsample_bwd_flow(g.S, N, h, w, dflow, s);
}

}  // namespace corr
