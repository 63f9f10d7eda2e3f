// corr_loss.hip — the training tail: the reference's sequence_loss (train.py:47-75; the L1 term of
// one prediction over the valid pixels, and the EPE / 1px / 3px / 5px metrics of the last one),
// alone over a stored prediction and fused with the convex upsampling (eraft.py:75-86) so that no
// full-resolution prediction or gradient is ever stored.
//
//   v    = (valid >= 0.5) && (sqrt(gx^2 + gy^2) < max_flow), as 0.f / 1.f, MULTIPLIED into |pred - gt|
//          (a non-finite prediction or ground truth poisons the sum where the reference's does)
//   out  = { sum v (|d0| + |d1|), n_valid, sum_valid epe, #epe<1, #epe<3, #epe<5 }   (six fp64 words)
//   bwd  : G_c = scale v sign(d_c), sign(0) = 0; scale is read from the device
//
// Fused geometry: the coarse map [N, ., h, w] upsamples to the padded frame 8h x 8w; the loss lives
// on H x W with the pad (8h - H, 8w - W) at the top and left (ImagePadder), so sub-pixel
// (8y + i, 8x + j) is pixel (8y + i - pad_h, 8x + j - pad_w) and one with a negative coordinate does
// not exist for the loss.  Both fused kernels use convex_upsample_bwd_kernel's mapping: a workgroup
// = 8 waves over 64 consecutive coarse pixels x of one row y, wave = sub-row i, lane = x, loop over
// j, so the mask logits (and dmask) are coalesced along x.  The prediction arithmetic is
// corr_upsample_math.h's, i.e. corr_convex_upsample's bits.
//
// Reduction: a thread sums its at most 16 terms in fp32; wave (xor butterfly), workgroup (LDS, wave
// order) and grid (one partial per workgroup, summed by loss_finalize_kernel over contiguous index
// ranges, then over the ranges in order) are fp64 in a fixed order; counts are integers.  No
// atomics, no arrival counter: two runs agree bit for bit.
#include <algorithm>
#include <cmath>

#include "corr_common.h"
#include "corr_loss_math.h"
#include "corr_upsample_math.h"

namespace corr {
namespace {

constexpr int kLossWaves = 8;
constexpr int kLossThreads = 64 * kLossWaves;
constexpr int kSeqPerThread = 8;                             // pixels of a thread: 16 L1 terms
constexpr int kSeqPerBlock = kLossThreads * kSeqPerThread;  // pixels of a workgroup

template <bool METRICS>
__global__ __launch_bounds__(kLossThreads) void upsample_loss_kernel(const float *__restrict__ flow,
                                                                    const float *__restrict__ mask,
                                                                    const float *__restrict__ gt,
                                                                    const float *__restrict__ valid, int h, int w,
                                                                    int H, int W, float max_flow,
                                                                    LossPartial *__restrict__ part) {
    const int nxb = (w + 63) / 64;
    const int xb = blockIdx.x % nxb, y = (blockIdx.x / nxb) % h, n = blockIdx.x / (nxb * h);
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
    const int x = xb * 64 + lane;
    const int Y = 8 * y + i - (8 * h - H), X0 = 8 * x - (8 * w - W);
    const size_t plane = (size_t)h * w;
    LossAcc acc;
    if (x < w && Y >= 0) {  // Y < H and X0 + j < W by H = 8h - pad_h, W = 8w - pad_w
        const float *f0 = flow + (size_t)n * 2 * plane, *f1 = f0 + plane;
        float u0[9], u1[9];
        upsample_taps(f0, f1, y, x, h, w, u0, u1);
        const size_t HW = (size_t)H * W;
        const float *g0p = gt + (size_t)n * 2 * HW + (size_t)Y * W, *vp = valid + (size_t)n * HW + (size_t)Y * W;
        for (int j = 0; j < 8; ++j) {
            const int X = X0 + j;
            if (X < 0) continue;
            const size_t mo = ((size_t)n * 576 + 8 * i + j) * plane + (size_t)y * w + x;
            float lg[9], e[9], p[9], a0, a1;
#pragma unroll
            for (int k = 0; k < 9; ++k) lg[k] = mask[mo + (size_t)k * 64 * plane];
            const float s = upsample_exp(lg, e);
            upsample_combine(e, s, u0, u1, p, a0, a1);
            loss_term<METRICS>(acc, a0, a1, g0p[X], g0p[HW + X], vp[X], max_flow);
        }
    }
    loss_block_reduce<kLossWaves>(acc, part + blockIdx.x);
}

template <bool METRICS>
__global__ __launch_bounds__(kLossThreads) void sequence_loss_kernel(const float *__restrict__ pred,
                                                                    const float *__restrict__ gt,
                                                                    const float *__restrict__ valid, size_t HW,
                                                                    size_t total, float max_flow,
                                                                    LossPartial *__restrict__ part) {
    const size_t base = (size_t)blockIdx.x * kSeqPerBlock + threadIdx.x;
    LossAcc acc;
#pragma unroll
    for (int q = 0; q < kSeqPerThread; ++q) {
        const size_t px = base + (size_t)q * kLossThreads;
        if (px < total) {
            const size_t n = px / HW, o = px + n * HW;  // n * 2 HW + (px - n HW)
            loss_term<METRICS>(acc, pred[o], pred[o + HW], gt[o], gt[o + HW], valid[px], max_flow);
        }
    }
    loss_block_reduce<kLossWaves>(acc, part + blockIdx.x);
}

// One wave: lane L sums the partials of its contiguous index range in index order, lane 0 then
// sums the 64 ranges in order.
__global__ __launch_bounds__(64) void loss_finalize_kernel(const LossPartial *__restrict__ part, int nparts,
                                                         double *__restrict__ out) {
    __shared__ LossPartial sh[64];
    const int lane = threadIdx.x, chunk = (nparts + 63) / 64;
    const int b = std::min(lane * chunk, nparts), e = std::min(b + chunk, nparts);
    LossPartial a = {0.0, 0.0, 0, 0, 0, 0};
    for (int q = b; q < e; ++q) {
        const LossPartial p = part[q];
        a.l1 += p.l1, a.epe += p.epe;
        a.n += p.n, a.c1 += p.c1, a.c3 += p.c3, a.c5 += p.c5;
    }
    sh[lane] = a;
    __syncthreads();
    if (lane == 0) {
        LossPartial t = {0.0, 0.0, 0, 0, 0, 0};
        for (int q = 0; q < 64; ++q) {
            t.l1 += sh[q].l1, t.epe += sh[q].epe;
            t.n += sh[q].n, t.c1 += sh[q].c1, t.c3 += sh[q].c3, t.c5 += sh[q].c5;
        }
        out[0] = t.l1, out[1] = (double)t.n, out[2] = t.epe;
        out[3] = (double)t.c1, out[4] = (double)t.c3, out[5] = (double)t.c5;
    }
}

// convex_upsample_bwd_kernel with G_c = scale v sign(a_c - g_c) formed in registers from the
// prediction it recomputes, instead of read from dout.  Sub-pixels the crop removes get dmask = 0
// and add nothing to S.
__global__ __launch_bounds__(kLossThreads) void upsample_loss_bwd_kernel(
    const float *__restrict__ flow, const float *__restrict__ mask, const float *__restrict__ gt,
    const float *__restrict__ valid, const float *__restrict__ scale_p, int h, int w, int H, int W, float max_flow,
    float *__restrict__ dmask, float *__restrict__ S) {
    __shared__ float red[kLossWaves][18][64];
    const int nxb = (w + 63) / 64;
    const int xb = blockIdx.x % nxb, y = (blockIdx.x / nxb) % h, n = blockIdx.x / (nxb * h);
    const int lane = threadIdx.x & 63, i = threadIdx.x >> 6;
    const int x = xb * 64 + lane;
    const bool ok = x < w;
    const int xc = ok ? x : w - 1;
    const int Y = 8 * y + i - (8 * h - H), X0 = 8 * xc - (8 * w - W);
    const size_t plane = (size_t)h * w, HW = (size_t)H * W;
    const float scale = *scale_p;
    const float *f0 = flow + (size_t)n * 2 * plane, *f1 = f0 + plane;
    float u0[9], u1[9];
    upsample_taps(f0, f1, y, xc, h, w, u0, u1);
    float s0[9], s1[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) s0[k] = s1[k] = 0.0f;
    if (ok) {
        const size_t grow = (size_t)n * 2 * HW + (size_t)(Y >= 0 ? Y : 0) * W;
        const size_t vrow = (size_t)n * HW + (size_t)(Y >= 0 ? Y : 0) * W;
        for (int j = 0; j < 8; ++j) {
            const size_t mo = ((size_t)n * 576 + 8 * i + j) * plane + (size_t)y * w + x;
            const int X = X0 + j;
            if (Y < 0 || X < 0) {
#pragma unroll
                for (int k = 0; k < 9; ++k) dmask[mo + (size_t)k * 64 * plane] = 0.0f;
                continue;
            }
            float lg[9], e[9], p[9], a0, a1;
#pragma unroll
            for (int k = 0; k < 9; ++k) lg[k] = mask[mo + (size_t)k * 64 * plane];
            const float sum = upsample_exp(lg, e);
            upsample_combine(e, sum, u0, u1, p, a0, a1);
            const float t0 = gt[grow + X], t1 = gt[grow + HW + X];
            const float sv = scale * loss_valid(valid[vrow + X], t0, t1, max_flow);
            const float g0 = sv * loss_sign(a0 - t0), g1 = sv * loss_sign(a1 - t1);
            float dv[9], pdv = 0.0f;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                dv[k] = g0 * u0[k] + g1 * u1[k];
                pdv += p[k] * dv[k];
            }
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                dmask[mo + (size_t)k * 64 * plane] = p[k] * (dv[k] - pdv);
                s0[k] += p[k] * g0;
                s1[k] += p[k] * g1;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        red[i][k][lane] = s0[k];
        red[i][9 + k][lane] = s1[k];
    }
    __syncthreads();
    // 18 planes x 64 lanes, summed over the 8 waves in order; wave t reduces planes t, t + 8, ...
    for (int q = i; q < 18; q += kLossWaves) {
        float a = 0.0f;
#pragma unroll
        for (int v = 0; v < kLossWaves; ++v) a += red[v][q][lane];
        const int c = q / 9, k = q - 9 * c;
        if (ok) S[(((size_t)n * 2 + c) * 9 + k) * plane + (size_t)y * w + x] = a;
    }
}

__global__ __launch_bounds__(256) void sequence_loss_bwd_kernel(const float *__restrict__ pred,
                                                               const float *__restrict__ gt,
                                                               const float *__restrict__ valid,
                                                               const float *__restrict__ scale_p, size_t HW,
                                                               size_t total, float max_flow,
                                                               float *__restrict__ dpred) {
    const float scale = *scale_p;
    for (size_t px = (size_t)blockIdx.x * blockDim.x + threadIdx.x; px < total;
         px += (size_t)gridDim.x * blockDim.x) {
        const size_t n = px / HW, o = px + n * HW;
        const float t0 = gt[o], t1 = gt[o + HW];
        const float sv = scale * loss_valid(valid[px], t0, t1, max_flow);
        dpred[o] = sv * loss_sign(pred[o] - t0);
        dpred[o + HW] = sv * loss_sign(pred[o + HW] - t1);
    }
}

hipError_t finalize(const LossPartial *part, size_t nparts, double *out, hipStream_t s) {
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(64), 0, s, part, (int)nparts, out);
    return hipGetLastError();
}

}  // namespace

// The grid sum alone, for a caller that has written the LossPartial words itself (corr_mask_loss.hip).
hipError_t launch_loss_finalize(const void *part, size_t nparts, double *out, hipStream_t s) {
    return finalize(static_cast<const LossPartial *>(part), nparts, out, s);
}

// The 18 S planes of the backward; the forward's per-workgroup partials (48 bytes for at most 64
// coarse pixels) fit in the same bytes.
size_t upsample_loss_workspace(int N, int h, int w) { return convex_upsample_bwd_workspace(N, h, w); }

size_t sequence_loss_workspace(int N, int H, int W) {
    return (((size_t)N * H * W + kSeqPerBlock - 1) / kSeqPerBlock) * sizeof(LossPartial);
}

hipError_t launch_upsample_loss(const float *flow, const float *mask, const float *gt, const float *valid, int N,
                                int h, int w, int H, int W, float max_flow, bool metrics, double *out, void *ws,
                                hipStream_t s) {
    static_assert(sizeof(LossPartial) <= 2 * 9 * sizeof(float), "the partials fit in the S planes");
    const size_t blocks = (size_t)N * h * ((w + 63) / 64);
    LossPartial *part = static_cast<LossPartial *>(ws);
    if (metrics)
        hipLaunchKernelGGL(upsample_loss_kernel<true>, dim3((unsigned)blocks), dim3(kLossThreads), 0, s, flow, mask, gt,
                           valid, h, w, H, W, max_flow, part);
    else
        hipLaunchKernelGGL(upsample_loss_kernel<false>, dim3((unsigned)blocks), dim3(kLossThreads), 0, s, flow, mask,
                           gt, valid, h, w, H, W, max_flow, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return finalize(part, blocks, out, s);
}

hipError_t launch_upsample_loss_bwd(const float *flow, const float *mask, const float *gt, const float *valid,
                                    const float *scale, int N, int h, int w, int H, int W, float max_flow,
                                    float *dflow, float *dmask, void *ws, hipStream_t s) {
    float *S = static_cast<float *>(ws);
    const unsigned blocks = (unsigned)((size_t)N * h * ((w + 63) / 64));
    hipLaunchKernelGGL(upsample_loss_bwd_kernel, dim3(blocks), dim3(kLossThreads), 0, s, flow, mask, gt, valid, scale,
                       h, w, H, W, max_flow, dmask, S);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_convex_upsample_bwd_flow(S, N, h, w, dflow, s);
}

hipError_t launch_sequence_loss(const float *pred, const float *gt, const float *valid, int N, int H, int W,
                                float max_flow, bool metrics, double *out, void *ws, hipStream_t s) {
    const size_t HW = (size_t)H * W, total = (size_t)N * HW;
    const size_t blocks = (total + kSeqPerBlock - 1) / kSeqPerBlock;
    LossPartial *part = static_cast<LossPartial *>(ws);
    if (metrics)
        hipLaunchKernelGGL(sequence_loss_kernel<true>, dim3((unsigned)blocks), dim3(kLossThreads), 0, s, pred, gt, valid,
                           HW, total, max_flow, part);
    else
        hipLaunchKernelGGL(sequence_loss_kernel<false>, dim3((unsigned)blocks), dim3(kLossThreads), 0, s, pred, gt,
                           valid, HW, total, max_flow, part);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return finalize(part, blocks, out, s);
}

hipError_t launch_sequence_loss_bwd(const float *pred, const float *gt, const float *valid, const float *scale, int N,
                                    int H, int W, float max_flow, float *dpred, hipStream_t s) {
    const size_t HW = (size_t)H * W, total = (size_t)N * HW;
    const int grid = (int)std::min<size_t>((total + 255) / 256, 65536);
    hipLaunchKernelGGL(sequence_loss_bwd_kernel, dim3(grid), dim3(256), 0, s, pred, gt, valid, scale, HW, total,
                       max_flow, dpred);
    return hipGetLastError();
}

}  // namespace corr
