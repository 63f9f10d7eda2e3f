// The sequence loss's per-pixel arithmetic and its workgroup reduction (include/corr_mi355x_train.h
// has the definitions), shared by the kernels that form loss terms: corr_loss.hip (over a stored
// prediction or a stored mask) and corr_mask_loss.hip (over logits it recomputes).  A thread sums
// at most 16 terms in fp32; wave (xor butterfly) and workgroup (LDS, wave order) sums are fp64 in a
// fixed order and the counts are integers; one LossPartial per workgroup goes to the workspace,
// which launch_loss_finalize (corr_loss.hip) sums.  Internal, not part of the C-ABI.
#pragma once

#include <hip/hip_runtime.h>

namespace corr {

struct LossPartial {
    double l1, epe;
    unsigned long long n, c1, c3, c5;
};
static_assert(sizeof(LossPartial) == 48, "workspace layout");

struct LossAcc {
    float l1 = 0.0f, epe = 0.0f;
    unsigned n = 0, c1 = 0, c3 = 0, c5 = 0;
};

__device__ inline float loss_valid(float vld, float gx, float gy, float max_flow) {
    return (vld >= 0.5f && sqrtf(gx * gx + gy * gy) < max_flow) ? 1.0f : 0.0f;
}

__device__ inline float loss_sign(float d) { return (float)(d > 0.0f) - (float)(d < 0.0f); }

template <bool METRICS>
__device__ inline void loss_term(LossAcc &acc, float a0, float a1, float g0, float g1, float vld, float max_flow) {
    const float v = loss_valid(vld, g0, g1, max_flow);
    const float d0 = a0 - g0, d1 = a1 - g1;
    acc.l1 += v * fabsf(d0);
    acc.l1 += v * fabsf(d1);
    if (v != 0.0f) {
        acc.n += 1;
        if (METRICS) {
            const float epe = sqrtf(d0 * d0 + d1 * d1);
            acc.epe += epe;
            acc.c1 += epe < 1.0f;
            acc.c3 += epe < 3.0f;
            acc.c5 += epe < 5.0f;
        }
    }
}

// Every thread of the workgroup (WAVES waves) calls this (no early exit before it).
template <int WAVES>
__device__ inline void loss_block_reduce(const LossAcc &acc, LossPartial *dst) {
    __shared__ double rd[WAVES][2];
    __shared__ unsigned ri[WAVES][4];
    double l1 = acc.l1, epe = acc.epe;
    unsigned n = acc.n, c1 = acc.c1, c3 = acc.c3, c5 = acc.c5;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        l1 += __shfl_xor(l1, o);
        epe += __shfl_xor(epe, o);
        n += __shfl_xor(n, o);
        c1 += __shfl_xor(c1, o);
        c3 += __shfl_xor(c3, o);
        c5 += __shfl_xor(c5, o);
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) {
        rd[wv][0] = l1, rd[wv][1] = epe;
        ri[wv][0] = n, ri[wv][1] = c1, ri[wv][2] = c3, ri[wv][3] = c5;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        LossPartial p = {0.0, 0.0, 0, 0, 0, 0};
        for (int v = 0; v < WAVES; ++v) {
            p.l1 += rd[v][0], p.epe += rd[v][1];
            p.n += ri[v][0], p.c1 += ri[v][1], p.c3 += ri[v][2], p.c5 += ri[v][3];
        }
        *dst = p;
    }
}

}  // namespace corr
