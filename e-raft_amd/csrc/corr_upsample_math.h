// The convex upsampling's prediction arithmetic, op for op that of corr_upsample.hip's
// convex_upsample_kernel (logits in tap order; mx, expf(lg - mx), s; p = e / s; u = 8 flow with
// zeros outside; a += p u for k = 0..8), for the kernels that recompute a prediction instead of
// reading it (corr_loss.hip): a sub-pixel's prediction then carries the bits corr_convex_upsample
// writes.
#pragma once

#include <hip/hip_runtime.h>

namespace corr {

// u_kc = 8 flow[c][y + k / 3 - 1][x + k % 3 - 1], 0 outside the coarse map.
__device__ inline void upsample_taps(const float *__restrict__ f0, const float *__restrict__ f1, int y, int x, int h,
                                     int w, float (&u0)[9], float (&u1)[9]) {
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        const bool in = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const size_t o = in ? (size_t)yy * w + xx : 0;
        u0[k] = in ? 8.0f * f0[o] : 0.0f;
        u1[k] = in ? 8.0f * f1[o] : 0.0f;
    }
}

// e_k = expf(lg_k - max lg); returns their sum in tap order.
__device__ inline float upsample_exp(const float (&lg)[9], float (&e)[9]) {
    float mx = lg[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) mx = fmaxf(mx, lg[k]);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        e[k] = expf(lg[k] - mx);
        s += e[k];
    }
    return s;
}

// p_k = e_k / s and the prediction a_c = sum_k p_k u_kc, tap order.
__device__ inline void upsample_combine(const float (&e)[9], float s, const float (&u0)[9], const float (&u1)[9],
                                        float (&p)[9], float &a0, float &a1) {
    a0 = a1 = 0.0f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        p[k] = e[k] / s;
        a0 += p[k] * u0[k];
        a1 += p[k] * u1[k];
    }
}

}  // namespace corr
