// The lookup's tap arithmetic, shared by corr_lookup.hip (lookups of the materialised pyramid)
// and corr_ondemand.hip (lookups straight from the feature maps): one copy, so both round every
// tap coordinate, floor and corner weight identically.
#pragma once

#include <hip/hip_runtime.h>

#include "corr_div.h"

namespace corr {

// Sentinel anchor for NaN / huge coordinates: every window cell is outside the map.
constexpr int kFarAnchor = -(1 << 28);

struct Axis {
    float f;   // floor(ix) as float (may be NaN / huge)
    float lo;  // (f + 1) - ix  : weight of corner f
    float hi;  // ix - f        : weight of corner f + 1
};

// rden = recip_rn(size - 1), hoisted by the callers (per level)
__device__ __forceinline__ Axis tap_axis(float c, float inv_scale, int t, int r, int size, float rden) {
    // corr.py:41  centroid = coords / 2**l   (exact: power-of-two scale)
    // corr.py:43  + delta (integer offsets from linspace(-r, r, 2r+1))
    // utils.py:11 2*x/(W-1) - 1 ; grid_sample unnormalise ((x'+1)/2)*(W-1)
    // The division is correctly rounded (corr_div.h: the same bits as __fdiv_rn in 3 VALU)
    const float cl = c * inv_scale;
    const float X = cl + (float)(t - r);
    const float den = (float)(size - 1);
    const float xn = __fsub_rn(div_rn(2.0f * X, den, rden), 1.0f);
    const float ix = __fmul_rn(__fmul_rn(__fadd_rn(xn, 1.0f), 0.5f), den);
    Axis a;
    a.f = floorf(ix);
    a.hi = __fsub_rn(ix, a.f);
    a.lo = __fsub_rn(__fadd_rn(a.f, 1.0f), ix);
    return a;
}

__device__ __forceinline__ int anchor_of(float f) {
    return (f >= -1048576.0f && f <= 1048576.0f) ? (int)f : kFarAnchor;
}

__device__ __forceinline__ bool in_map(float xf, float yf, int Wl, int Hl) {
    return xf >= 0.0f && xf < (float)Wl && yf >= 0.0f && yf < (float)Hl;
}

}  // namespace corr
