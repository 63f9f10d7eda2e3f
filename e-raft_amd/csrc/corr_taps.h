// The lookup's tap arithmetic, shared by the lookups of the materialised pyramid
// (corr_lookup_block.h forward; corr_lookup_bwd.hip and corr_lookup_fold.hip backward) and
// corr_ondemand*.hip (lookups straight from the feature maps): one copy, so all round every tap
// coordinate, floor and corner weight identically.
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

// Both axes of one tap as one packed chain: component 0 = x, 1 = y, carried as float2 through
// tap_axis' operations in tap_axis' order (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: each
// component is one IEEE round-to-nearest operation, so the bits are tap_axis' bits); the
// infinite-quotient select of div_rn and floorf stay per component.
typedef float pk2 __attribute__((ext_vector_type(2)));

struct Axis2 {
    pk2 f, lo, hi;
    __device__ __forceinline__ Axis x() const { return Axis{f.x, lo.x, hi.x}; }
    __device__ __forceinline__ Axis y() const { return Axis{f.y, lo.y, hi.y}; }
};

// recip_rn (corr_div.h) of both components
__device__ __forceinline__ pk2 recip_rn2(pk2 d) {
    const pk2 y0 = {__builtin_amdgcn_rcpf(d.x), __builtin_amdgcn_rcpf(d.y)};
    return __builtin_elementwise_fma(__builtin_elementwise_fma(-d, y0, pk2{1.0f, 1.0f}), y0, y0);
}

// den = (size_x - 1, size_y - 1) as floats, rden = recip_rn2(den), hoisted by the callers (per level)
__device__ __forceinline__ Axis2 tap_axis2(float cx, float cy, float inv_scale, int t, int r, pk2 den, pk2 rden) {
    const pk2 cl = pk2{cx, cy} * inv_scale;
    const pk2 X = cl + (float)(t - r);
    const pk2 a = X * 2.0f;
    // div_rn (corr_div.h) on both components
    const pk2 q = a * rden;
    const pk2 qc = __builtin_elementwise_fma(__builtin_elementwise_fma(-q, den, a), rden, q);
    const pk2 d = {__builtin_isinf(q.x) ? q.x : qc.x, __builtin_isinf(q.y) ? q.y : qc.y};
    const pk2 xn = d - 1.0f;
    const pk2 ix = ((xn + 1.0f) * 0.5f) * den;
    Axis2 o;
    o.f = pk2{floorf(ix.x), floorf(ix.y)};
    o.hi = ix - o.f;
    o.lo = (o.f + 1.0f) - ix;
    return o;
}

__device__ __forceinline__ int anchor_of(float f) {
    return (f >= -1048576.0f && f <= 1048576.0f) ? (int)f : kFarAnchor;
}

__device__ __forceinline__ bool in_map(float xf, float yf, int Wl, int Hl) {
    return xf >= 0.0f && xf < (float)Wl && yf >= 0.0f && yf < (float)Hl;
}

// True when every in-map corner of the query's taps lies inside its (S+2)^2 neighbourhood.
template <int S>
__device__ __forceinline__ bool window_covers(float fx0, float fxl, float fy0, float fyl) {
    if (anchor_of(fx0) == kFarAnchor || anchor_of(fy0) == kFarAnchor) return true;
    return (fxl - fx0) <= (float)S && (fyl - fy0) <= (float)S;
}

}  // namespace corr
