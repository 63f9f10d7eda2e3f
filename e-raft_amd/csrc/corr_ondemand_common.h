// What the on-demand lookup (corr_ondemand.hip) and its backward (corr_ondemand_bwd.hip) share:
// the forward workspace's layout, the 16-B vector types and the in-wave LDS hand-over.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

#include "corr_common.h"

namespace corr {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kOdWaves = 4;               // waves per workgroup
constexpr int kOdQPW = 4;                 // queries per wave (in sequence)
constexpr int kOdQB = kOdWaves * kOdQPW;  // queries per workgroup
constexpr int kOdMaxS = 2 * CORR_MAX_RADIUS + 1;

inline int padded_d(int D) { return (D + 3) & ~3; }

struct OdLayout {
    size_t f1;                       // float offset of the fmap1 rows
    size_t p[CORR_MAX_LEVELS];       // float offset of pooled level l's rows
    size_t total;                    // floats in all
};

inline OdLayout ondemand_offsets(int B, int D, int H, int W, int levels) {
    OdLayout o{};
    const size_t Dp = (size_t)padded_d(D);
    size_t at = 0;
    o.f1 = at;
    at += (size_t)B * H * W * Dp;
    for (int l = 0; l < levels; ++l) {
        o.p[l] = at;
        at += (size_t)B * (H >> l) * (W >> l) * Dp;
    }
    o.total = at;
    return o;
}

// LDS hand-over between the lanes of one wave: a wave's DS operations execute in order, so
// only the compiler has to be kept from moving accesses across this point.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace corr
