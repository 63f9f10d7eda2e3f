// The lookup backward kernels' argument table, shared by corr_lookup_bwd.hip (lookup_bwd_kernel)
// and corr_lookup_fold.hip (lookup_bwd_fold_kernel).
#pragma once

namespace corr {

// T lookups' (coords, upstream gradient) pairs of one build, processed in order by one launch
// (corr_lookup_bwd_multi / corr_backward), passed by value.  zero: lookup_bwd_kernel first zeroes
// its queries' gradient maps (the fold keeps its maps in LDS and ignores it).
constexpr int kMaxLookups = 32;
struct BwdLookups {
    const float *coords[kMaxLookups];
    const float *grad[kMaxLookups];
    int T, zero;
};

}  // namespace corr
