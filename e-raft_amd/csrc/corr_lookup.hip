// corr_lookup.hip — the (2r+1)^2 bilinear window lookup of the materialised pyramid on gfx950,
// and the tiled pyramid's import / export.
//
// The lookup replaces CorrBlock.__call__ (model/corr.py:29-50) + bilinear_sampler
// (model/utils.py:7-21, F.grid_sample(align_corners=True), zero padding).  The ~12 ATen ops
// per level, the per-call CPU->GPU offset copies (corr.py:37-39), the cat and the
// permute().contiguous() (corr.py:49-50) become ONE launch that writes the NCHW output
// directly: a workgroup owns QB consecutive query pixels of one batch item at one pyramid level
// (corr_lookup_block.h: taps, window gather, bilinear taps) and stores output tap (i, j) to
// out[b][l*K + i*S + j][n] — consecutive n per wave, fully coalesced.
//
// The lookup fused with convc1 is in corr_lookup_conv.hip; the backward in corr_lookup_bwd.hip
// (per lookup, and the avg-pool backward) and corr_lookup_fold.hip (a build's lookups and the
// pool backward in one launch).
#include <algorithm>

#include "corr_common.h"
#include "corr_lookup_block.h"

namespace corr {
namespace {

template <int S, int QB, int ABL = 0, bool TIGHT = false>
__global__ __launch_bounds__(lookup_threads(S, QB)) void lookup_kernel(
    ConstLevelPtrs pyr, const float *__restrict__ coords, int B, int NQ, int H, int W, int L,
    float *__restrict__ out) {
    constexpr int K = S * S, NT = lookup_threads(S, QB);
    __shared__ LookupSmem<S, QB> sm;
    const int N = NQ;  // query pixels per batch item (H*W, or a row slab of it)
    const int nqb = (N + QB - 1) / QB;
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x / nqb);
    const int n0 = __builtin_amdgcn_readfirstlane((blockIdx.x - b * nqb) * QB);
    const int l = blockIdx.y;
    const int i = threadIdx.x / QB, n = n0 + threadIdx.x % QB;
    // (a scalar base per store plus a 32-bit thread offset saves ~20 VALU per wave here, but the
    // stores then measured slower: DSEC 5.22 -> 5.31 us, train 9.68 -> 9.84; a 32-bit thread offset
    // into the 64-bit pointer alone is a wash; profiles/r07_lookup_gather.md)
    float *o = out + (((size_t)b * L + l) * K + (size_t)i * S) * N + n;
    lookup_block<S, QB, NT, ABL, TIGHT>(sm, pyr.p[l], coords, b, n0, N, H, W, l, (int)threadIdx.x, [&](int j, float acc) {
        // non-temporal: the output streams past L2 (nothing in this kernel re-reads it), so the
        // kernel's end has no dirty lines of it to write back (DSEC 5.8 -> 5.4 us, train 12.2 ->
        // 11.4 us, same bits; profiles/r04q_kbench_lookup_nt.txt)
        if constexpr ((ABL & 8) != 0) o[(size_t)j * N] = acc;
        else __builtin_nontemporal_store(acc, &o[(size_t)j * N]);
    });
}

template <int S, int QB>
hipError_t launch_lookup_qb(const ConstLevelPtrs &pyr, const float *coords, int B, int NQ, int H, int W, int L,
                            float *out, hipStream_t s) {
    // TIGHT (only the window rows / 16-B chunks the query's taps touch) pays once the grid is
    // bandwidth-bound, >= 18,000 queries; below that its extents arithmetic sits on the latency
    // chain (same bits; profiles/r05m_kbench_lookup.txt: 1280x960 16.8 -> 16.1 us, B12 36x48
    // 15.9 -> 15.5, MVSEC 36x44 B16 18.6 -> 18.5; DSEC 5.6 -> 6.1, train B8 10.4 -> 10.6)
    const int nqb = (NQ + QB - 1) / QB;
    if ((long)B * NQ >= 18000)
        hipLaunchKernelGGL((lookup_kernel<S, QB, 0, true>), dim3(nqb * B, L), dim3(lookup_threads(S, QB)), 0, s,
                           pyr, coords, B, NQ, H, W, L, out);
    else
        hipLaunchKernelGGL((lookup_kernel<S, QB, 0, false>), dim3(nqb * B, L), dim3(lookup_threads(S, QB)), 0, s,
                           pyr, coords, B, NQ, H, W, L, out);
    return hipGetLastError();
}

template <int S>
hipError_t launch_lookup_s(const ConstLevelPtrs &pyr, const float *coords, int B, int NQ, int H,
                           int W, int L, float *out, hipStream_t s) {
    // queries per workgroup: 32; 16 for r = 4 on maps of <= 2048 cells with >= 20,000 queries in
    // all, where the smaller workgroups pack the CUs better over several rounds (same bits;
    // tools/kbench_lookup with the non-temporal output stores, profiles/r04t_kbench_lookup_qb2.txt:
    // QB 16 / 32 = MVSEC 36x44 B16 19.0 / 19.6 us, B12 36x48 16.1 / 16.1; train B8 12.0 / 11.7,
    // MVSEC crop 32x32 B16 12.3 / 11.3, DSEC 5.5 / 5.4, 1280x960 22.6 / 22.1; with the tiled
    // pyramid, profiles/r05m_kbench_lookup.txt: MVSEC 18.6 / 19.2, B12 15.9 / 15.7, train 10.3 / 10.2)
    if (S == 9 && H * W <= 2048 && (long)B * NQ >= 20000) return launch_lookup_qb<S, 16>(pyr, coords, B, NQ, H, W, L, out, s);
    return launch_lookup_qb<S, 32>(pyr, coords, B, NQ, H, W, L, out, s);
}

}  // namespace

hipError_t launch_lookup(const ConstLevelPtrs &pyr, const float *coords, int B, int NQ, int H,
                         int W, int levels, int radius, float *out, hipStream_t s) {
    return dispatch_radius(radius, [&](auto sc) {
        return launch_lookup_s<decltype(sc)::value>(pyr, coords, B, NQ, H, W, levels, out, s);
    });
}

// ---------------------------------------------------------------------------------------
// Tiled pyramid (corr_common.h) <-> the reference's row-major [BN][H_l][W_l]: EXPORT
// materialises corr_pyramid's view (corr.py:16,24,27,36 read it as [B*N, 1, H_l, W_l]); IMPORT
// installs a pyramid given in that layout (padding cells zeroed).  One thread per 16-B tile row.
// ---------------------------------------------------------------------------------------
namespace {
template <bool EXPORT>
__global__ __launch_bounds__(256) void pyramid_layout_kernel(const float *__restrict__ src, float *__restrict__ dst,
                                                             long BN, int Hl, int Wl) {
    const int TC = map_tcols(Wl);
    const long per = (long)map_floats(Hl, Wl) / 4;  // 16-B chunks per map
    const long total = BN * per;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long n = i / per;
        const int rem = (int)(i - n * per);
        const int t = rem / kTileW, cq = rem % kTileW;  // tile, chunk in the tile (kTileW / 4 per row)
        const int Y = 4 * (t / TC) + cq / (kTileW / 4), X = kTileW * (t % TC) + 4 * (cq % (kTileW / 4));
        const size_t row = ((size_t)n * Hl + Y) * Wl;
        if (EXPORT) {
            if (Y >= Hl) continue;
            const f32x4 v = reinterpret_cast<const f32x4 *>(src)[i];
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (X + c < Wl) dst[row + X + c] = v[c];
        } else {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if (Y < Hl && X + c < Wl) v[c] = src[row + X + c];
            reinterpret_cast<f32x4 *>(dst)[i] = v;
        }
    }
}

template <bool EXPORT>
hipError_t launch_pyramid_layout(const ConstLevelPtrs &src, long BN, int H, int W, int levels, const LevelPtrs &dst,
                                 hipStream_t s) {
    for (int l = 0; l < levels; ++l) {
        const int Hl = H >> l, Wl = W >> l;
        const long rows = BN * (long)(map_floats(Hl, Wl) / 4);
        const int grid = (int)std::min<long>((rows + 255) / 256, 8192);
        hipLaunchKernelGGL((pyramid_layout_kernel<EXPORT>), dim3(grid), dim3(256), 0, s, src.p[l], dst.p[l], BN, Hl,
                           Wl);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
}  // namespace

hipError_t launch_pyramid_export(const ConstLevelPtrs &pyr, long BN, int H, int W, int levels, const LevelPtrs &out,
                                 hipStream_t s) {
    return launch_pyramid_layout<true>(pyr, BN, H, W, levels, out, s);
}

hipError_t launch_pyramid_import(const ConstLevelPtrs &src, long BN, int H, int W, int levels, const LevelPtrs &pyr,
                                 hipStream_t s) {
    return launch_pyramid_layout<false>(src, BN, H, W, levels, pyr, s);
}

}  // namespace corr
