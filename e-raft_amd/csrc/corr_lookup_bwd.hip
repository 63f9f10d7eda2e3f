// corr_lookup_bwd.hip — the window lookup's input-gradient, one launch per lookup (or per
// chunk of a build's lookups), and the avg-pool backward, on gfx950.
//
// Backward (autograd of utils.py:15 w.r.t. the pyramid; coords are detached at
// eraft.py:128): with regular taps (floor of tap t = anchor + t on both axes — the common
// case) each neighbourhood cell receives exactly the <= 4 (tap, corner) contributions
//   se(cx-1, cy-1), ne(cx-1, cy), sw(cx, cy-1), nw(cx, cy)
// and is computed as a GATHER, summed in the reference's scatter order (taps row-major,
// corners nw, ne, sw, se), then added once to the gradient pyramid.  A query's cells belong
// to its own map only, so there are no atomics and results are deterministic.  Irregular
// workgroups fall back to a sequential per-query scatter in the same order.
#include <algorithm>
#include <type_traits>

#include "corr_common.h"
#include "corr_div.h"
#include "corr_lookup_bwd_common.h"
#include "corr_taps.h"

namespace corr {
namespace {

template <int S, int BQ>
struct LookupBwdSmem {
    static constexpr int WIN = S + 2;
    static constexpr int WSTR = (WIN * WIN) | 1;  // odd stride: lane = query writes conflict-free
    float g[S * S][BQ];   // upstream gradient tile
    float tx[3][S][BQ];   // floor, lo, hi per x-tap
    float ty[3][S][BQ];
    int ax[BQ], ay[BQ];
    float win[BQ * WSTR];  // per-query neighbourhood sums (cell (cy, cx) at cy * WIN + cx)
};

constexpr int lookup_bwd_threads(int S, int BQ) { return (BQ * (S + 2) + 63) / 64 * 64; }
constexpr int kBwdQB = 64;  // queries per workgroup (32: 4 workgroups per CU but 10% slower, measured)
// ... halved where 64 queries' S + 2 columns exceed a workgroup's 1024 threads (radius 7: 1088).
// The per-query sums do not depend on the workgroup's other queries, whichever form it takes.
constexpr int lookup_bwd_qb(int S) { return lookup_bwd_threads(S, kBwdQB) <= 1024 ? kBwdQB : kBwdQB / 2; }

// Backward, three phases (BQ queries; thread (q, t) = (tid % BQ, tid / BQ), t < S + 2):
//   1. thread (q, t < S): tap t of query q on both axes + the gradient row of x-tap t -> LDS;
//   2. q = query, t = neighbourhood COLUMN cx: every cell (cx, cy) of the column sums its
//      contributions in the reference's scatter order (x-tap i outer, y-tap j inner; one
//      corner per (i, j)) — reads conflict-free (query-fastest LDS rows), sums -> win;
//   3. lane = consecutive cells of one query: coalesced read-modify-write of the gradient
//      pyramid, G = G + sum (one RMW per cell, no atomics: the cells are the query's own).
// Regular workgroups (floor(tap t) = floor(tap 0) + t on both axes) use the closed form — cell
// (cx, cy) of the (S+1)^2 block gets se(cx-1, cy-1), ne(cx-1, cy), sw(cx, cy-1), nw(cx, cy) —
// with all of a column's taps in registers.  Other workgroups find each column's / row's taps
// as the contiguous ranges {i : floor_i - anchor in {c - 1, c}} (floors are monotone in the
// tap index), which reduces to the same four terms, in the same order, for regular taps.
// Workgroups where some corner falls outside the (S+2)^2 neighbourhood (|coords| near 2^20)
// take the sequential per-query scatter (wave 0, lane = query) of the previous design.
// T lookups' (coords, upstream gradient) pairs of one build, processed in order by one launch
// (corr_lookup_bwd_multi / corr_backward): zero = the workgroup first zeroes its queries' maps of
// its level, so the gradient pyramid needs no separate memset and every lookup's RMW hits cells
// this workgroup wrote moments before (L2-resident).  The single-lookup entry is T = 1, zero = 0.
template <int S, int BQ>
__global__ __launch_bounds__(lookup_bwd_threads(S, BQ)) void lookup_bwd_kernel(BwdLookups lk, int B, int NQ, int H,
                                                                           int W, int L, LevelPtrs gpyr) {
    constexpr int R = (S - 1) / 2, K = S * S, NT = lookup_bwd_threads(S, BQ);
    using SM = LookupBwdSmem<S, BQ>;
    constexpr int WIN = SM::WIN, WS = WIN * WIN, WSTR = SM::WSTR;
    constexpr int C = S + 1;  // cells per axis reached by regular taps
    __shared__ SM sm;

    const int N = NQ;  // query pixels per batch item (H*W, or a row slab of it)
    const int nqb = (N + BQ - 1) / BQ;
    const int b = blockIdx.x / nqb;
    const int n0 = (blockIdx.x - b * nqb) * BQ;
    const int l = blockIdx.y;
    const int Hl = H >> l, Wl = W >> l;
    const float inv_scale = 1.0f / (float)(1 << l);
    float *G = gpyr.p[l];
    const size_t mapsz = (size_t)Hl * Wl;
    const size_t qbase = (size_t)b * N + n0;

    const int tid = threadIdx.x;
    const int q = tid % BQ;
    const int t = tid / BQ;  // tap in phase 1, neighbourhood column in phase 2
    const int n = n0 + q;
    const bool qok = n < N;

    if (lk.zero) {  // this workgroup's query maps of level l (contiguous), before the first lookup
        const size_t cells = (size_t)min(BQ, N - n0) * mapsz;
        float *Z = G + qbase * mapsz;
        for (size_t i = tid; i < cells; i += NT) Z[i] = 0.0f;
        __syncthreads();
    }
    const float rdx = recip_rn((float)(Wl - 1)), rdy = recip_rn((float)(Hl - 1));
    for (int lt = 0; lt < lk.T; ++lt) {
    // constant-index selects (s_cselect): a dynamic index into the by-value table would copy it
    // to scratch
    const float *__restrict__ coords = lk.coords[0];
    const float *__restrict__ grad_out = lk.grad[0];
#pragma unroll
    for (int k = 1; k < kMaxLookups; ++k)
        if (k == lt) {
            coords = lk.coords[k];
            grad_out = lk.grad[k];
        }

    // ---- 1. taps and the upstream gradient tile ----
    Axis a{}, c{};
    if (t < S) {
        const float cxv = qok ? coords[((size_t)b * 2 + 0) * N + n] : 0.0f;
        const float cyv = qok ? coords[((size_t)b * 2 + 1) * N + n] : 0.0f;
        a = tap_axis(cxv, inv_scale, t, R, Wl, rdx);
        c = tap_axis(cyv, inv_scale, t, R, Hl, rdy);
        const float *g = grad_out + (((size_t)b * L + l) * K + (size_t)t * S) * N + n;
        float v[S];
#pragma unroll
        for (int u = 0; u < S; ++u) v[u] = qok ? g[(size_t)u * N] : 0.0f;
        sm.tx[0][t][q] = a.f;
        sm.tx[1][t][q] = a.lo;
        sm.tx[2][t][q] = a.hi;
        sm.ty[0][t][q] = c.f;
        sm.ty[1][t][q] = c.lo;
        sm.ty[2][t][q] = c.hi;
        if (t == 0) {
            sm.ax[q] = anchor_of(a.f);
            sm.ay[q] = anchor_of(c.f);
        }
#pragma unroll
        for (int u = 0; u < S; ++u) sm.g[t * S + u][q] = v[u];
    }
    __syncthreads();
    const float fx0 = sm.tx[0][0][q], fy0 = sm.ty[0][0][q];
    const bool far = anchor_of(fx0) == kFarAnchor || anchor_of(fy0) == kFarAnchor;
    const bool reg = t >= S || far || (a.f - fx0 == (float)t && c.f - fy0 == (float)t);
    const bool cov = t > 0 || window_covers<S>(fx0, sm.tx[0][S - 1][q], fy0, sm.ty[0][S - 1][q]);
    const int irregular = __syncthreads_or(!reg);
    const int uncovered = __syncthreads_or(!cov);

    if (!uncovered) {
        float *wq = &sm.win[q * WSTR];
        const int cx = t;
        if (!irregular) {
            // ---- 2a. closed form: column cx of the (S+1)^2 block ----
            if (cx < C && !far) {
                float wlo = 0.f, whi = 0.f;  // x weights: lo of tap cx, hi of tap cx - 1
                if (cx < S) wlo = sm.tx[1][cx][q];
                if (cx >= 1) whi = sm.tx[2][cx - 1][q];
                float ylo[S], yhi[S], gp[S], gc[S];
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    ylo[j] = sm.ty[1][j][q];
                    yhi[j] = sm.ty[2][j][q];
                    gp[j] = cx >= 1 ? sm.g[(cx - 1) * S + j][q] : 0.f;
                    gc[j] = cx < S ? sm.g[cx * S + j][q] : 0.f;
                }
#pragma unroll
                for (int cy = 0; cy < C; ++cy) {
                    float s = 0.0f;
                    if (cx >= 1 && cy >= 1) s = s + __fmul_rn(gp[cy - 1], __fmul_rn(yhi[cy - 1], whi));  // se
                    if (cx >= 1 && cy < S) s = s + __fmul_rn(gp[cy], __fmul_rn(ylo[cy], whi));           // ne
                    if (cx < S && cy >= 1) s = s + __fmul_rn(gc[cy - 1], __fmul_rn(yhi[cy - 1], wlo));   // sw
                    if (cx < S && cy < S) s = s + __fmul_rn(gc[cy], __fmul_rn(ylo[cy], wlo));            // nw
                    wq[cy * WIN + cx] = s;
                }
            }
        } else if (!far && cx < WIN) {
            // ---- 2b. general taps: contiguous hit ranges per column / row ----
            float dy[S];
#pragma unroll
            for (int j = 0; j < S; ++j) dy[j] = sm.ty[0][j][q] - fy0;
            int i0 = 0, i1 = 0;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const float d = sm.tx[0][i][q] - fx0;
                i0 += d < (float)(cx - 1);
                i1 += d <= (float)cx;
            }
#pragma unroll
            for (int cy = 0; cy < WIN; ++cy) {
                int j0 = 0, j1 = 0;
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    j0 += dy[j] < (float)(cy - 1);
                    j1 += dy[j] <= (float)cy;
                }
                float s = 0.0f;
                for (int i = i0; i < i1; ++i) {
                    const float wx = (sm.tx[0][i][q] - fx0 == (float)cx) ? sm.tx[1][i][q] : sm.tx[2][i][q];
                    for (int j = j0; j < j1; ++j) {
                        const float wy = (sm.ty[0][j][q] - fy0 == (float)cy) ? sm.ty[1][j][q] : sm.ty[2][j][q];
                        s = s + __fmul_rn(sm.g[i * S + j][q], __fmul_rn(wy, wx));
                    }
                }
                wq[cy * WIN + cx] = s;
            }
        }
        __syncthreads();
        // ---- 3. coalesced read-modify-write of the query's cells ----
        int tidv = tid;
        asm volatile("" : "+v"(tidv));  // opaque per lookup: keeps the cell-index math out of the
                                        // loop preheader (hoisted, it held ~120 VGPRs and spilled)
        auto rmw = [&](auto cc_tag) {
            constexpr int CC = decltype(cc_tag)::value;
            constexpr int CELLS = BQ * CC * CC;
            constexpr int PER = (CELLS + NT - 1) / NT;
            float sum[PER], old[PER];
            size_t dst[PER];
            bool live[PER];
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int item = tidv + NT * u;
                const int qq = item / (CC * CC);
                const int e = item - qq * (CC * CC);
                const int cy = e / CC, cx2 = e - cy * CC;
                const int X = sm.ax[qq] + cx2, Y = sm.ay[qq] + cy;
                live[u] = item < CELLS && n0 + qq < N && X >= 0 && X < Wl && Y >= 0 && Y < Hl;
                sum[u] = live[u] ? sm.win[qq * WSTR + cy * WIN + cx2] : 0.0f;
                dst[u] = live[u] ? (qbase + qq) * mapsz + (size_t)Y * Wl + X : 0;
                old[u] = live[u] ? G[dst[u]] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < PER; ++u)
                if (live[u]) G[dst[u]] = old[u] + sum[u];
        };
        if (!irregular)
            rmw(std::integral_constant<int, C>{});
        else
            rmw(std::integral_constant<int, WIN>{});
        __syncthreads();  // the next lookup reuses the LDS and re-reads these cells
        continue;
    }

    // ---- 2c. uncovered workgroup: sequential per-query scatter (wave 0, lane = query) ----
    for (int g = tid; g < BQ * WSTR; g += NT) sm.win[g] = 0.0f;
    __syncthreads();
    if (t == 0 && qok) {
        const int ax = sm.ax[q], ay = sm.ay[q];
        float *wq = &sm.win[q * WSTR];
        float *Gq = G + (qbase + q) * mapsz;
        auto scatter = [&](float xf, float yf, float v) {
            if (!in_map(xf, yf, Wl, Hl)) return;
            const int xi = (int)xf, yi = (int)yf;
            const unsigned ux = (unsigned)(xi - ax), uy = (unsigned)(yi - ay);
            if (ux < (unsigned)WIN && uy < (unsigned)WIN)
                wq[uy * WIN + ux] += v;
            else
                Gq[(size_t)yi * Wl + xi] += v;  // outside the neighbourhood: disjoint cells
        };
        for (int ii = 0; ii < S; ++ii) {
            const float x0 = sm.tx[0][ii][q], x1 = __fadd_rn(x0, 1.0f);
            const float ex = sm.tx[1][ii][q], wx = sm.tx[2][ii][q];
            for (int j = 0; j < S; ++j) {
                const float gv = sm.g[ii * S + j][q];
                const float y0 = sm.ty[0][j][q], y1 = __fadd_rn(y0, 1.0f);
                const float ey = sm.ty[1][j][q], ny = sm.ty[2][j][q];
                scatter(x0, y0, __fmul_rn(gv, __fmul_rn(ey, ex)));
                scatter(x1, y0, __fmul_rn(gv, __fmul_rn(ey, wx)));
                scatter(x0, y1, __fmul_rn(gv, __fmul_rn(ny, ex)));
                scatter(x1, y1, __fmul_rn(gv, __fmul_rn(ny, wx)));
            }
        }
    }
    __syncthreads();
    for (int g = tid; g < BQ * WS; g += NT) {
        const int qq = g / WS;
        const int e = g - qq * WS;
        if (n0 + qq >= N) continue;
        const int ry = e / WIN, rx = e - ry * WIN;
        const int Y = sm.ay[qq] + ry, X = sm.ax[qq] + rx;
        if (X >= 0 && X < Wl && Y >= 0 && Y < Hl) {
            float *d = G + (qbase + qq) * mapsz + (size_t)Y * Wl + X;
            *d = *d + sm.win[qq * WSTR + e];
        }
    }
    __syncthreads();
    }  // lookups
}

// avg_pool2d backward, one level: fine[q][y][x] += coarse[q][y/2][x/2] * 0.25 on the pooled
// region (y < 2*Hc, x < 2*Wc); floor-dropped rows / cols receive nothing.
// Idx: 32-bit cell index whenever the level fits (no 64-bit divisions).
template <typename Idx>
__global__ __launch_bounds__(256) void pool_bwd_kernel(const float *__restrict__ coarse,
                                                       float *__restrict__ fine, long BN, int Hf,
                                                       int Wf) {
    const int Hc = Hf >> 1, Wc = Wf >> 1;
    const int Hr = 2 * Hc, Wr = 2 * Wc;
    const Idx per = (Idx)Hr * Wr;
    const Idx total = (Idx)BN * per;
    for (Idx i = (Idx)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (Idx)gridDim.x * blockDim.x) {
        const size_t qq = i / per;
        const int rem = (int)(i - (Idx)qq * per);
        const int y = rem / Wr, x = rem - y * Wr;
        float *d = fine + qq * Hf * Wf + (size_t)y * Wf + x;
        *d = *d + coarse[qq * Hc * Wc + (size_t)(y >> 1) * Wc + (x >> 1)] * 0.25f;
    }
}

template <int S>
hipError_t launch_lookup_bwd_s(const BwdLookups &lk, int B, int NQ, int H, int W, int L, const LevelPtrs &gpyr,
                               hipStream_t s) {
    constexpr int QB = lookup_bwd_qb(S);
    static_assert(lookup_bwd_threads(S, QB) <= 1024, "a workgroup has at most 1024 threads");
    const int nqb = (NQ + QB - 1) / QB;
    hipLaunchKernelGGL((lookup_bwd_kernel<S, QB>), dim3(nqb * B, L), dim3(lookup_bwd_threads(S, QB)), 0, s, lk, B, NQ,
                       H, W, L, gpyr);
    return hipGetLastError();
}

hipError_t launch_lookup_bwd_lk(const BwdLookups &lk, int B, int NQ, int H, int W, int levels, int radius,
                                const LevelPtrs &gpyr, hipStream_t s) {
    return dispatch_radius(radius, [&](auto sc) {
        return launch_lookup_bwd_s<decltype(sc)::value>(lk, B, NQ, H, W, levels, gpyr, s);
    });
}

}  // namespace

hipError_t launch_lookup_bwd(const float *coords, const float *grad_out, int B, int NQ, int H,
                             int W, int levels, int radius, const LevelPtrs &gpyr, hipStream_t s) {
    BwdLookups lk{};
    lk.coords[0] = coords;
    lk.grad[0] = grad_out;
    lk.T = 1;
    lk.zero = 0;
    return launch_lookup_bwd_lk(lk, B, NQ, H, W, levels, radius, gpyr, s);
}

// T lookups in order into a gradient pyramid that this call OVERWRITES (zero-initialised by the
// kernel itself); more than kMaxLookups lookups go in chunks (the later chunks accumulate).
hipError_t launch_lookup_bwd_multi(const float *const *coords, const float *const *grad_out, int T, int B, int NQ,
                                   int H, int W, int levels, int radius, const LevelPtrs &gpyr, hipStream_t s) {
    for (int t0 = 0; t0 < T || t0 == 0; t0 += kMaxLookups) {
        BwdLookups lk{};
        lk.T = std::min(kMaxLookups, T - t0);
        lk.zero = t0 == 0;
        for (int k = 0; k < lk.T; ++k) {
            lk.coords[k] = coords[t0 + k];
            lk.grad[k] = grad_out[t0 + k];
        }
        hipError_t e = launch_lookup_bwd_lk(lk, B, NQ, H, W, levels, radius, gpyr, s);
        if (e != hipSuccess) return e;
        if (T == 0) break;
    }
    return hipSuccess;
}

hipError_t launch_pool_bwd(const LevelPtrs &gpyr, long BN, int H, int W, int levels,
                           hipStream_t s) {
    for (int l = levels - 1; l >= 1; --l) {
        const int Hf = H >> (l - 1), Wf = W >> (l - 1);
        const size_t total = (size_t)BN * (2 * (Hf >> 1)) * (2 * (Wf >> 1));
        if (total == 0) continue;
        const int grid = (int)((total + 255) / 256 < 32768 ? (total + 255) / 256 : 32768);
        if (total + (size_t)grid * 256 < (1ull << 32))
            hipLaunchKernelGGL(pool_bwd_kernel<unsigned>, dim3(grid), dim3(256), 0, s, gpyr.p[l], gpyr.p[l - 1],
                               BN, Hf, Wf);
        else
            hipLaunchKernelGGL(pool_bwd_kernel<size_t>, dim3(grid), dim3(256), 0, s, gpyr.p[l], gpyr.p[l - 1],
                               BN, Hf, Wf);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace corr
