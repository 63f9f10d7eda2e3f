// corr_ondemand_bwd.hip — the on-demand lookup's backward on gfx950: dfmap1 / dfmap2 of one
// corr_ondemand_prepare and its T lookups, without the all-pairs volume or its gradient.
//
// With P_0 = fmap2, P_l = avg_pool2d(P_{l-1}) and g_t the upstream gradient of lookup t:
//   Wg_t[b,n,l][cell] = sum over taps (i, j) and their corners landing on `cell` inside H_l x W_l
//                       of g_t[b, l K + i S + j, n] * (wy * wx)     (corr_taps.h: the forward's weights)
//   dF1[b,n,:]     = 1/sqrt(D) sum_t sum_l sum_cell Wg_t[b,n,l][cell] P_l[b,cell,:]
//   dP_l[b,cell,:] = 1/sqrt(D) sum_t sum_n Wg_t[b,n,l][cell] F1[b,n,:]
//   dF2 = dP_0 + poolT(dP_1 + poolT(dP_2 + ...)),  poolT: a coarse cell gives 0.25 of itself to each
//         of its four children; rows / columns dropped by the floor halving receive nothing.
// Everything works on the forward workspace's pixel-major rows ([cells][Dp], corr_ondemand_common.h)
// and accumulates into rows of the same shape in the backward workspace:
//   float dF1rows[B][N][Dp]; float dProws_l[B][H_l W_l][Dp] (l = 0 .. L-1);
//   float part_l[seg_l][B][H_l W_l][Dp] (l = 1 .. L-1);           (one lookup's; reused lookup after lookup)
//   int origin[B][L][N][2]; float block[B][L][N][(S+2)^2]        (likewise)
//
// Per lookup, in list order:
// 1. ondemand_bwd_window_kernel — a wave owns a query (all its levels, in order).  The K upstream
//    values are scattered into the query's own (S+2)^2 cell block anchored at the floor of tap 0,
//    each tap taking its floor from its own coordinate (floors are NOT assumed regular: on and near
//    the integer grid single floors move by one cell, see lookup_bwd_kernel in corr_lookup_bwd.hip).
//    Lane = cell: the cell sums its contributions x-tap outer, y-tap inner (at most one corner of a
//    tap lands on a given cell), i.e. the sequential scatter's order restricted to that cell.  The
//    block and its origin go to the workspace (origin = kFarAnchor: nothing here), and
//    dF1rows[b,n,:] += sum_cells Wg P_l[cell,:]: lanes hold the row's 16-B pieces, D walked in chunks
//    of 256, only cells some corner reached (inside the map) are loaded.  The wave is the row's only
//    writer: a plain read-modify-write (a store on the first lookup: the workspace arrives
//    uninitialised).
//
//    Which corners the block holds.  floor(tap t) - floor(tap 0) lies in [0, S] for every query
//    that has an in-map corner, so all corners lie in [anchor, anchor + S + 1]^2: the backward accepts
//    H, W <= 2^16 (ondemand_bwd_workspace_bytes returns 0 beyond), a corner inside the map has
//    |X| < 2^17 for its tap coordinate X = c / 2^l + (t - r), every tap of that query then has
//    |X| < 2^17 + 15, and tap_axis' five roundings (X, 2X / den, - 1, + 1, * den; * 0.5 is exact) put
//    the computed ix within 4 * 2^-24 * (2 |X| + den) + 2^-8 < 0.1 of X.  Two floors of taps S - 1
//    apart therefore differ by at most S.  A query whose floors spread farther (|c| ~ 2^20 and
//    beyond) or whose anchor is the far sentinel (NaN, +-inf, huge, one-cell levels) has no corner
//    inside any accepted map and contributes nothing — what CorrBlock's backward gives for it.
//
// 2. ondemand_bwd_dp_kernel — dP_l as a gather: a workgroup owns one batch item, one level, one
//    8 x 8 tile of target cells and (coarse levels) one segment of the query range.  It walks its
//    block origins in ascending query index, 1024 at a time; each thread tests four block rectangles
//    against the tile, ballot + prefix compact the hits into an LDS list that stays in ascending n.
//    The hits are consumed in that order, 16 at a time (the remainder is carried into the next
//    1024): Wg restricted to the tile
//    ([16][64 cells], zeros where the block misses the cell) and F1[n, chunk] ([16][256]) are staged
//    in LDS and acc[64 cells][256 features] += Wg^T F1 runs on v_mfma_f32_32x32x2_f32 (fp32
//    operands; 16 output tiles over 4 waves, 64 accumulator VGPRs per lane).  At the end
//    dProws_l[cell, chunk] += acc: the workgroup is the tile's only owner (with segments: it stores
//    to its own slab, and ondemand_bwd_segsum_kernel adds the slabs in segment order).  No cap and
//    no fallback: any coordinates only make the list longer.  D > 256 repeats the walk per
//    256-feature chunk.
//
// 3. once: poolT from the coarsest level down on the rows, then dF1rows and dProws_0 are divided
//    by sqrt(D) and transposed to [B, D, H, W] (channels D .. Dp-1 dropped).
//
// No float atomics, no allocation, no synchronisation; every launch goes on the given stream and
// the summation order is a function of the coordinates only, so reruns are bit-identical.
#include <algorithm>
#include <cmath>

#include "corr_common.h"
#include "corr_div.h"
#include "corr_ondemand_common.h"
#include "corr_taps.h"

namespace corr {
namespace {

constexpr int kObMaxWin = kOdMaxS + 2;                // cells per axis of a query's block
constexpr int kObMaxCells = kObMaxWin * kObMaxWin;    // 289
constexpr int kObRounds = (kObMaxCells + 63) / 64;    // lane = cell rounds
constexpr int kObMaxHW = 1 << 16;                     // see "which corners the block holds"

struct ObLayout {
    size_t df1;                  // float offsets
    size_t dp[CORR_MAX_LEVELS];
    size_t part[CORR_MAX_LEVELS];  // the dP gather's segment slabs (levels with more than one segment)
    size_t origin, block;
    size_t total;
};

inline int dp_segments(int l) { return l >= 3 ? 64 : 1 << (2 * l); }

inline ObLayout bwd_offsets(int B, int D, int H, int W, int levels, int radius) {
    ObLayout o{};
    const size_t Dp = (size_t)padded_d(D), N = (size_t)H * W, win = (size_t)(2 * radius + 3);
    size_t at = 0;
    o.df1 = at;
    at += (size_t)B * N * Dp;
    for (int l = 0; l < levels; ++l) {
        o.dp[l] = at;
        at += (size_t)B * (H >> l) * (W >> l) * Dp;
    }
    for (int l = 0; l < levels; ++l) {
        o.part[l] = at;
        if (dp_segments(l) > 1) at += (size_t)dp_segments(l) * B * (H >> l) * (W >> l) * Dp;
    }
    o.origin = at;
    at += (size_t)B * levels * N * 2;
    o.block = at;
    at += (size_t)B * levels * N * win * win;
    o.total = at;
    return o;
}

struct ObArgs {
    const f32x4 *F1;                  // fmap1 rows [B][N][D4]
    const f32x4 *P[CORR_MAX_LEVELS];  // pooled fmap2 rows
    const float *coords, *grad;       // this lookup's
    f32x4 *dF1;                       // accumulator rows, or null (that side is skipped)
    float *dP[CORR_MAX_LEVELS];       // accumulator rows (all null when dfmap2 is skipped)
    int *origin;                      // [B][L][N][2]
    float *block;                     // [B][L][N][WIN^2]
    float *part[CORR_MAX_LEVELS];     // the segments' slabs [seg_l][B][H_l W_l][Dp] (levels with seg_l > 1)
    int seg[CORR_MAX_LEVELS];         // query segments per level in the dP gather
    int maxwg;                        // its workgroups per batch item: max_l tiles_l * seg_l
    int B, N, H, W, L, D4, S;
    int first;                        // the first lookup initialises the accumulators
};

constexpr int kObQB = kOdWaves;  // queries per workgroup: one per wave (all its levels in sequence)
constexpr int kObFly = 8;        // reached cells per accumulation step (row loads in flight per lane)

struct ObSmem {
    float g[kOdMaxS * kOdMaxS][kObQB];   // the workgroup's upstream gradients of one level [channel][query]
    float cell[kOdWaves][kObMaxCells];   // a wave's query's block
    int row[kOdWaves][kObMaxCells];      // its cells' row numbers y W_l + x in the level (in-map cells)
    float tap[kOdWaves][6][kOdMaxS + 1]; // x: f, lo, hi; y: f, lo, hi
};

// Window gradients and dF1: grid B * ceil(N / 4), 4 waves, wave w owns query n0 + w.
__global__ __launch_bounds__(kOdWaves * 64) void ondemand_bwd_window_kernel(ObArgs a) {
    __shared__ ObSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.S, R = (S - 1) / 2, K = S * S, WIN = S + 2, NC = WIN * WIN, N = a.N, D4 = a.D4;
    const int nqb = (N + kObQB - 1) / kObQB;
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x / nqb);
    const int n0 = __builtin_amdgcn_readfirstlane((blockIdx.x - b * nqb) * kObQB);
    const int n = n0 + w;
    const bool live = n < N;  // wave-uniform
    float *cell = sm.cell[w];
    int *cellrow = sm.row[w];
    float(*tap)[kOdMaxS + 1] = sm.tap[w];
    const bool want2 = a.dP[0] != nullptr;
    float cxv = 0.f, cyv = 0.f;
    if (live) cxv = a.coords[((size_t)b * 2 + 0) * N + n], cyv = a.coords[((size_t)b * 2 + 1) * N + n];

#pragma unroll 1
    for (int l = 0; l < a.L; ++l) {
        const int Hl = a.H >> l, Wl = a.W >> l;
        const f32x4 *Pb = a.P[l] + (size_t)b * Hl * Wl * D4;
        const float inv_scale = 1.0f / (float)(1 << l);
        const float rdx = recip_rn((float)(Wl - 1)), rdy = recip_rn((float)(Hl - 1));
        __syncthreads();  // the previous level's tile has been consumed
        {
            const float *g = a.grad + ((size_t)b * a.L + l) * K * N + n0;
            for (int idx = tid; idx < K * kObQB; idx += kOdWaves * 64) {
                const int t = idx / kObQB, q = idx - t * kObQB;
                sm.g[t][q] = n0 + q < N ? g[(size_t)t * N + q] : 0.0f;
            }
        }
        __syncthreads();
        if (!live) continue;  // wave-uniform; the barriers above are reached every level
        // ---- taps ----
        if (lane < S) {
            const Axis tx = tap_axis(cxv, inv_scale, lane, R, Wl, rdx);
            const Axis ty = tap_axis(cyv, inv_scale, lane, R, Hl, rdy);
            tap[0][lane] = tx.f, tap[1][lane] = tx.lo, tap[2][lane] = tx.hi;
            tap[3][lane] = ty.f, tap[4][lane] = ty.lo, tap[5][lane] = ty.hi;
        }
        wave_sync();
        const float fx0 = tap[0][0], fy0 = tap[3][0];
        const int ax = anchor_of(fx0), ay = anchor_of(fy0);
        // nothing here: a far anchor, or floors spread wider than the block (no in-map corner)
        const bool skip = ax == kFarAnchor || ay == kFarAnchor || !(tap[0][S - 1] - fx0 <= (float)S) ||
                          !(tap[3][S - 1] - fy0 <= (float)S);  // wave-uniform
        const size_t oi = ((size_t)b * a.L + l) * N + n;
        if (want2 && lane == 0) {
            a.origin[2 * oi] = skip ? kFarAnchor : ax;
            a.origin[2 * oi + 1] = skip ? kFarAnchor : ay;
        }
        // ---- the block: lane = cell.  Column cx takes corner f of the taps with floor - anchor = cx
        // (weight lo) and corner f + 1 of those with floor - anchor = cx - 1 (weight hi); floors are
        // monotone in the tap index, so these taps are the range [i0, i1) (rows likewise): the sum
        // runs x-tap outer, y-tap inner, the sequential scatter's order restricted to this cell. ----
        unsigned long long reached[kObRounds];
#pragma unroll
        for (int k = 0; k < kObRounds; ++k) reached[k] = 0;
#pragma unroll 1
        for (int r = 0; !skip && r * 64 < NC; ++r) {  // wave-uniform
            const int c = r * 64 + lane;
            const int cy = c / WIN, cx = c - cy * WIN;
            float s = 0.0f;
            bool hit = false;
            if (c < NC && (unsigned)(ax + cx) < (unsigned)Wl && (unsigned)(ay + cy) < (unsigned)Hl) {
                cellrow[c] = (ay + cy) * Wl + (ax + cx);
                int i0 = 0, i1 = 0, j0 = 0, j1 = 0;
                for (int i = 0; i < S; ++i) {
                    const float dx = tap[0][i] - fx0, dy = tap[3][i] - fy0;
                    i0 += dx < (float)(cx - 1), i1 += dx <= (float)cx;
                    j0 += dy < (float)(cy - 1), j1 += dy <= (float)cy;
                }
                hit = i0 < i1 && j0 < j1;
                for (int i = i0; i < i1; ++i) {
                    const float wx = tap[0][i] - fx0 == (float)cx ? tap[1][i] : tap[2][i];
                    for (int j = j0; j < j1; ++j) {
                        const float wy = tap[3][j] - fy0 == (float)cy ? tap[4][j] : tap[5][j];
                        s = s + __fmul_rn(sm.g[i * S + j][w], __fmul_rn(wy, wx));
                    }
                }
            }
            const unsigned long long bal = __ballot(hit);
#pragma unroll
            for (int k = 0; k < kObRounds; ++k)  // constant-index selects: reached stays in SGPRs
                if (k == r) reached[k] = bal;
            if (c < NC) {
                cell[c] = s;
                if (want2) a.block[oi * NC + c] = s;
            }
        }
        wave_sync();
        // ---- dF1rows[b, n, :] += sum_cells Wg P_l[cell, :] ----
        const bool init = a.first && l == 0;
        if (a.dF1 && (!skip || init)) {
            f32x4 *row = a.dF1 + ((size_t)b * N + n) * D4;
            for (int d0 = 0; d0 < D4; d0 += 64) {
                const int p = d0 + lane;
                const bool pok = p < D4;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                if (pok && !init) acc = row[p];
#pragma unroll 1
                for (int r = 0; r < kObRounds; ++r) {
                    unsigned long long m = reached[0];  // constant-index selects: reached stays in SGPRs
#pragma unroll
                    for (int k = 1; k < kObRounds; ++k)
                        if (k == r) m = reached[k];
                    while (m) {  // wave-uniform: kObFly reached cells per step, their loads in flight together
                        float wv[kObFly];
                        f32x4 rv[kObFly];
#pragma unroll
                        for (int u = 0; u < kObFly; ++u) {
                            wv[u] = 0.0f;
                            rv[u] = f32x4{0.f, 0.f, 0.f, 0.f};
                            if (m) {
                                const int c = r * 64 + __builtin_ctzll(m);
                                m &= m - 1;
                                wv[u] = cell[c];
                                if (pok) rv[u] = Pb[(size_t)cellrow[c] * D4 + p];
                            }
                        }
#pragma unroll
                        for (int u = 0; u < kObFly; ++u)  // an absent cell adds 0 * 0
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[e] = __builtin_fmaf(wv[u], rv[u][e], acc[e]);
                    }
                }
                if (pok) row[p] = acc;
            }
        }
        wave_sync();  // the next level rewrites tap / cell
    }
}

// dP_l as a gather: grid (B * max_l(tiles_l * seg_l), L); workgroups past their level's count leave.
// Level l has 4^l times fewer tiles than level 0 and as many window blocks, so its query range is
// cut into seg_l = min(4^l, 64) equal segments, one workgroup per (tile, segment): every level
// then brings about as many workgroups of about as much work.  A level with seg_l = 1 adds its
// accumulators to dProws_l itself; the others store them to their segment's slab of `part` and
// ondemand_bwd_segsum_kernel adds the slabs to dProws_l in segment order (ascending n again).
constexpr int kDpBatch = 16;            // hits staged per MFMA pass (k = 16)
constexpr int kDpScanU = 4;             // origins tested per thread and step
constexpr int kDpScan = 256 * kDpScanU; // origins tested per step
constexpr int kDpList = kDpScan + kDpBatch;
constexpr int kDpFS = 256 + 4;          // staged F1 row stride (floats): rows k, k + 1 land 4 banks apart

struct DpSmem {
    int n[kDpList], ax[kDpList], ay[kDpList];  // the hit list, ascending n
    int wcnt[kDpScanU][4];
    float wg[kDpBatch][64];                    // Wg restricted to the tile, k-major
    alignas(16) float f1[kDpBatch][kDpFS];     // F1 rows' chunk, k-major (16-B staging stores)
};

__global__ __launch_bounds__(256, 2) void ondemand_bwd_dp_kernel(ObArgs a) {
    __shared__ DpSmem sm;
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int half = lane >> 5, l32 = lane & 31;
    const int l = blockIdx.y, Hl = a.H >> l, Wl = a.W >> l, N = a.N, D4 = a.D4;
    const int WIN = a.S + 2, NC = WIN * WIN;
    const int tw = (Wl + 7) >> 3, th = (Hl + 7) >> 3, ntile = tw * th, G = a.seg[l];
    const int b = __builtin_amdgcn_readfirstlane(blockIdx.x / a.maxwg);
    const int wg = blockIdx.x - b * a.maxwg;
    if (wg >= ntile * G) return;  // workgroup-uniform
    const int seg = wg / ntile, tile = wg - seg * ntile;
    const int per = (N + G - 1) / G, nlo = min(N, seg * per), nhi = min(N, nlo + per);
    const int y0 = (tile / tw) * 8, x0 = (tile - (tile / tw) * tw) * 8;
    const int *org = a.origin + ((size_t)b * a.L + l) * N * 2;
    const float *blk = a.block + ((size_t)b * a.L + l) * N * NC;
    const f32x4 *F1b = a.F1 + (size_t)b * N * D4;
    const size_t lvl = (size_t)Hl * Wl * D4 * 4;  // floats of one batch item's rows
    float *dst = G == 1 ? a.dP[l] + (size_t)b * lvl : a.part[l] + ((size_t)seg * a.B + b) * lvl;
    const bool store = G != 1 || a.first;  // a slab, or the first lookup: nothing to add to

    for (int d0 = 0; d0 < D4; d0 += 64) {
        const int nfeat = 4 * min(64, D4 - d0);  // live features of this chunk (a multiple of 4)
        f32x16 acc[2][2];
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[m][j][e] = 0.f;

        // hits [head, head + m) of the list: stage, then acc += Wg^T F1
        auto consume = [&](int head, int m) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = tid + 256 * u, k = idx >> 6, c = idx & 63;
                float v = 0.0f;
                if (k < m) {
                    const unsigned ux = (unsigned)(x0 + (c & 7) - sm.ax[head + k]);
                    const unsigned uy = (unsigned)(y0 + (c >> 3) - sm.ay[head + k]);
                    if (ux < (unsigned)WIN && uy < (unsigned)WIN) v = blk[(size_t)sm.n[head + k] * NC + uy * WIN + ux];
                }
                sm.wg[k][c] = v;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = tid + 256 * u, k = idx >> 6, p = idx & 63;
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (k < m && d0 + p < D4) v = F1b[(size_t)sm.n[head + k] * D4 + d0 + p];
                *(f32x4 *)&sm.f1[k][4 * p] = v;
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < kDpBatch / 2; ++kk) {
                const float a0 = sm.wg[2 * kk + half][l32], a1 = sm.wg[2 * kk + half][32 + l32];
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int f0 = 32 * (2 * w + j);
                    if (f0 < nfeat) {  // wave-uniform
                        const float bv = sm.f1[2 * kk + half][f0 + l32];
                        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0][j], 0, 0, 0);
                        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1][j], 0, 0, 0);
                    }
                }
            }
            __syncthreads();  // the next batch restages wg / f1
        };

        int cnt = 0;  // hits waiting in the list (workgroup-uniform, < kDpBatch between steps)
        for (int base = nlo; base < nhi; base += kDpScan) {
            // thread tid tests queries base + 256 u + tid: (u, wave, lane) order is ascending n
            int ox[kDpScanU], oy[kDpScanU];
            unsigned long long bal[kDpScanU];
#pragma unroll
            for (int u = 0; u < kDpScanU; ++u) {
                const int n = base + 256 * u + tid;
                ox[u] = oy[u] = kFarAnchor;
                if (n < nhi) ox[u] = org[2 * (size_t)n], oy[u] = org[2 * (size_t)n + 1];
            }
#pragma unroll
            for (int u = 0; u < kDpScanU; ++u) {
                const bool hit = ox[u] != kFarAnchor && ox[u] < x0 + 8 && ox[u] + WIN > x0 && oy[u] < y0 + 8 &&
                                 oy[u] + WIN > y0;
                bal[u] = __ballot(hit);
                if (lane == 0) sm.wcnt[u][w] = __builtin_popcountll(bal[u]);
            }
            __syncthreads();
            int off = cnt;
#pragma unroll
            for (int u = 0; u < kDpScanU; ++u) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int c = sm.wcnt[u][k];
                    if (k == w && ((bal[u] >> lane) & 1ull)) {
                        const int at = off + __builtin_popcountll(bal[u] & ((1ull << lane) - 1ull));
                        sm.n[at] = base + 256 * u + tid, sm.ax[at] = ox[u], sm.ay[at] = oy[u];
                    }
                    off += c;
                }
            }
            __syncthreads();
            cnt = off;
            // consume whole batches; after the last step also the partial one (zeros pad it)
            const bool last = base + kDpScan >= nhi;
            int head = 0;
            while (cnt - head >= kDpBatch || (last && cnt > head)) {
                const int m = min(kDpBatch, cnt - head);
                consume(head, m);
                head += m;
            }
            if (!last && head > 0) {  // carry the remainder (< 16 hits) to the front
                const int rem = cnt - head;
                int vn = 0, vx = 0, vy = 0;
                if (tid < rem) vn = sm.n[head + tid], vx = sm.ax[head + tid], vy = sm.ay[head + tid];
                __syncthreads();
                if (tid < rem) sm.n[tid] = vn, sm.ax[tid] = vx, sm.ay[tid] = vy;
                __syncthreads();
                cnt = rem;
            }
        }

        // ---- dst[cell, chunk] (+)= acc ----
        // acc[m][j][e]: cell 32 m + (e & 3) + 8 (e >> 2) + 4 half, feature 32 (2 w + j) + l32
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int f = 32 * (2 * w + j) + l32;
                if (f >= nfeat) continue;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int c = 32 * m + (e & 3) + 8 * (e >> 2) + 4 * half;
                    const int y = y0 + (c >> 3), x = x0 + (c & 7);
                    if (y < Hl && x < Wl) {
                        float *d = dst + ((size_t)y * Wl + x) * D4 * 4 + 4 * d0 + f;
                        *d = store ? acc[m][j][e] : *d + acc[m][j][e];
                    }
                }
            }
    }
}

// dProws_l (+)= sum over the segments' slabs, in segment order (a level with more than one segment).
__global__ __launch_bounds__(256) void ondemand_bwd_segsum_kernel(f32x4 *__restrict__ dP,
                                                                   const f32x4 *__restrict__ part, size_t total,
                                                                   int G, int first) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (!first) v = dP[idx];
    for (int g = 0; g < G; ++g) {
        const f32x4 p = part[(size_t)g * total + idx];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v[k] + p[k];
    }
    dP[idx] = v;
}

// poolT on the rows: fine[b][y][x][:] += 0.25 coarse[b][y >> 1][x >> 1][:] where the parent exists.
__global__ __launch_bounds__(256) void ondemand_bwd_unpool_kernel(f32x4 *__restrict__ fine,
                                                                   const f32x4 *__restrict__ coarse, int B, int Hf,
                                                                   int Wf, int D4) {
    const int Hc = Hf >> 1, Wc = Wf >> 1;
    const size_t total = (size_t)B * Hf * Wf * D4;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int c = (int)(idx % D4);
    const size_t cellf = idx / D4;
    const int x = (int)(cellf % Wf);
    const size_t r = cellf / Wf;
    const int y = (int)(r % Hf);
    const size_t b = r / Hf;
    if ((y >> 1) >= Hc || (x >> 1) >= Wc) return;  // dropped by the floor halving
    const f32x4 v = coarse[((b * Hc + (y >> 1)) * Wc + (x >> 1)) * D4 + c];
    f32x4 o = fine[idx];
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = o[k] + __fmul_rn(0.25f, v[k]);
    fine[idx] = o;
}

// rows [B][N][Dp] -> out [B][D][N], divided by sqrt(D): 32 x 32 tiles through LDS.
__global__ __launch_bounds__(256) void ondemand_bwd_finish_kernel(const float *__restrict__ rows,
                                                                   float *__restrict__ out, int D, int Dp, int N,
                                                                   float sqrtD) {
    __shared__ float t[32][33];
    const int ntn = (N + 31) / 32;
    const int b = blockIdx.x / ntn;
    const float *src = rows + (size_t)b * N * Dp;
    float *dst = out + (size_t)b * D * N;
    const int n0 = (blockIdx.x - b * ntn) * 32, d0 = blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int n = n0 + ty + 8 * k, d = d0 + tx;
        t[ty + 8 * k][tx] = (n < N && d < D) ? src[(size_t)n * Dp + d] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int d = d0 + ty + 8 * k, n = n0 + tx;
        if (d < D && n < N) dst[(size_t)d * N + n] = __fdiv_rn(t[tx][ty + 8 * k], sqrtD);
    }
}

}  // namespace

size_t ondemand_bwd_workspace_bytes(int B, int D, int H, int W, int levels, int radius) {
    if (H > kObMaxHW || W > kObMaxHW) return 0;
    return bwd_offsets(B, D, H, W, levels, radius).total * sizeof(float);
}

hipError_t launch_ondemand_backward(const void *fwd_ws, const float *const *coords, const float *const *grads, int T,
                                    int B, int D, int H, int W, int levels, int radius, void *bwd_ws, float *df1,
                                    float *df2, hipStream_t s) {
    const OdLayout fl = ondemand_offsets(B, D, H, W, levels);
    const ObLayout bl = bwd_offsets(B, D, H, W, levels, radius);
    const int Dp = padded_d(D), D4 = Dp / 4, N = H * W;
    const float *fbase = (const float *)fwd_ws;
    float *bbase = (float *)bwd_ws;
    ObArgs a{};
    a.F1 = (const f32x4 *)(fbase + fl.f1);
    for (int l = 0; l < levels; ++l) {
        a.P[l] = (const f32x4 *)(fbase + fl.p[l]);
        a.dP[l] = df2 ? bbase + bl.dp[l] : nullptr;
    }
    a.dF1 = df1 ? (f32x4 *)(bbase + bl.df1) : nullptr;
    a.origin = (int *)(bbase + bl.origin);
    a.block = bbase + bl.block;
    a.B = B, a.N = N, a.H = H, a.W = W, a.L = levels, a.D4 = D4, a.S = 2 * radius + 1;
    const unsigned nqb = (unsigned)((N + kObQB - 1) / kObQB);
    a.maxwg = 0;
    for (int l = 0; l < levels; ++l) {
        a.seg[l] = dp_segments(l);
        a.part[l] = bbase + bl.part[l];
        a.maxwg = std::max(a.maxwg, (((W >> l) + 7) / 8) * (((H >> l) + 7) / 8) * a.seg[l]);
    }
    for (int t = 0; t < T; ++t) {
        a.coords = coords[t], a.grad = grads[t], a.first = t == 0;
        hipLaunchKernelGGL(ondemand_bwd_window_kernel, dim3(nqb * (unsigned)B), dim3(kOdWaves * 64), 0, s, a);
        if (!df2) continue;
        hipLaunchKernelGGL(ondemand_bwd_dp_kernel, dim3((unsigned)a.maxwg * (unsigned)B, levels), dim3(256), 0, s, a);
        for (int l = 1; l < levels; ++l) {
            const size_t total = (size_t)B * (H >> l) * (W >> l) * D4;
            hipLaunchKernelGGL(ondemand_bwd_segsum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                               (f32x4 *)(bbase + bl.dp[l]), (const f32x4 *)(bbase + bl.part[l]), total, a.seg[l],
                               a.first);
        }
    }
    const float sqrtD = std::sqrt((float)D);
    const dim3 fgrid((unsigned)((N + 31) / 32) * (unsigned)B, (D + 31) / 32);
    if (df2) {
        for (int l = levels - 1; l >= 1; --l) {
            const int Hf = H >> (l - 1), Wf = W >> (l - 1);
            const size_t total = (size_t)B * Hf * Wf * D4;
            hipLaunchKernelGGL(ondemand_bwd_unpool_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                               (f32x4 *)(bbase + bl.dp[l - 1]), (const f32x4 *)(bbase + bl.dp[l]), B, Hf, Wf, D4);
        }
        hipLaunchKernelGGL(ondemand_bwd_finish_kernel, fgrid, dim3(256), 0, s, bbase + bl.dp[0], df2, D, Dp, N, sqrtD);
    }
    if (df1)
        hipLaunchKernelGGL(ondemand_bwd_finish_kernel, fgrid, dim3(256), 0, s, bbase + bl.df1, df1, D, Dp, N, sqrtD);
    return hipGetLastError();
}

}  // namespace corr
