// corr_lookup_block.h — the (2r+1)^2 bilinear window lookup of one block of queries at one
// pyramid level, shared by lookup_kernel (corr_lookup.hip) and the kernels that fuse the lookup
// with convc1 (corr_lookup_conv.hip: lookup_conv_kernel, lookup_conv_bwd_dw_kernel).
//
// Replaces CorrBlock.__call__ (model/corr.py:29-50) + bilinear_sampler (model/utils.py:7-21,
// F.grid_sample(align_corners=True), zero padding).
//
// Work layout: a block is QB (32; 16 on small maps) consecutive query pixels of one batch item
// at one pyramid level; thread (q, i) is query q's window column i (the x-tap; corr.py:37-43:
// the slow window index moves x).
//   1. thread (q, i): tap i of query q on both axes, rounded exactly as the reference does
//      (x/2^l + (i - r) -> 2X/(W_l-1) - 1 -> ((x'+1)/2)(W_l-1); one fp32 rounding per op),
//      its floor and the two 1-D weights; y-taps -> LDS, the thread keeps its x-tap;
//   2. every query's (S+2)^2 neighbourhood (anchored at the floor of its tap 0, zero outside
//      the map) is gathered from the TILED map (corr_common.h) into LDS, one 16-B tile row per
//      lane — all of a thread's loads issued before any LDS store, so the gather costs one
//      memory round trip;
//   3. thread (q, i) produces the S outputs (i, j = 0..S-1): 4 corner reads from LDS, fmaf in
//      the order nw, ne, sw, se (bit-identical to ATen's CPU grid_sampler_2d), handed to the
//      caller's emit().
// Tap floors are monotone in the tap index, so one check of the first and last tap proves
// that every corner lies inside the neighbourhood.  A workgroup where that fails for some
// query (only possible for |coordinates| near 2^20) takes a uniform slow path that reads such
// corners from global memory — keeping global loads out of the common loop (a load there
// makes every iteration wait on vmcnt, i.e. on the previous iteration's stores).
#pragma once

#include "corr_common.h"
#include "corr_div.h"
#include "corr_taps.h"

namespace corr {

typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int S, int QB>
struct LookupSmem {
    static constexpr int WIN = S + 2;
    static constexpr int NTC = (WIN + 6) / 4;  // tile columns that hold WIN cells at any offset
    // Window row of query q: cell cx (column anchor + cx) at win[q * WQ + cy * WW + 3 + cx].  A
    // gather lane stores its tile row's 4 cells at columns 4 tc - (anchor & 3) + 3 + c, i.e.
    // without predicates: cells left or right of the window land in the 3 + (4 NTC - WIN) spare
    // columns of the row.  Odd query stride: lane = query reads are conflict-free.
    static constexpr int WW = 4 * NTC + 3;
    static constexpr int WQ = (WIN * WW) | 1;
    float win[QB * WQ];
    float ty[3][S][QB];
    float fx[2][QB];  // floor of x-tap 0 and S-1
    int ax[QB], ay[QB];
    unsigned gw[QB];  // the gather's per-query words (gather_words), written by the tap-0 threads
    int go[QB];
    int flags;
};

// The gather's two words of a query anchored at (X0, Y0) (not far):
// word: bits 0..4 the chunk columns inside the map (and, TIGHT, touched by the taps), 5..7 the
// chunk column that holds the map's last cells (7: none), 8..24 the rows likewise, 26..27 y3,
// 28..29 a; qoff: the wave-uniform byte offset.  Fully outside queries: no bits but a.
template <int S, int QB, bool TIGHT>
__device__ __forceinline__ void gather_words(const LookupSmem<S, QB> &sm, int qq, int X0, int Y0, int TW, int TC,
                                             int Hl, unsigned &word, int &qoff) {
    constexpr int WIN = LookupSmem<S, QB>::WIN, NTC = LookupSmem<S, QB>::NTC;
    const int sX = X0 >> 2, a = X0 & 3, sY = Y0 >> 2, y3 = Y0 & 3;
    int xhi = TW - sX, yhi = Hl - Y0;
    if (TIGHT) {
        const float fx0 = sm.fx[0][qq], fxl = sm.fx[1][qq], fy0 = sm.ty[0][0][qq], fyl = sm.ty[0][S - 1][qq];
        if (window_covers<S>(fx0, fxl, fy0, fyl)) {  // chunk columns start at X0 & ~3
            xhi = min(xhi, ((int)(fxl - fx0) + 2 + a + 3) >> 2);
            yhi = min(yhi, (int)(fyl - fy0) + 2);
        } else {
            xhi = min(xhi, (WIN + a + 3) >> 2);
        }
    }
    const int xlo = min(max(-sX, 0), NTC), ylo = min(max(-Y0, 0), WIN);
    xhi = min(max(xhi, xlo), NTC), yhi = min(max(yhi, ylo), WIN);
    const unsigned cols = ((1u << (xhi - xlo)) - 1u) << xlo, rows = ((1u << (yhi - ylo)) - 1u) << ylo;
    const unsigned tl = (unsigned)(TW - 1 - sX) < (unsigned)NTC ? (unsigned)(TW - 1 - sX) : 7u;
    word = (unsigned)a << 28;
    if (cols != 0 && rows != 0) {
        word |= cols | (tl << 5) | (rows << 8) | ((unsigned)y3 << 26);
        qoff = (int)(64u * (unsigned)(sY * TC + sX) + 16u * (unsigned)y3);
    }
}

// Forward gather from the tiled maps (corr_common.h): one wave per query at a time, lane =
// (window row rr, tile column tc): one 16-B load of the tile row holding cells (anchor_y + rr,
// 4 (anchor_x / 4 + tc) .. + 3), zero outside the map; then four LDS stores realigned to the
// window (unconditional: out-of-window cells go to the row's spare columns).  All of a thread's
// loads are issued before any LDS store, so the gather costs one memory round trip.  What
// depends only on the lane is computed once per level, what depends only on the query once per
// workgroup (PRE) or per wave (all of its queries at once, lane k for query k), then readlane; per
// query and lane there remain two selects, a mask test, the buffer load and the LDS stores
// (profiles/r07_lookup_gather.md: 383 -> 309 VALU instructions per wave at DSEC;
// profiles/r09_lookup_issue.md for PRE).  TIGHT: only the rows / 16-B chunks the query's taps can
// touch (anchor .. floor(last tap) + 1 on each axis: floors are monotone in the tap index) are
// loaded — a regular window is 10 x 10 of the 11 x 11 neighbourhood; uncovered and far queries
// load all of it.  The cells not loaded are written as zeros and never read.  NOLOAD: ablation
// (tools/kbench_lookup.hip).  PRE: the per-query words were left in sm.gw / sm.go by the tap-0
// threads (lookup_block_v) and each wave only reads its queries' two.
template <int S, int QB, int NT, bool NOLOAD = false, bool TIGHT = false, bool PRE = false>
__device__ __forceinline__ void gather_window_tiled(LookupSmem<S, QB> &sm, const float *P, size_t qbase,
                                                    unsigned mapsz, int n0, int N, int Wl, int Hl, int tid) {
    using SM = LookupSmem<S, QB>;
    constexpr int WIN = SM::WIN, NTC = SM::NTC, WW = SM::WW, WQ = SM::WQ;
    constexpr int LPQ = NTC * WIN;           // lanes per query
    constexpr int EPL = (LPQ + 63) / 64;     // loads per lane and query
    constexpr int NW = NT / 64;
    constexpr int QPW = (QB + NW - 1) / NW;  // queries per wave
    static_assert(QPW <= 64, "one lane per query of the wave");
    static_assert(NTC <= 5 && WIN <= 17, "the packed lane predicate holds 5 chunk and 17 row bits");
    const int TW = map_tiles(Wl);   // 16-B chunks per map row
    const int TC = map_tcols(Wl);   // tiles per map row
    const int lane = tid & 63;
    const int wu = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned qb = __builtin_amdgcn_readfirstlane((unsigned)qbase);
    // ---- lane constants (per level, not per query) ----
    // The chunk of lane (rr, tc) of a query anchored at (X0, Y0) = (4 sX + a, 4 sY + y3) lies at
    // byte   64 (sY TC + sX) + 16 y3                        wave-uniform: added to the query's base
    //      + 64 tc + 16 rr + ((y3 + rr) >> 2) (64 TC - 64)    lane term: (y3 + rr) >> 2 is rr >> 2, plus
    // one when (rr & 3) + y3 carries, so it is one of two lane constants (offA, and offA + tile row
    // step).  pbit: the lane's chunk-column bit (0..4) and row bit (8..24) of the query's predicate
    // word; bit 31 (never set in a predicate word) for lanes beyond the window.
    const unsigned rstep = 64u * (unsigned)TC - 64u;
    unsigned offA[EPL], offB[EPL], pbit[EPL];
    int r3[EPL], tcl[EPL];
    float *lrow[EPL];
#pragma unroll
    for (int v = 0; v < EPL; ++v) {
        const int e = lane + 64 * v;
        const int rr = e / NTC, tc = e - rr * NTC;
        offA[v] = 64u * tc + 16u * rr + (unsigned)(rr >> 2) * rstep;
        offB[v] = offA[v] + rstep;
        asm volatile("" : "+v"(offB[v]));  // a register of its own: the choice below is one select, not select + add
        pbit[v] = e < LPQ ? (1u << tc) | (1u << (8 + rr)) : 0x80000000u;
        r3[v] = rr & 3;
        tcl[v] = tc;
        lrow[v] = &sm.win[wu * WQ + rr * WW + 4 * tc + 3];
    }
    // ---- per query, computed for all of the wave's queries at once: lane k = query wu + NW k ----
    // Far, dead and fully outside queries: no bits (gather_words).
    unsigned word = 0;
    int qoff = 0;
    {
        const int qq = wu + NW * lane;
        if (PRE) {
            if (lane < QPW && qq < QB) word = sm.gw[qq], qoff = sm.go[qq];
        } else if (lane < QPW && qq < QB && n0 + qq < N) {
            const int X0 = sm.ax[qq], Y0 = sm.ay[qq];
            if (X0 != kFarAnchor && Y0 != kFarAnchor) gather_words<S, QB, TIGHT>(sm, qq, X0, Y0, TW, TC, Hl, word, qoff);
        }
    }
    // ---- loads: all of a wave's queries before any LDS store ----
    // One buffer load per lane and query through a descriptor based at the query's map plus qoff
    // (scalar arithmetic): lanes outside the map or the window get an offset past the
    // descriptor's range and read 0.0f without a branch; map cells pass through untouched.
    const char *qmap = reinterpret_cast<const char *>(P) + (size_t)(qb + (unsigned)wu) * mapsz * 4;
    const size_t qstep = (size_t)NW * mapsz * 4;
    constexpr unsigned kPast = 0x80000000u;  // = the descriptor's range
    f32x4 vals[QPW][EPL];
    float *row[QPW][EPL];  // the LDS destination, realigned to the window: column 4 tc + 3 - a
#pragma unroll
    for (int k = 0; k < QPW; ++k) {
        const unsigned wk = (unsigned)__builtin_amdgcn_readlane((int)word, k);
        const int qk = __builtin_amdgcn_readlane(qoff, k);
        const int c3 = 4 - (int)((wk >> 26) & 3u);
        // (the realignment stays on the store side: one scalar-plus-lane add per query, and the
        // window rows keep the odd query stride that makes the lane = query reads conflict-free;
        // opaque, so the four stores share this one address and take immediate offsets)
        int shift = k * NW * WQ - (int)((wk >> 28) & 3u);
        asm volatile("" : "+s"(shift));
#pragma unroll
        for (int v = 0; v < EPL; ++v) {
            row[k][v] = lrow[v] + shift;
            if (NOLOAD) {
                vals[k][v] = f32x4{0.f, 0.f, 0.f, 0.f};
                continue;
            }
            const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
                const_cast<char *>(qmap + (size_t)k * qstep + (ptrdiff_t)qk), 0, (int)kPast, 0x00020000);
            const unsigned off = r3[v] >= c3 ? offB[v] : offA[v];
            const unsigned voff = (wk & pbit[v]) == pbit[v] ? off : kPast;
            vals[k][v] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs, (int)voff, 0, 0));
        }
    }
    // ---- LDS stores ----
    auto store_all = [&](auto rag) {
        constexpr bool RAGGED = decltype(rag)::value;
        const int wr = Wl & 3;
#pragma unroll
        for (int v = 0; v < EPL; ++v) {
            if (lane + 64 * v >= LPQ) continue;
#pragma unroll
            for (int k = 0; k < QPW; ++k) {
                if (wu + NW * k >= QB) continue;
                f32x4 x = vals[k][v];
                if (RAGGED) {  // the map's last chunk column holds cells past W_l: zero them
                    const unsigned wk = (unsigned)__builtin_amdgcn_readlane((int)word, k);
                    const bool last = tcl[v] == (int)((wk >> 5) & 7u);
#pragma unroll
                    for (int c = 1; c < 4; ++c) x[c] = (last && c >= wr) ? 0.0f : x[c];
                }
#pragma unroll
                for (int c = 0; c < 4; ++c) row[k][v][c] = x[c];
            }
        }
    };
    if ((Wl & 3) != 0) store_all(std::true_type{});
    else store_all(std::false_type{});
}

constexpr int lookup_threads(int S, int QB) { return (QB * S + 63) / 64 * 64; }

// ABL: diagnostic ablations for tools/kbench_lookup.hip only (0 in the library): bit 0 = no
// neighbourhood loads, bit 1 = no output stores, bit 2 = no coords load, bit 3 = plain (L2-cached)
// output stores instead of the non-temporal ones (lookup_kernel).
// One pyramid level of one block of QB queries (NT threads): the whole lookup of
// lookup_kernel (corr_lookup.hip).  emit(j, acc) receives output tap (i, j) of this thread's window column
// i = tid / QB for query q = tid % QB (called only for live queries).  Shared by lookup_kernel
// (global NCHW stores), lookup_conv_kernel (LDS tile feeding the fused 1x1 convolution) and
// lookup_conv_bwd_dw_kernel.  The lookup of one block with its coords already loaded (cxv, cyv:
// this thread's query; 0 for threads without one).
template <int S, int QB, int NT, int ABL, class Emit, bool TIGHT = false>
__device__ __forceinline__ void lookup_block_v(LookupSmem<S, QB> &sm, const float *__restrict__ P, float cxv,
                                               float cyv, int b, int n0, int N, int H, int W, int l, int tid,
                                               Emit emit) {
    constexpr int R = (S - 1) / 2;
    using SM = LookupSmem<S, QB>;
    constexpr int WIN = SM::WIN, WW = SM::WW, WQ = SM::WQ;
    const int Hl = H >> l, Wl = W >> l;
    const float inv_scale = __uint_as_float((unsigned)(127 - l) << 23);  // 2^-l, exactly (no division sequence)
    const unsigned mapsz = (unsigned)map_floats(Hl, Wl);
    const int TC = map_tcols(Wl);
    const size_t qbase = (size_t)b * N + n0;

    const int q = tid % QB;
    const int i = tid / QB;  // this thread's x-tap (window column); i >= S: gather only
    const bool act = i < S;
    const int n = n0 + q;
    const bool qok = act && n < N;

    // ---- 1. taps ----
    if (tid == 0) sm.flags = 0;
    // both axes as one packed chain (tap_axis2: tap_axis' bits)
    const pk2 den = {(float)(Wl - 1), (float)(Hl - 1)};
    const Axis2 t2 = tap_axis2(cxv, cyv, inv_scale, i, R, den, recip_rn2(den));
    const Axis tx = t2.x(), ty = t2.y();
    // The gather's per-query words: once per workgroup, by the tap-0 threads before the barrier.
    // TIGHT's extents need the last tap's floors, which other waves produce: its words are
    // computed per wave, after the barrier (gather_window_tiled).
    constexpr bool PRE = !TIGHT;
    if (act) {
        sm.ty[0][i][q] = ty.f;
        sm.ty[1][i][q] = ty.lo;
        sm.ty[2][i][q] = ty.hi;
        if (i == 0) {
            const int X0 = anchor_of(tx.f), Y0 = anchor_of(ty.f);
            sm.ax[q] = X0;
            sm.ay[q] = Y0;
            sm.fx[0][q] = tx.f;
            if constexpr (PRE) {  // the tap-0 threads hold all the gather's words need: once per workgroup
                unsigned word = 0;
                int qoff = 0;
                if (n < N && X0 != kFarAnchor && Y0 != kFarAnchor)
                    gather_words<S, QB, false>(sm, q, X0, Y0, map_tiles(Wl), TC, Hl, word, qoff);
                sm.gw[q] = word;
                sm.go[q] = qoff;
            }
        }
        if (i == S - 1) sm.fx[1][q] = tx.f;
    }
    __syncthreads();
    // Workgroup-uniform mode: bit 0 = some corner lies outside its neighbourhood (slow path),
    // bit 1 = some query's taps are not regular (floor(tap t) != floor(tap 0) + t).  Reduced per
    // wave by two ballots, so one LDS atomic per wave and not one pass of a loop per flagged lane
    // (on integer coordinates nearly every lane is flagged); set ahead of the gather's loads
    // (profiles/r09_lookup_issue.md for what else was tried).  A lambda on purpose: as a plain block
    // the compiler orders the kernel differently (one more SGPR; profiles/r10_lookup_split.md).
    auto set_flags = [&]() {
        int f = 0;
        if (act) {
            const int ax0 = sm.ax[q], ay0 = sm.ay[q];
            const bool far = ax0 == kFarAnchor || ay0 == kFarAnchor;
            const bool reg = far || (tx.f == (float)(ax0 + i) && ty.f == (float)(ay0 + i));
            f = reg ? 0 : 2;
            // covering is a property of the query: its tap-0 threads test it (one wave, not all)
            if (i == 0 && !window_covers<S>(sm.fx[0][q], sm.fx[1][q], sm.ty[0][0][q], sm.ty[0][S - 1][q])) f |= 1;
        }
        // every thread of the wave is here: the wave's flags, then one atomic
        const int wf = (__builtin_amdgcn_ballot_w64((f & 1) != 0) != 0 ? 1 : 0) |
                       (__builtin_amdgcn_ballot_w64((f & 2) != 0) != 0 ? 2 : 0);
        if (wf != 0 && (tid & 63) == 0) atomicOr(&sm.flags, wf);
    };
    set_flags();

    // ---- 2. neighbourhoods -> LDS ----
    gather_window_tiled<S, QB, NT, (ABL & 1) != 0, TIGHT, PRE>(sm, P, qbase, mapsz, n0, N, Wl, Hl, tid);
    __syncthreads();
    const int mode = sm.flags;
    if (!act) return;

    // ---- 3. outputs (i, 0..S-1) of query q ----
    const int ax = sm.ax[q], ay = sm.ay[q];
    const float *wq = &sm.win[q * WQ + 3];
    const float x0 = tx.f, ex = tx.lo, wx = tx.hi;
    if (mode == 0) {
        // regular taps: tap (i, j) has corners at neighbourhood column i, i+1 and rows j, j+1,
        // so the S+1 rows of the column pair are read once and shared by consecutive taps
        // (far queries read an all-zero neighbourhood: their taps have no in-map corner).
        const float *col = wq + i;
        float c0[S + 1], c1[S + 1];
#pragma unroll
        for (int j = 0; j <= S; ++j) {
            c0[j] = col[j * WW];
            c1[j] = col[j * WW + 1];
        }
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const float ey = sm.ty[1][j][q], ny = sm.ty[2][j][q];
            float acc = __fmul_rn(c0[j], __fmul_rn(ey, ex));
            acc = __builtin_fmaf(c1[j], __fmul_rn(ey, wx), acc);
            acc = __builtin_fmaf(c0[j + 1], __fmul_rn(ny, ex), acc);
            acc = __builtin_fmaf(c1[j + 1], __fmul_rn(ny, wx), acc);
            if (qok && (!(ABL & 2) || acc == 1234.5f)) emit(j, acc);
        }
    } else if (!(mode & 1)) {
        // every corner is inside the neighbourhood (cells outside the map hold 0)
        const bool far = (ax == kFarAnchor) || (ay == kFarAnchor);
        const int cx = far ? 0 : (int)x0 - ax;
        const float *col = wq + cx;
#pragma unroll
        for (int j = 0; j < S; ++j) {
            const float y0 = sm.ty[0][j][q], ey = sm.ty[1][j][q], ny = sm.ty[2][j][q];
            const int cy = far ? 0 : (int)y0 - ay;
            const float *c = col + cy * WW;
            float acc = __fmul_rn(c[0], __fmul_rn(ey, ex));
            acc = __builtin_fmaf(c[1], __fmul_rn(ey, wx), acc);
            acc = __builtin_fmaf(c[WW], __fmul_rn(ny, ex), acc);
            acc = __builtin_fmaf(c[WW + 1], __fmul_rn(ny, wx), acc);
            if (qok) emit(j, acc);
        }
    } else {
        const float *Pq = P + (qbase + q) * mapsz;
        auto fetch = [&](float xf, float yf) -> float {
            if (!in_map(xf, yf, Wl, Hl)) return 0.0f;
            const int xi = (int)xf, yi = (int)yf;
            const unsigned ux = (unsigned)(xi - ax), uy = (unsigned)(yi - ay);
            if (ux < (unsigned)WIN && uy < (unsigned)WIN) return wq[uy * WW + ux];
            return Pq[map_cell(yi, xi, TC)];
        };
        const float x1 = __fadd_rn(x0, 1.0f);
        for (int j = 0; j < S; ++j) {
            const float y0 = sm.ty[0][j][q], ey = sm.ty[1][j][q], ny = sm.ty[2][j][q];
            const float y1 = __fadd_rn(y0, 1.0f);
            float acc = __fmul_rn(fetch(x0, y0), __fmul_rn(ey, ex));
            acc = __builtin_fmaf(fetch(x1, y0), __fmul_rn(ey, wx), acc);
            acc = __builtin_fmaf(fetch(x0, y1), __fmul_rn(ny, ex), acc);
            acc = __builtin_fmaf(fetch(x1, y1), __fmul_rn(ny, wx), acc);
            if (qok) emit(j, acc);
        }
    }
}

template <int S, int QB, int NT, int ABL, bool TIGHT = false, class Emit>
__device__ __forceinline__ void lookup_block(LookupSmem<S, QB> &sm, const float *__restrict__ P,
                                             const float *__restrict__ coords, int b, int n0, int N,
                                             int H, int W, int l, int tid, Emit emit) {
    const int n = n0 + tid % QB;
    const bool qok = tid / QB < S && n < N;
    const float cxv = (ABL & 4) ? (float)(n % W) : qok ? coords[((size_t)b * 2 + 0) * N + n] : 0.0f;
    const float cyv = (ABL & 4) ? (float)(n / W) : qok ? coords[((size_t)b * 2 + 1) * N + n] : 0.0f;
    lookup_block_v<S, QB, NT, ABL, Emit, TIGHT>(sm, P, cxv, cyv, b, n0, N, H, W, l, tid, emit);
}

}  // namespace corr
