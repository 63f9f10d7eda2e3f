// corr_lookup_fold.hip — the fused backward of one build's lookups on gfx950:
// lookup_bwd_fold_kernel and its launch.
#include <algorithm>
#include <atomic>
#include <type_traits>

#include "corr_build_common.h"
#include "corr_common.h"
#include "corr_div.h"
#include "corr_lookup_bwd_common.h"
#include "corr_taps.h"

namespace corr {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// ---------------------------------------------------------------------------------------------
// Fused backward of one build's T lookups + the avg-pool backward (corr_backward's fast path).
// A workgroup owns BQ query pixels and ALL (<= 4) levels of their gradient maps, resident in LDS
// for the whole launch: zeroed, then every lookup's window sums are added in lookup order (the
// same per-cell values as lookup_bwd_kernel: s = the cell's contributions of one lookup in the
// reference's scatter order, then M = M + s), then the maps are folded coarse-to-fine into
// level 0 (pool_fold_max_kernel's per-cell recurrence) and ONLY dC = level 0 is written, with
// its row maxima (written) and column maxima (atomicMax).  The coarse levels never reach HBM and
// no cell is read-modify-written in HBM: traffic = the upstream gradients + coords + dC.
// Wave w = level w; lane = (query q, neighbourhood column cx) with SLOTS = pow2 >= S + 2 lanes
// per query, so BQ = 64 / SLOTS queries (4 at r = 4).  A wave touches only its own level's maps
// and staging, so the lookup loop has NO workgroup barrier: each wave streams through the T
// lookups on its own (the next lookup's loads in flight), and the workgroup meets once, before
// the fold.  Per lookup: lanes cx < S compute tap cx of both axes; the closed form takes the
// group's other taps by DPP (row_newbcast for the y-taps and the anchors, row_shr for x-tap
// cx - 1 and its gradients), so a regular lookup touches LDS only for its cells.  Lane cx then
// produces its column's cells — closed form (regular taps), contiguous hit ranges (irregular;
// separable: the general separable form), or, when a corner leaves the (S+2)^2 neighbourhood,
// lookup_bwd_kernel's sequential scatter into a zeroed window scratch (the exact kernel reads
// every tap and gradient for these from the wave's LDS staging, written only when some group of
// the wave needs it; the separable kernel has no staging and shuffles them) — and adds them to
// the map (out-of-map cells: clamped into guard rows, or a per-lane dump slot).
constexpr int kFusedLv = 4;  // level slots (= waves) per workgroup

// median of three (v_med3_i32: clang does not form it from min / max with runtime bounds)
__device__ __forceinline__ int med3_i32(int x, int lo, int hi) {
    int r;
    asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "v"(hi));
    return r;
}

// A byte address past any workgroup's LDS allocation (<= 160 KiB) even after a map's worth of rows
// is subtracted: DS reads there return 0, DS writes are dropped.
constexpr int kLdsOob = 1 << 20;

constexpr int fused_slots(int S) { return S + 2 <= 4 ? 4 : S + 2 <= 8 ? 8 : S + 2 <= 16 ? 16 : 32; }

struct FusedOut {
    float *dc;              // [B * NQ][H * W]
    unsigned *rmax, *cmax;  // [B][NQ] (written), [B][H * W] (atomicMax; zeroed by the caller); may be null
    float *cpart;           // [B][groups][H * W]: per-workgroup column maxima instead of cmax atomics
    int B, NQ, H, W, L;
    int moff[kFusedLv], msz[kFusedLv];  // LDS float offset of level l's maps, cells per map
    int qstr[kFusedLv];                 // LDS floats between two queries' maps (bank-staggered)
    int aux;                            // LDS float offset of the per-wave staging
    int nfold;                          // fold workgroups; blocks past them compute rm
    int rm_rows_per_wave;
    FoldRowMax rm;
};

// Row |max| work of the blocks appended to the fold grid (rowmax2_kernel's per-row reduction:
// a wave walks each of its rows with 16-B loads, one cross-lane reduction per row).  They sit
// at the end of the grid, so they run in the fold's last, partly empty round of workgroups.
__device__ __forceinline__ void fold_rowmax_block(const FusedOut &o, int blk, int waves) {
    const FoldRowMax &a = o.rm;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int per_op = o.B * a.rows;  // rows of one operand, over the batch
    for (int k = 0; k < o.rm_rows_per_wave; ++k) {
        const int g = (blk * waves + wv) * o.rm_rows_per_wave + k;
        if (g >= 2 * per_op) return;  // whole waves
        const int t = g / per_op, br = g - t * per_op;
        const int cols = a.cols[t];
        const float *x = a.x[t] + (size_t)br * cols;
        float m = 0.f;
        if ((cols & 3) == 0 && ((uintptr_t)a.x[t] & 15) == 0) {
#pragma unroll 4
            for (int c = lane * 4; c < cols; c += 256) {
                const float4 q = *reinterpret_cast<const float4 *>(x + c);
                m = fmaxf(m, fmaxf(fmaxf(fabsf(q.x), fabsf(q.y)), fmaxf(fabsf(q.z), fabsf(q.w))));
            }
        } else {
#pragma unroll 4
            for (int c = lane; c < cols; c += 64) m = fmaxf(m, fabsf(x[c]));
        }
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) m = fmaxf(m, __shfl_xor(m, sh));
        if (lane == 0) a.out[t][br] = m > 0.f ? __float_as_uint(m) : 0u;
    }
}

// Per-wave staging (floats): taps TX/TY [3][S][BQ], gradients [K][BQ], anchors [2][BQ], dump
// slots [64].
template <int S>
struct FusedStage {
    static constexpr int SLOTS = fused_slots(S), BQ = 64 / SLOTS, K = S * S, WIN = S + 2;
    static constexpr int TX = 0, TY = TX + 3 * S * BQ, GG = TY + 3 * S * BQ, AX = GG + K * BQ, AY = AX + BQ,
                         DUMP = AY + BQ, SIZE = DUMP + 64;
};

// The separable fold with one DPP row per (query, level) group keeps no per-wave staging in LDS:
// its irregular windows take the general separable form and its rare windows (corners outside
// the neighbourhood, taps more than one cell off, non-finite gradients) the sequential scatter,
// which reads the group's taps and gradients by lane shuffles (ds_bpermute: no LDS allocated).
template <int S, bool SEP>
constexpr bool fold_no_staging() { return SEP && FusedStage<S>::SLOTS == 16; }

// Workgroups are dispatched round-robin over the 8 XCDs (each with its own L2).  Renumber them so
// every XCD gets a contiguous range: neighbouring query groups — which share the 128-B lines of
// the upstream gradients and coords — then read those lines through one L2 instead of eight.
// A bijection on [0, n) for any n.
__device__ __forceinline__ int xcd_contiguous(int bid, int n) {
    constexpr int kXcd = 8;
    const int q = n / kXcd, r = n % kXcd;
    const int x = bid % kXcd, k = bid / kXcd;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + k;
}

// x of the previous lane of a SLOTS-lane group, 0 for the group's first lane (cx = 0).  Groups of
// <= 16 lanes sit inside one DPP row: row_shr:1 (bound_ctrl: lane 0 of a row reads 0); larger
// groups use a bpermute.
template <int SLOTS>
__device__ __forceinline__ float lane_prev(float x, int cx) {
    if constexpr (SLOTS == 16) {  // the group is the DPP row: its lane 0 (cx = 0) reads the 0
        return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xF, 0xF, true));
    } else if constexpr (SLOTS < 16) {
        const int y = __builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xF, 0xF, true);
        return cx == 0 ? 0.f : __int_as_float(y);
    } else {
        const float y = __shfl_up(x, 1, 64);
        return cx == 0 ? 0.f : y;
    }
}

// Lane J of this lane's SLOTS-lane group.  Groups of 16 lanes are DPP rows: row_newbcast:J (one
// VALU move, no LDS); other group sizes use a bpermute.
template <int SLOTS, int J>
__device__ __forceinline__ float group_lane(float x, int lane) {
    if constexpr (SLOTS == 16) {  // every lane is written: no old value to initialise
        return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x150 + J, 0xF, 0xF, false));
    } else {
        return __shfl(x, (lane & ~(SLOTS - 1)) + J, 64);
    }
}

template <int SLOTS, int N, int J = 0>
__device__ __forceinline__ void group_lanes(float x, int lane, float (&out)[N]) {
    if constexpr (J < N) {
        out[J] = group_lane<SLOTS, J>(x, lane);
        group_lanes<SLOTS, N, J + 1>(x, lane, out);
    }
}

// Orders this wave's LDS traffic (LDS executes one wave's operations in issue order; the asm
// also keeps the compiler from moving LDS accesses across it).
__device__ __forceinline__ void wave_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// The lookup table (the kernel's FIRST argument) in VGPRs: lane i holds lookup i's two pointers,
// read once from the kernarg segment by a vector load; lookup t's are then two pairs of
// v_readlane.  Indexing the by-value copy with a runtime t makes the compiler either spill the
// table to scratch or emit a 32-way branch tree, and a scalar load per lookup would make every
// lookup wait for lgkmcnt(0) — i.e. also for the previous lookup's LDS writes — before its loads.
struct LaneTable {
    uint32_t c_lo, c_hi, g_lo, g_hi;
    __device__ __forceinline__ explicit LaneTable(int lane) {
        typedef const BwdLookups __attribute__((address_space(4))) *KPtr;
        const KPtr kp = (KPtr)__builtin_amdgcn_kernarg_segment_ptr();
        const int i = min(lane, kMaxLookups - 1);
        const uint64_t c = (uint64_t)kp->coords[i], g = (uint64_t)kp->grad[i];
        c_lo = (uint32_t)c, c_hi = (uint32_t)(c >> 32), g_lo = (uint32_t)g, g_hi = (uint32_t)(g >> 32);
    }
    __device__ __forceinline__ void get(int t, const float *&c, const float *&g) const {
        // (readlane returns int: widen through uint32_t, or a low word >= 2^31 sign-extends)
        c = reinterpret_cast<const float *>(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(c_hi, t) << 32) |
                                            (uint64_t)(uint32_t)__builtin_amdgcn_readlane(c_lo, t));
        g = reinterpret_cast<const float *>(((uint64_t)(uint32_t)__builtin_amdgcn_readlane(g_hi, t) << 32) |
                                            (uint64_t)(uint32_t)__builtin_amdgcn_readlane(g_lo, t));
    }
};

// PROBE (measurement builds only, tools/kbench_bwd.hip; the library uses 0): bit 0 = no lookup
// loop, bit 1 = no fold (no dC / maxima), bit 2 = no LDS zero-init (wrong results, timing only),
// bit 3 = plain (L2-cached) dC stores instead of the non-temporal ones, bit 4 = wait for the
// lookup's LDS writes at the end of each lookup (round 5's s_waitcnt).  (Moving the closed form's
// y-tap broadcasts, or its previous-column gradients, from DPP to ds_bpermute — LDS pipe
// instead of VALU — was measured and dropped: T = 12 79 -> 88 / 83 us,
// profiles/r06f_kbench_bwd_lean.txt; so was an L2 warm-up of lookup t + 3's gradient lines, one
// dword per row by the first workgroup of each 32-query line group: 145 -> 144 us with the
// gradients evicted before the launch, 79 -> 114 us warm, profiles/r06i_kbench_bwd_l2warm.txt.)
// SEP: regular windows by the separable closed form (corr_backward's default); false replays
// grid_sampler_2d_backward's per-tap products bit for bit (CORR_BACKWARD_EXACT_FOLD).
// (Several query groups per workgroup — 8 or 16 queries, so that the groups' waves would share
// L1 fills of the upstream-gradient lines — were measured and dropped: L2 requests unchanged,
// T = 12 92 -> 101 / 164 us, profiles/r05zi_kbench_bwd_groups_dropped.txt.)
// LEAN: the fold phase for the common case — 4 levels, no maxima (the bf16x6 backward),
// W % 4 == 0 and 16-B aligned dC — with the level values shared across a thread's 4 cells read
// once and no maxima arithmetic (the generic fold recomputed the coarse chain per cell and took
// |max| of every value: ~45 % of the fold phase's VALU).  The same per-cell sums in the same
// order (bit-identical).
template <int S, int PROBE = 0, bool SEP = false, bool LEAN = false>
__global__ __launch_bounds__(64 * kFusedLv) void lookup_bwd_fold_kernel(BwdLookups lk, FusedOut o) {
    using ST = FusedStage<S>;
    constexpr int R = (S - 1) / 2, K = S * S, C = S + 1, WIN = ST::WIN;
    constexpr int SLOTS = ST::SLOTS, BQ = ST::BQ, WQ = BQ, NT = 64 * kFusedLv;
    constexpr bool NOST = fold_no_staging<S, SEP>();
    extern __shared__ float fsm[];

    if ((int)blockIdx.x >= o.nfold) {  // appended row-maxima blocks (uniform per workgroup)
        fold_rowmax_block(o, (int)blockIdx.x - o.nfold, kFusedLv);
        return;
    }
    const int NQ = o.NQ, H = o.H, W = o.W, L = o.L, N = H * W;
    const int nqb = (NQ + WQ - 1) / WQ;
    const int blk = xcd_contiguous(blockIdx.x, o.nfold);
    const int b = blk / nqb, n0 = (blk - b * nqb) * WQ;
    const int tid = threadIdx.x, lane = tid & 63;
    const int l = tid >> 6;  // wave = level
    const int q = lane / SLOTS, cx = lane - q * SLOTS;
    const bool act = l < L;
    const int n = n0 + q;
    const bool qok = n < NQ;
    const int lc = act ? l : 0;
    const int Hl = H >> lc, Wl = W >> lc;
    const float inv_scale = 1.0f / (float)(1 << lc);
    const float rdx = recip_rn((float)(Wl - 1)), rdy = recip_rn((float)(Hl - 1));
    float *st = fsm + o.aux + lc * ST::SIZE;  // this wave's staging
    const int mbase = o.moff[lc] + q * o.qstr[lc];
    // fsm's LDS byte address (0 unless the kernel gains static LDS) and an LDS float at an
    // absolute byte address
    const int lds_base = (int)(uintptr_t)(__attribute__((address_space(3))) float *)fsm;
    auto lds_at = [](unsigned a) { return (__attribute__((address_space(3))) float *)(uintptr_t)a; };
    const int dump = o.aux + lc * ST::SIZE + ST::DUMP + lane;
    auto tx = [&](int c, int t) -> float & { return st[ST::TX + (c * S + t) * BQ + q]; };
    auto ty = [&](int c, int t) -> float & { return st[ST::TY + (c * S + t) * BQ + q]; };
    auto gg = [&](int k) -> float & { return st[ST::GG + k * BQ + q]; };
    unsigned *RM = reinterpret_cast<unsigned *>(fsm + o.aux + (NOST ? 0 : kFusedLv * ST::SIZE));  // [WQ]

    // the next lookup's coords and upstream gradients are loaded one lookup ahead (registers),
    // by buffer loads over batch item b's slice: every lane loads, and the lanes that own no
    // (tap, query) point past the slice, so the range check returns their zeros (no branch
    // around the loads, no select at use, 32-bit offsets).  The gradients are loaded in the
    // transposed lane order (lane 4 cx + q holds x-tap cx of query q), so the 4 lanes of a quad
    // read one 16-B run (the BQ queries' values of one row): one cache access per quad instead
    // of one per lane — the vector memory pipe (TA / TD ~85 % busy) bounded the lookup loop
    // (profiles/r05zg_fold_pmc.txt) — and one ds_bpermute per value restores lane order.
    const bool loader = act && cx < S && qok;
    const int cxl = min(cx, S - 1);
    constexpr uint32_t kOob = 0x80000000u;
    const uint32_t coff = loader ? (uint32_t)n * 4u : kOob;
    constexpr bool kQuadLoads = SLOTS == 16 && BQ == 4;
    const int lq = kQuadLoads ? ((lane & 3) ^ ((lane >> 5) << 1)) : q, lx = kQuadLoads ? (lane >> 2) : cx;
    const bool gloader = act && lx < S && n0 + lq < NQ;
    const uint32_t goff = gloader ? (uint32_t)(((lc * K + lx * S) * NQ + n0 + lq) * 4) : kOob;
    // ds_bpermute byte address of this lane's loader (lane 4 cx + (q ^ 2 [cx >= 8]))
    const int gsrc = kQuadLoads ? 4 * (4 * cx + (q ^ ((cx >> 3) << 1))) : 0;
    float pcx, pcy, pv[S];
    const LaneTable table(lane);
    auto prefetch = [&](int t) {
        const float *coords, *grad_out;
        table.get(t, coords, grad_out);
        const auto rc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(coords + (size_t)b * 2 * NQ), 0,
                                                          2 * NQ * 4, 0x00020000);
        const auto rg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(grad_out + (size_t)b * L * K * NQ), 0,
                                                          L * K * NQ * 4, 0x00020000);
        pcx = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rc, coff, 0, 0));
        pcy = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rc, coff, NQ * 4, 0));
#pragma unroll
        for (int u = 0; u < S; ++u)
            pv[u] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rg, goff, u * NQ * 4, 0));
    };
    if (act) prefetch(0);  // issued before the LDS zeroing, so its latency hides behind it
    if (!(PROBE & 4))
        // every map of the workgroup, 16 B per store (o.aux is a multiple of 4 floats)
        for (int i = 4 * tid; i < o.aux; i += 4 * NT) *reinterpret_cast<float4 *>(fsm + i) = make_float4(0.f, 0.f, 0.f, 0.f);
    if (tid < WQ) RM[tid] = 0u;
    __syncthreads();

    for (int t = 0; !(PROBE & 1) && act && t < lk.T; ++t) {  // absent levels (l >= L) only join the fold
        // ---- 1. tap cx of both axes; the group's taps reach the other lanes by DPP ----
        const float cxv = pcx, cyv = pcy;  // 0 for the lanes without a (tap, query)
        float v[S];
#pragma unroll
        for (int u = 0; u < S; ++u)
            v[u] = kQuadLoads ? __int_as_float(__builtin_amdgcn_ds_bpermute(gsrc, __float_as_int(pv[u]))) : pv[u];
        prefetch(min(t + 1, lk.T - 1));
        const Axis a = tap_axis(cxv, inv_scale, cxl, R, Wl, rdx);
        const Axis c = tap_axis(cyv, inv_scale, cxl, R, Hl, rdy);
        // ---- 2. the (query, level) group's form, decided per group ----
        const float fx0 = group_lane<SLOTS, 0>(a.f, lane), fy0 = group_lane<SLOTS, 0>(c.f, lane);
        const bool bad = cx < S && !(a.f - fx0 == (float)cx && c.f - fy0 == (float)cx);
        const unsigned long long gmask = (SLOTS == 64 ? ~0ull : ((1ull << SLOTS) - 1)) << (q * SLOTS);
        const bool irregular = (__ballot(bad) & gmask) != 0;
        const int ax = anchor_of(fx0), ay = anchor_of(fy0);
        const bool far = ax == kFarAnchor || ay == kFarAnchor;
        const bool unc = qok && !window_covers<S>(fx0, group_lane<SLOTS, S - 1>(a.f, lane), fy0,
                                                  group_lane<SLOTS, S - 1>(c.f, lane));
        // irregular groups take the range form (exact) — or, without staging (NOST), the general
        // separable form below, unless a tap's floor is more than one cell off its regular place
        // (only near |coordinates| ~ 2^20) or some upstream gradient of the wave is not finite
        // (that form multiplies every candidate tap, so a zero weight would turn an infinite
        // gradient into a NaN the reference does not have): those groups, like the groups whose
        // corners leave the neighbourhood, take the sequential scatter (seq)
        bool rangef = irregular, seq = unc;
        if constexpr (NOST) {
            rangef = false;
            if (__ballot(irregular)) {
                const bool odd = cx < S && !(fabsf(a.f - fx0 - (float)cx) <= 1.f && fabsf(c.f - fy0 - (float)cx) <= 1.f);
                bool nonfin = false;
#pragma unroll
                for (int u = 0; u < S; ++u) nonfin |= !__builtin_isfinite(v[u]);
                seq = unc || (irregular && qok && !far &&
                              (__ballot(nonfin) != 0 || (__ballot(odd && qok && !far) & gmask) != 0));
            }
        } else if (__ballot(rangef || unc)) {
            // the range form and the sequential scatter read any tap and any tap's gradients from
            // the wave's staging: written only when some group of the wave takes one of those paths
            if (cx < S) {
                tx(0, cx) = a.f, tx(1, cx) = a.lo, tx(2, cx) = a.hi;
                ty(0, cx) = c.f, ty(1, cx) = c.lo, ty(2, cx) = c.hi;
#pragma unroll
                for (int u = 0; u < S; ++u) gg(cx * S + u) = v[u];
            }
            wave_lds_sync();
        }
        const int X = ax + cx;
        const bool colok = qok && !seq && !far && cx < WIN && X >= 0 && X < Wl;
        // cell (cx, cy) of the window -> its map address, or the lane's dump slot when the cell
        // is outside the map / the column is not this lane's to write
        const int ayv = colok ? ay : -(1 << 30);
        const int rowbase = mbase + ay * Wl + X;
        auto cell_at = [&](int cy) { return (unsigned)(ayv + cy) < (unsigned)Hl ? rowbase + cy * Wl : dump; };
        // adds the column's NC cells sv[cy] (rows ay + cy) to the map.  Byte addresses: row ay + cy
        // clamped to [-1, Hl] — rows -1 and Hl of every map are guard rows (fused_lds_bytes), so
        // the window's cells above / below the map land in a guard row nothing reads — and a column
        // that is not this lane's to write starts past the workgroup's LDS allocation, where DS
        // reads return 0 and DS writes are dropped.  Clamping the ADDRESS of row ay + cy between
        // those of rows -1 and H_l is the same (addresses grow with the row), so a cell costs one
        // add and one v_med3.
        auto add_column = [&]<int NC>(const float (&sv)[NC]) {
            const bool mine = colok && cx < NC;
            // absolute LDS byte addresses (fsm's own offset folded into cb once: the accesses
            // then take the clamped address as is, no add per cell)
            const int cb = lds_base + (mine ? 4 * (mbase + X) : kLdsOob);
            const int s4 = 4 * Wl;
            const int gtop = cb - s4, gbot = cb + Hl * s4;
            // rows past [-NC, H_l] clamp like those bounds (and keep s4 * ay in range)
            int ra = cb + s4 * (mine ? min(max(ay, -NC), Hl) : 0);
            float old[NC];
            unsigned at[NC];
#pragma unroll
            for (int cy = 0; cy < NC; ++cy, ra += s4) at[cy] = (unsigned)med3_i32(ra, gtop, gbot);
#pragma unroll
            for (int cy = 0; cy < NC; ++cy) old[cy] = *lds_at(at[cy]);  // all reads, then all writes
#pragma unroll
            for (int cy = 0; cy < NC; ++cy) *lds_at(at[cy]) = old[cy] + sv[cy];
        };
        if (!irregular) {
            // closed form.  Absent terms (window edges) carry zero weights and gradients: adding
            // +-0 to a sum that started at +0 leaves it unchanged, so every cell sums its 4 terms
            // in the reference's order (se, ne, sw, nw) with the same bits.  Arrays are indexed
            // by y-tap j + 1 with zero sentinels at j = -1 and j = S, and two cells (cy, cy + 1)
            // go through each packed-fp32 instruction (v_pk_mul_f32 / v_pk_add_f32, IEEE per lane).
            // x-tap cx is this lane's own, x-tap cx - 1 the previous lane's; y-tap j is lane j's.
            const float wlo = cx < S ? a.lo : 0.f;
            const float hprev = lane_prev<SLOTS>(a.hi, cx);
            const float whi = cx >= 1 && cx <= S ? hprev : 0.f;
            float ylo_[S], yhi_[S];
            group_lanes<SLOTS, S>(c.lo, lane, ylo_);
            group_lanes<SLOTS, S>(c.hi, lane, yhi_);
            auto yv = [&](int cc, int j) { return j >= 0 && j < S ? (cc == 1 ? ylo_[j] : yhi_[j]) : 0.f; };
            // the gradients of x-tap cx are this lane's own loads (v: zero for cx >= S and for
            // absent queries), those of x-tap cx - 1 the previous lane's (lane_prev: zero at cx = 0)
            float gpr[S];
#pragma unroll
            for (int j = 0; j < S; ++j) gpr[j] = lane_prev<SLOTS>(v[j], cx);
            auto gpv = [&](int j) { return j >= 0 && j < S ? gpr[j] : 0.f; };
            auto gcv = [&](int j) { return j >= 0 && j < S ? v[j] : 0.f; };
            const f32x2 WH = f32x2{whi, whi}, WL = f32x2{wlo, wlo};
            float sv[C + 1];
            if constexpr (SEP) {
                // separable (the default): the column's two x-taps first, hx[j] = g(cx - 1, j) whi +
                // g(cx, j) wlo for each y-tap j, then the y-taps, cell cy = hx[cy - 1] yhi[cy - 1] +
                // hx[cy] ylo[cy] — the same four (tap, corner) terms with the same per-tap weights,
                // rounded in another order (~1e-7 relative; tests/test_gpu_parity.py), for ~30
                // instead of ~70 VALU per lane
                float hx[S];
#pragma unroll
                for (int j = 0; j + 1 < S; j += 2) {
                    const f32x2 h = __builtin_elementwise_fma(f32x2{v[j], v[j + 1]}, WL, f32x2{gpr[j], gpr[j + 1]} * WH);
                    hx[j] = h.x, hx[j + 1] = h.y;
                }
                if constexpr ((S & 1) != 0) hx[S - 1] = __builtin_fmaf(v[S - 1], wlo, gpr[S - 1] * whi);
#pragma unroll
                for (int cy = 0; cy < C; ++cy) {
                    const float up = cy >= 1 ? hx[cy - 1] * yhi_[cy - 1] : 0.f;
                    sv[cy] = cy < S ? __builtin_fmaf(hx[cy], ylo_[cy], up) : up;
                }
            } else
#pragma unroll
            for (int cy = 0; cy < C; cy += 2) {  // cells cy, cy + 1; se / sw use y-tap cy - 1, ne / nw cy
                const f32x2 yhi = f32x2{yv(2, cy - 1), yv(2, cy)}, ylo = f32x2{yv(1, cy), yv(1, cy + 1)};
                const f32x2 gpm = f32x2{gpv(cy - 1), gpv(cy)}, gp0 = f32x2{gpv(cy), gpv(cy + 1)};
                const f32x2 gcm = f32x2{gcv(cy - 1), gcv(cy)}, gc0 = f32x2{gcv(cy), gcv(cy + 1)};
                // se first.  The reference's cell starts at +0 (0 + se): starting at se differs
                // only when every term is -0, giving -0 instead of +0 — and the map value it is
                // added to is never -0 (it starts at +0 and no round-to-nearest sum of it is -0),
                // so old + sv is the same bits either way.
                f32x2 acc = gpm * (yhi * WH);
                acc = acc + gp0 * (ylo * WH);                    // ne
                acc = acc + gcm * (yhi * WL);                    // sw
                acc = acc + gc0 * (ylo * WL);                    // nw
                sv[cy] = acc.x;
                sv[cy + 1] = acc.y;
            }
            add_column(reinterpret_cast<const float (&)[C]>(sv));
        } else if (!rangef) {
            if constexpr (SEP && SLOTS == 16) {
                // general separable form (irregular windows: taps of a query whose floors are not all
                // anchor + t, e.g. the cold-start integer grid, where rounding leaves some taps a hair
                // below their integer).  Tap t's floor is anchor + t + e_t with e_t in {-1, 0, 1}, so it
                // reaches cells t - 1 .. t + 2 of the neighbourhood: slot k in {-1, 0, 1, 2} weighs
                // lo at k = e_t, hi at k = e_t + 1, 0 elsewhere.  Column cx gathers x-taps cx, cx - 1,
                // cx - 2, cx + 1 (DPP row shifts: the 16-lane group is the DPP row, lanes outside it
                // read 0), then row cy gathers y-taps cy, cy - 1, cy - 2, cy + 1 (broadcast weights).
                // Non-reached slots multiply a finite gradient by 0 (seq takes the waves with non-finite ones).
                const bool tv = cx < S;
                auto slots = [&](float e, float lo, float hi, float &wm1, float &w0, float &w1, float &w2) {
                    const bool m = e == -1.f, z = e == 0.f, p = e == 1.f;  // e = 2: no tap
                    wm1 = m ? lo : 0.f;
                    w0 = m ? hi : (z ? lo : 0.f);
                    w1 = z ? hi : (p ? lo : 0.f);
                    w2 = p ? hi : 0.f;
                };
                float xm1, x0, x1, x2, ym1, y0, y1, y2;
                slots(tv ? a.f - fx0 - (float)cx : 2.f, a.lo, a.hi, xm1, x0, x1, x2);
                slots(tv ? c.f - fy0 - (float)cx : 2.f, c.lo, c.hi, ym1, y0, y1, y2);
                auto shr1 = [](float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x111, 0xF, 0xF, true)); };
                auto shr2 = [](float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x112, 0xF, 0xF, true)); };
                auto shl1 = [](float x) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), 0x101, 0xF, 0xF, true)); };
                const float wp1 = shr1(x1), wp2 = shr2(x2), wn1 = shl1(xm1);
                float hx[S];
#pragma unroll
                for (int j = 0; j < S; ++j)
                    hx[j] = __builtin_fmaf(v[j], x0, __builtin_fmaf(shr1(v[j]), wp1, __builtin_fmaf(shr2(v[j]), wp2, shl1(v[j]) * wn1)));
                float Ym1[S], Y0[S], Y1[S], Y2[S];
                group_lanes<SLOTS, S>(ym1, lane, Ym1);
                group_lanes<SLOTS, S>(y0, lane, Y0);
                group_lanes<SLOTS, S>(y1, lane, Y1);
                group_lanes<SLOTS, S>(y2, lane, Y2);
                float sv[WIN];
#pragma unroll
                for (int cy = 0; cy < WIN; ++cy) {
                    float acc = cy < S ? hx[cy] * Y0[cy] : 0.f;
                    if (cy >= 1 && cy - 1 < S) acc = __builtin_fmaf(hx[cy - 1], Y1[cy - 1], acc);
                    if (cy >= 2 && cy - 2 < S) acc = __builtin_fmaf(hx[cy - 2], Y2[cy - 2], acc);
                    if (cy + 1 < S) acc = __builtin_fmaf(hx[cy + 1], Ym1[cy + 1], acc);
                    sv[cy] = acc;
                }
                add_column(sv);
            }
        } else if constexpr (!NOST) {
            float dy[S];
#pragma unroll
            for (int j = 0; j < S; ++j) dy[j] = ty(0, j) - fy0;
            int i0 = 0, i1 = 0;
#pragma unroll
            for (int i = 0; i < S; ++i) {
                const float d = tx(0, i) - fx0;
                i0 += d < (float)(cx - 1);
                i1 += d <= (float)cx;
            }
            for (int cy = 0; cy < WIN; ++cy) {
                int j0 = 0, j1 = 0;
#pragma unroll
                for (int j = 0; j < S; ++j) {
                    j0 += dy[j] < (float)(cy - 1);
                    j1 += dy[j] <= (float)cy;
                }
                float sv = 0.0f;
                if (colok)
                    for (int i = i0; i < i1; ++i) {
                        const float wx = (tx(0, i) - fx0 == (float)cx) ? tx(1, i) : tx(2, i);
                        for (int j = j0; j < j1; ++j) {
                            const float wy = (ty(0, j) - fy0 == (float)cy) ? ty(1, j) : ty(2, j);
                            sv = sv + __fmul_rn(gg(i * S + j), __fmul_rn(wy, wx));
                        }
                    }
                const int at = cell_at(cy);
                fsm[at] = fsm[at] + sv;
            }
        }
        // ---- 2c. groups whose corners leave the neighbourhood (and, NOST, the rare irregular
        // ones): sequential scatter ----
        // The group's in-map window cells are saved to registers and zeroed, so they serve as the
        // zeroed window scratch; afterwards cell = saved + scatter sum (lookup_bwd_kernel's order).
        if (__ballot(seq)) {
            float *Mq = fsm + mbase;
            const bool mine = seq && cx < WIN && X >= 0 && X < Wl;
            float keep[WIN];
#pragma unroll
            for (int ry = 0; ry < WIN; ++ry) {
                const int Y = ay + ry;
                keep[ry] = 0.f;
                if (mine && Y >= 0 && Y < Hl) {
                    keep[ry] = Mq[Y * Wl + X];
                    Mq[Y * Wl + X] = 0.0f;
                }
            }
            wave_lds_sync();
            auto scatter = [&](float xf, float yf, float val) {
                if (!in_map(xf, yf, Wl, Hl)) return;
                Mq[(int)yf * Wl + (int)xf] += val;  // window cells: the zeroed scratch
            };
            if constexpr (NOST) {
                // the group's taps and gradients by lane shuffles (all lanes take part; lane 0 of
                // each sequential group scatters)
                const int g0 = lane & ~(SLOTS - 1);
                for (int ii = 0; ii < S; ++ii) {
                    const float x0 = __shfl(a.f, g0 + ii, 64), ex = __shfl(a.lo, g0 + ii, 64);
                    const float wx = __shfl(a.hi, g0 + ii, 64), x1 = __fadd_rn(x0, 1.0f);
#pragma unroll
                    for (int j = 0; j < S; ++j) {
                        const float gv = __shfl(v[j], g0 + ii, 64);
                        const float y0 = __shfl(c.f, g0 + j, 64), ey = __shfl(c.lo, g0 + j, 64);
                        const float ny = __shfl(c.hi, g0 + j, 64), y1 = __fadd_rn(y0, 1.0f);
                        if (seq && cx == 0) {
                            scatter(x0, y0, __fmul_rn(gv, __fmul_rn(ey, ex)));
                            scatter(x1, y0, __fmul_rn(gv, __fmul_rn(ey, wx)));
                            scatter(x0, y1, __fmul_rn(gv, __fmul_rn(ny, ex)));
                            scatter(x1, y1, __fmul_rn(gv, __fmul_rn(ny, wx)));
                        }
                    }
                }
            } else if (seq && cx == 0) {
                for (int ii = 0; ii < S; ++ii) {
                    const float x0 = tx(0, ii), x1 = __fadd_rn(x0, 1.0f);
                    const float ex = tx(1, ii), wx = tx(2, ii);
                    for (int j = 0; j < S; ++j) {
                        const float gv = gg(ii * S + j);
                        const float y0 = ty(0, j), y1 = __fadd_rn(y0, 1.0f);
                        const float ey = ty(1, j), ny = ty(2, j);
                        scatter(x0, y0, __fmul_rn(gv, __fmul_rn(ey, ex)));
                        scatter(x1, y0, __fmul_rn(gv, __fmul_rn(ey, wx)));
                        scatter(x0, y1, __fmul_rn(gv, __fmul_rn(ny, ex)));
                        scatter(x1, y1, __fmul_rn(gv, __fmul_rn(ny, wx)));
                    }
                }
            }
            wave_lds_sync();
#pragma unroll
            for (int ry = 0; ry < WIN; ++ry) {
                const int Y = ay + ry;
                if (mine && Y >= 0 && Y < Hl) Mq[Y * Wl + X] = keep[ry] + Mq[Y * Wl + X];
            }
        }
        // the next lookup rewrites the staging: a compiler barrier keeps this lookup's LDS accesses
        // before the next one's (one wave's DS operations execute in issue order, so no wait is
        // needed: the map writes drain while the next lookup's taps are computed)
        if constexpr ((PROBE & 16) != 0) wave_lds_sync();
        else asm volatile("" ::: "memory");
    }
    __syncthreads();

    if constexpr ((PROBE & 2) != 0) return;
    // ---- 3. fold into level 0, write dC with its row / column maxima ----
    if constexpr (LEAN) {
        // 4 consecutive level-0 cells of one row per thread (x % 4 == 0): they share one level-2
        // and one level-3 cell and two level-1 cells, so the coarse chain is folded once per
        // shared cell — g2 = c2 + c3 / 4, g1 = c1 + g2 / 4, g0 = c0 + g1 / 4, each "+ coarse *
        // 0.25" only where the finer cell lies in the coarser level's pooled region (corr_pool_bwd)
        const int W1 = W >> 1, W2 = W >> 2, W3 = W >> 3;
        const int PH0 = 2 * (H >> 1), PH1 = 2 * (H >> 2), PH2 = 2 * (H >> 3);  // pooled rows of levels 0..2
        const int PW1 = 2 * (W1 >> 1), PW2 = 2 * (W2 >> 1);                      // pooled columns of levels 1, 2
        const f32x4 *F4 = reinterpret_cast<const f32x4 *>(fsm);
        const f32x2 *F2 = reinterpret_cast<const f32x2 *>(fsm);
        for (int u = tid; u < N / 4; u += NT) {
            const int m = 4 * u, y = m / W, x = m - y * W;
            const int y1 = y >> 1, y2 = y >> 2, y3 = y >> 3, x1 = x >> 1, x2 = x >> 2, x3 = x >> 3;
            // pooled-region flags: level-0 rows (columns always: W even), level-1 cells x1, x1 + 1,
            // the level-2 cell
            const bool p0 = y < PH0;
            const bool p1a = y1 < PH1 && x1 < PW1, p1b = y1 < PH1 && x1 + 1 < PW1;
            const bool p2 = y2 < PH2 && x2 < PW2;
            const int o0 = (o.moff[0] + y * W + x) >> 2, o1 = (o.moff[1] + y1 * W1 + x1) >> 1;
            const int o2 = o.moff[2] + y2 * W2 + x2, o3 = o.moff[3] + y3 * W3 + x3;
#pragma unroll
            for (int k = 0; k < WQ; ++k) {
                if (n0 + k >= NQ) continue;
                const f32x4 c0 = F4[o0 + ((k * o.qstr[0]) >> 2)];
                const f32x2 c1 = F2[o1 + ((k * o.qstr[1]) >> 1)];
                const float c2 = fsm[o2 + k * o.qstr[2]], c3 = fsm[o3 + k * o.qstr[3]];
                const float g2 = p2 ? c2 + c3 * 0.25f : c2;
                const float g1a = p1a ? c1.x + g2 * 0.25f : c1.x, g1b = p1b ? c1.y + g2 * 0.25f : c1.y;
                f32x4 r;
                r.x = p0 ? c0.x + g1a * 0.25f : c0.x;
                r.y = p0 ? c0.y + g1a * 0.25f : c0.y;
                r.z = p0 ? c0.z + g1b * 0.25f : c0.z;
                r.w = p0 ? c0.w + g1b * 0.25f : c0.w;
                f32x4 *dst = reinterpret_cast<f32x4 *>(o.dc + ((size_t)b * NQ + n0 + k) * N + m);
                if constexpr ((PROBE & 8) != 0) *dst = r;
                else __builtin_nontemporal_store(r, dst);
            }
        }
        return;
    }
    float rq[WQ];
#pragma unroll
    for (int k = 0; k < WQ; ++k) rq[k] = 0.f;
    if (W % 4 == 0 && ((uintptr_t)o.dc & 15) == 0 && ((uintptr_t)o.cpart & 15) == 0) {
        // 4 consecutive cells of one row per thread: one 16-B LDS read of level 0, one 8-B read of
        // level 1 (W/2 even, so its 2 cells are 8-B aligned), one value of each coarser level
        // (shared by the 4 cells), one 16-B store of dC
        for (int u = tid; u < N / 4; u += NT) {
            const int m = 4 * u, y = m / W, x = m - y * W;
            int off[kFusedLv];
            unsigned rc = 0;
#pragma unroll
            for (int v = 0; v < kFusedLv; ++v) {
                const int Hv = H >> v, Wv = W >> v, yv = y >> v, xv = x >> v;
                off[v] = o.moff[v < L ? v : 0] + yv * Wv + xv;
                if (v + 1 < L && yv < 2 * (Hv >> 1) && xv < 2 * (Wv >> 1)) rc |= 1u << v;
            }
            float cm[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < WQ; ++k) {
                if (n0 + k >= NQ) continue;
                float lv[kFusedLv][4];
                const float4 t0 = *reinterpret_cast<const float4 *>(fsm + off[0] + k * o.qstr[0]);
                lv[0][0] = t0.x, lv[0][1] = t0.y, lv[0][2] = t0.z, lv[0][3] = t0.w;
                if (L > 1) {
                    const float2 t1 = *reinterpret_cast<const float2 *>(fsm + off[1] + k * o.qstr[1]);
                    lv[1][0] = lv[1][1] = t1.x;
                    lv[1][2] = lv[1][3] = t1.y;
                }
#pragma unroll
                for (int v = 2; v < kFusedLv; ++v)
                    if (v < L) lv[v][0] = lv[v][1] = lv[v][2] = lv[v][3] = fsm[off[v] + k * o.qstr[v]];
                float res[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float up = 0.f;
                    bool have = false;
#pragma unroll
                    for (int v = kFusedLv - 1; v >= 0; --v) {
                        if (v >= L) continue;
                        float gv = lv[v][j];
                        if (have) gv = gv + up * 0.25f;  // fine += coarse * 0.25 (corr_pool_bwd order)
                        up = gv;
                        have = v > 0 && ((rc >> (v - 1)) & 1u);
                    }
                    res[j] = up;
                    const float av = fabsf(up);
                    cm[j] = fmaxf(cm[j], av);
                    rq[k] = fmaxf(rq[k], av);
                }
                // dC streams past the caches (non-temporal): same bits; in back-to-back launches of
                // this kernel alone the upstream gradients then stay cache-resident (T = 12: 153 ->
                // 135 us, profiles/r04q_kbench_bwd_nt.txt); in the training step, where the forward
                // runs in between, neutral (corr_backward 336-337 us)
                f32x4 *dst = reinterpret_cast<f32x4 *>(o.dc + ((size_t)b * NQ + n0 + k) * N + m);
                if constexpr ((PROBE & 8) != 0) *dst = f32x4{res[0], res[1], res[2], res[3]};
                else __builtin_nontemporal_store(f32x4{res[0], res[1], res[2], res[3]}, dst);
            }
            if (o.cpart)
                *reinterpret_cast<float4 *>(o.cpart + ((size_t)b * nqb + (blk - b * nqb)) * N + m) =
                    make_float4(cm[0], cm[1], cm[2], cm[3]);
            else if (o.cmax)
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (cm[j] > 0.f) atomicMax(&o.cmax[(size_t)b * N + m + j], __float_as_uint(cm[j]));
        }
    } else {
        for (int m = tid; m < N; m += NT) {
            const int y = m / W, x = m - y * W;
            float cm = 0.f;
            int off[kFusedLv];
            unsigned rc = 0;
#pragma unroll
            for (int v = 0; v < kFusedLv; ++v) {
                const int Hv = H >> v, Wv = W >> v, yv = y >> v, xv = x >> v;
                off[v] = o.moff[v < L ? v : 0] + yv * Wv + xv;
                if (v + 1 < L && yv < 2 * (Hv >> 1) && xv < 2 * (Wv >> 1)) rc |= 1u << v;
            }
#pragma unroll
            for (int k = 0; k < WQ; ++k) {
                if (n0 + k >= NQ) continue;
                float up = 0.f;
                bool have = false;
#pragma unroll
                for (int v = kFusedLv - 1; v >= 0; --v) {
                    if (v >= L) continue;
                    float gv = fsm[off[v] + k * o.qstr[v]];
                    if (have) gv = gv + up * 0.25f;
                    up = gv;
                    have = v > 0 && ((rc >> (v - 1)) & 1u);
                }
                if constexpr ((PROBE & 8) != 0) o.dc[((size_t)b * NQ + n0 + k) * N + m] = up;
                else __builtin_nontemporal_store(up, &o.dc[((size_t)b * NQ + n0 + k) * N + m]);
                const float av = fabsf(up);
                cm = fmaxf(cm, av);
                rq[k] = fmaxf(rq[k], av);
            }
            if (o.cpart)
                o.cpart[((size_t)b * nqb + (blk - b * nqb)) * N + m] = cm;
            else if (o.cmax && cm > 0.f)
                atomicMax(&o.cmax[(size_t)b * N + m], __float_as_uint(cm));
        }
    }
#pragma unroll
    for (int k = 0; k < WQ; ++k) {
        float r = rq[k];
#pragma unroll
        for (int sh = 32; sh >= 1; sh >>= 1) r = fmaxf(r, __shfl_xor(r, sh));
        if (lane == 0 && r > 0.f) atomicMax(&RM[k], __float_as_uint(r));
    }
    __syncthreads();
    if (o.rmax && tid < WQ && n0 + tid < NQ) o.rmax[(size_t)b * NQ + n0 + tid] = RM[tid];
}

}  // namespace

// corr_backward's fused path: hipErrorNotSupported when the workgroup's LDS image (BQ queries'
// maps at every level + per-wave staging) exceeds 160 KiB, or levels > 4, or T > kMaxLookups —
// the caller then takes the staged path.
namespace {
template <int S, bool SEP = false>
size_t fused_lds_bytes(int H, int W, int levels, FusedOut *o) {
    using ST = FusedStage<S>;
    // query stride = map cells plus one guard row, rounded up to an ODD multiple of 64 / BQ
    // floats: the BQ queries' maps then start in BQ different LDS banks (q * stride mod 64), so a
    // wave's read-modify-writes of neighbouring queries' windows (whose anchors differ by about
    // one pixel) do not collide.  Every map has a guard row above (row -1) and below (row H_l),
    // which the closed form's clamped rows write (one row may serve as one map's row H_l and the
    // next map's row -1); a level's region is a leading guard row and BQ query strides, rounded
    // to 4 floats (16-B zeroing; the fold's 16-B / 8-B reads of levels 0 / 1).  The per-wave
    // staging follows unless the kernel has none (fold_no_staging).
    size_t maps = 0;
    const int stag = 64 / ST::BQ;
    for (int l = 0; l < kFusedLv; ++l) {
        const int Hl = H >> l, Wl = W >> l;
        const int msz = l < levels ? Hl * Wl : 0;
        int qs = 0;
        if (msz) {
            qs = ((Hl + 1) * Wl + stag - 1) / stag * stag;
            if (ST::BQ > 1 && ((qs / stag) & 1) == 0) qs += stag;
        }
        if (o) o->moff[l] = (int)maps + (msz ? Wl : 0), o->msz[l] = msz, o->qstr[l] = qs;
        if (msz) maps += ((size_t)Wl + (size_t)ST::BQ * qs + 3) / 4 * 4;
    }
    if (o) o->aux = (int)maps;
    return (maps + (fold_no_staging<S, SEP>() ? 0 : (size_t)kFusedLv * ST::SIZE) + ST::BQ) * 4;
}

template <int S, bool SEP = false>
hipError_t launch_fused_s(const BwdLookups &lk, FusedOut o, hipStream_t s) {
    const size_t bytes = fused_lds_bytes<S, SEP>(o.H, o.W, o.L, &o);
    // the dynamic-LDS limit is raised once per device to the largest image this path accepts
    // (not to this call's size: a later, larger shape must not run against a smaller limit),
    // capped at what the device offers per workgroup
    int dev = 0, dev_max = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&dev_max, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (e != hipSuccess) return e;
    const int limit = std::min(160 * 1024, dev_max);
    if (bytes > (size_t)limit) return hipErrorNotSupported;
    // the lean fold (no maxima, 4 levels, 16-B rows of dC): the bf16x6 backward at radius 4
    const bool lean = S == 9 && !o.rmax && !o.cmax && !o.cpart && o.L == kFusedLv && o.W % 4 == 0 &&
                      ((uintptr_t)o.dc & 15) == 0;
    const void *fn = lean ? (const void *)lookup_bwd_fold_kernel<S, 0, SEP, S == 9>
                          : (const void *)lookup_bwd_fold_kernel<S, 0, SEP>;
    static std::atomic<unsigned long long> done[2];
    e = ensure_lds_limit(fn, limit, done[lean]);
    if (e != hipSuccess) return e;
    constexpr int WQ = FusedStage<S>::BQ, WAVES = kFusedLv;
    const int nqb = (o.NQ + WQ - 1) / WQ;
    o.nfold = nqb * o.B;
    // row-maxima blocks: at most half a round of workgroup slots (the fold's tail), >= 1 row per wave
    int extra = 0;
    if (o.rm.rows > 0) {
        const long rows = 2L * o.B * o.rm.rows;
        const long cap = std::max(1L, (long)(256 * std::max<size_t>(1, 160 * 1024 / bytes)) / 2);
        o.rm_rows_per_wave = (int)std::max(1L, (rows + cap * WAVES - 1) / (cap * WAVES));
        extra = (int)((rows + (long)o.rm_rows_per_wave * WAVES - 1) / ((long)o.rm_rows_per_wave * WAVES));
    }
    if (lean)
        hipLaunchKernelGGL((lookup_bwd_fold_kernel<S, 0, SEP, S == 9>), dim3((unsigned)(o.nfold + extra)),
                           dim3(64 * WAVES), bytes, s, lk, o);
    else
        hipLaunchKernelGGL((lookup_bwd_fold_kernel<S, 0, SEP>), dim3((unsigned)(o.nfold + extra)), dim3(64 * WAVES),
                           bytes, s, lk, o);
    return hipGetLastError();
}
}  // namespace

int lookup_bwd_fold_groups(int NQ, int radius) {
    if (radius < 0 || radius > 7) return 0;
    const int bq = 64 / fused_slots(2 * radius + 1);
    return (NQ + bq - 1) / bq;
}

hipError_t launch_lookup_bwd_fold(const float *const *coords, const float *const *grad_out, int T, int B, int NQ,
                                  int H, int W, int levels, int radius, float *dc, unsigned *rmax, unsigned *cmax,
                                  float *cpart, hipStream_t s, const FoldRowMax &rm, bool exact) {
    if (T < 1 || T > kMaxLookups || levels < 1 || levels > kFusedLv) return hipErrorNotSupported;
    BwdLookups lk{};
    lk.T = T;
    for (int k = 0; k < T; ++k) {
        lk.coords[k] = coords[k];
        lk.grad[k] = grad_out[k];
    }
    FusedOut o{};
    o.dc = dc, o.rmax = rmax, o.cmax = cmax, o.cpart = cpart;
    o.B = B, o.NQ = NQ, o.H = H, o.W = W, o.L = levels;
    o.rm = rm;
    return dispatch_radius(radius, [&](auto sc) {
        constexpr int S = decltype(sc)::value;
        // the separable closed form is instantiated for E-RAFT's radius only
        if constexpr (S == 9) {
            if (!exact) return launch_fused_s<9, true>(lk, o, s);
        }
        return launch_fused_s<S, false>(lk, o, s);
    });
}

}  // namespace corr
