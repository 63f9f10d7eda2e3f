// The on-demand lookup's per-block routines as corr_ondemand_conv.hip uses them: the general
// per-query routine (od_general_query) and the tiled path's phases A-D as one routine with an
// emit functor (od_tiled_block), so the results can go to an LDS tile instead of global memory.
//
// THIS IS A COPY of corr_ondemand.hip's od_general_query and of the body of its
// ondemand_lookup_tiled_kernel (the originals; DESIGN §21 says why there are two): the same
// statements in the same order, with the two store sites replaced by the functor and `general`
// added to the route choice.  A change to the arithmetic, the route choice or TlSmem in one of
// them belongs in the other too; tests/test_ondemand_conv.py's selection-weight tests compare the
// two bit for bit on both routes.  Internal, not part of the C-ABI.
#pragma once

#include "corr_build_common.h"
#include "corr_common.h"
#include "corr_div.h"
#include "corr_ondemand_common.h"
#include "corr_taps.h"

namespace corr {
namespace {  // per translation unit, as the kernels that use these

constexpr int kOdMaxCells = (kOdMaxS + 1) * (kOdMaxS + 1);
constexpr int kOdChunk = 64;  // 16-B pieces of a row held in registers at a time (256 features)

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b, float acc) {
    acc = __builtin_fmaf(a[0], b[0], acc);
    acc = __builtin_fmaf(a[1], b[1], acc);
    acc = __builtin_fmaf(a[2], b[2], acc);
    return __builtin_fmaf(a[3], b[3], acc);
}

// One whole-wave dot product of two rows of D4 16-B pieces (the irregular path only).
__device__ __forceinline__ float wave_dot(const f32x4 *__restrict__ q, const f32x4 *__restrict__ row, int D4,
                                          int lane) {
    float acc = 0.0f;
    for (int c = lane; c < D4; c += 64) acc = dot4(q[c], row[c], acc);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) acc += __shfl_xor(acc, m);
    return acc;
}

// What every lookup workgroup needs (by value: no device-side tables).
struct OdArgs {
    const f32x4 *F1;                 // fmap1 rows [B][N][D4]
    const f32x4 *P[CORR_MAX_LEVELS]; // pooled fmap2 rows [B][H_l W_l][D4]
    const float *coords;
    float *out;
    int B, N, H, W, L, D4, S;
    float sqrtD;
};

// Per-level constants of a workgroup.
struct OdLevel {
    const f32x4 *Pb;  // this batch item's rows
    int Hl, Wl;
    float inv_scale, rdx, rdy;
};

__device__ __forceinline__ OdLevel od_level(const OdArgs &a, int b, int l) {
    OdLevel v;
    v.Hl = a.H >> l, v.Wl = a.W >> l;
    v.Pb = a.P[l] + (size_t)b * v.Hl * v.Wl * a.D4;
    v.inv_scale = 1.0f / (float)(1 << l);
    v.rdx = recip_rn((float)(v.Wl - 1)), v.rdy = recip_rn((float)(v.Hl - 1));
    return v;
}

// The general path for ONE query (b, n) at one level, run by one wave: outputs t = 0 .. K-1 to
// tile[t * tstride].  cell (>= (S+1)^2 floats) and tap (6 x 16 floats) are the wave's own LDS.
__device__ __forceinline__ void od_general_query(const OdArgs &a, const OdLevel &lv, int b, int n, float *cell,
                                                 float (*tap)[kOdMaxS + 1], float *tile, int tstride, int lane) {
    const int S = a.S, D4 = a.D4, R = (S - 1) / 2, K = S * S, S1 = S + 1, NC = S1 * S1;
    const int Hl = lv.Hl, Wl = lv.Wl;
    const f32x4 *Pb = lv.Pb;
    const float sqrtD = a.sqrtD;
    const int g = lane >> 3, sub = lane & 7;  // cell of the batch, 16-B piece of the step
    const f32x4 *Q = a.F1 + ((size_t)b * a.N + n) * D4;
    // ---- 1. taps ----
    const float cxv = a.coords[((size_t)b * 2 + 0) * a.N + n], cyv = a.coords[((size_t)b * 2 + 1) * a.N + n];
    if (lane < S) {
        const Axis tx = tap_axis(cxv, lv.inv_scale, lane, R, Wl, lv.rdx);
        const Axis ty = tap_axis(cyv, lv.inv_scale, lane, R, Hl, lv.rdy);
        tap[0][lane] = tx.f, tap[1][lane] = tx.lo, tap[2][lane] = tx.hi;
        tap[3][lane] = ty.f, tap[4][lane] = ty.lo, tap[5][lane] = ty.hi;
    }
    wave_sync();
    const int ax = anchor_of(tap[0][0]), ay = anchor_of(tap[3][0]);
    const bool far = ax == kFarAnchor || ay == kFarAnchor;
    bool reg_lane = true;
    if (lane < S) reg_lane = tap[0][lane] == (float)(ax + lane) && tap[3][lane] == (float)(ay + lane);
    const bool regular = far || __all(reg_lane);  // wave-uniform
    if (regular) {
        // ---- 2. the (S+1)^2 neighbourhood's dot products (all 0 for a far query) ----
        for (int d0 = 0; d0 < D4; d0 += kOdChunk) {
            f32x4 qv[8];  // this lane's pieces of the query's chunk
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int p = d0 + 8 * i + sub;
                qv[i] = p < D4 ? Q[p] : f32x4{0.f, 0.f, 0.f, 0.f};
            }
            for (int c0 = 0; c0 < NC; c0 += 8) {
                const int c = c0 + g;
                const int cy = c / S1, cx = c - cy * S1;
                const int y = ay + cy, x = ax + cx;
                const bool ok = !far && c < NC && (unsigned)y < (unsigned)Hl && (unsigned)x < (unsigned)Wl;
                float acc = 0.0f;
                if (ok) {
                    const f32x4 *row = Pb + ((size_t)y * Wl + x) * D4;
                    f32x4 rv[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int p = d0 + 8 * i + sub;
                        rv[i] = p < D4 ? row[p] : f32x4{0.f, 0.f, 0.f, 0.f};
                    }
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc = dot4(qv[i], rv[i], acc);
                }
                acc += __shfl_xor(acc, 1);
                acc += __shfl_xor(acc, 2);
                acc += __shfl_xor(acc, 4);
                if (sub == 0 && c < NC) cell[c] = d0 == 0 ? acc : cell[c] + acc;
            }
        }
        wave_sync();
        for (int c = lane; c < NC; c += 64) cell[c] = __fdiv_rn(cell[c], sqrtD);
        wave_sync();
        // ---- 3. taps (i, j): corners at neighbourhood columns i, i+1 and rows j, j+1 ----
        for (int t = lane; t < K; t += 64) {
            const int i = t / S, j = t - i * S;
            const float ex = tap[1][i], wx = tap[2][i], ey = tap[4][j], ny = tap[5][j];
            const float *c = cell + j * S1 + i;
            float acc = __fmul_rn(c[0], __fmul_rn(ey, ex));
            acc = __builtin_fmaf(c[1], __fmul_rn(ey, wx), acc);
            acc = __builtin_fmaf(c[S1], __fmul_rn(ny, ex), acc);
            acc = __builtin_fmaf(c[S1 + 1], __fmul_rn(ny, wx), acc);
            tile[(size_t)t * tstride] = acc;
        }
    } else {
        // irregular taps: every corner from its own tap's floor
        for (int t = 0; t < K; ++t) {
            const int i = t / S, j = t - i * S;
            const float x0 = tap[0][i], ex = tap[1][i], wx = tap[2][i];
            const float y0 = tap[3][j], ey = tap[4][j], ny = tap[5][j];
            const float x1 = __fadd_rn(x0, 1.0f), y1 = __fadd_rn(y0, 1.0f);
            auto fetch = [&](float xf, float yf) -> float {
                if (!in_map(xf, yf, Wl, Hl)) return 0.0f;  // wave-uniform
                const float d = wave_dot(Q, Pb + ((size_t)(int)yf * Wl + (int)xf) * D4, D4, lane);
                return __fdiv_rn(d, sqrtD);
            };
            float acc = __fmul_rn(fetch(x0, y0), __fmul_rn(ey, ex));
            acc = __builtin_fmaf(fetch(x1, y0), __fmul_rn(ey, wx), acc);
            acc = __builtin_fmaf(fetch(x0, y1), __fmul_rn(ny, ex), acc);
            acc = __builtin_fmaf(fetch(x1, y1), __fmul_rn(ny, wx), acc);
            if (lane == 0) tile[(size_t)t * tstride] = acc;
        }
    }
    wave_sync();  // the next query rewrites tap / cell
}

// ---------------------------------------------------------------------------------------
// Tiled path (radius <= 4).  A workgroup (4 waves) owns an 8 x 8 block of queries of one batch
// item at one level.
//   A. thread q < 64 computes its query's taps; the block is TILED when every query in the image
//      is regular and not far, and the bounding box of the queries' (S+1)^2 neighbourhoods
//      (unclipped: cells outside the map count, and are staged as zeros) holds at most kTlCells
//      cells — 18 x 18 at r = 4, the uniform-flow case at level 0, is 324.  Otherwise the block
//      runs the general path (od_general_query per query): a function of the coordinates only.
//   B. C[64 queries][box cells] = Q Cells^T on v_mfma_f32_32x32x2_f32 (fp32 operands, an fp32
//      fmaf chain in k order per entry): D is walked in chunks of 16 features, staged k-major in
//      LDS (Xs[k][row]: operand reads are consecutive, staging writes conflict-free), the next
//      chunk's global loads in flight during the MFMAs.  Wave w owns box-cell tiles w, w+4, ..
//      (32 cells each) x both 32-query tiles.
//   C. every accumulator entry whose cell lies in its query's own neighbourhood is scaled and
//      written to win[q][cy (S+1) + cx]; each neighbourhood cell is in the box, so each is written
//      exactly once.
//   D. thread (q, i) recomputes its taps (tap_axis: the same bits) and combines as corr_lookup.
constexpr int kTlMaxS = 9, kTlQ = 64, kTlNT = 13, kTlCells = 32 * kTlNT /* 416 */, kTlDK = 16;
constexpr int kTlRows = kTlQ + kTlCells, kTlRS = kTlRows + 2;  // row stride = 2 mod 8: conflict-free staging writes
constexpr int kTlWS = (kTlMaxS + 1) * (kTlMaxS + 1) + 1;       // odd stride: lane = query reads conflict-free
constexpr int kTlItems = (kTlRows * (kTlDK / 4) + 255) / 256;   // staged 16-B pieces per thread and chunk

struct TlSmem {
    union {
        float xs[kTlDK][kTlRS];  // the chunk's operands, k-major: rows 0..63 queries, 64.. box cells
        struct {                 // general-path fallback (od_general_query)
            float cell[kOdWaves][kOdMaxCells];
            float tap[kOdWaves][6][kOdMaxS + 1];
        } g;
    } u;
    float win[kTlQ * kTlWS];  // neighbourhoods [q][cy (S+1) + cx]; fallback: the outputs [t][q]
    float cx[kTlQ], cy[kTlQ];
    int ax[kTlQ], ay[kTlQ];   // anchors; kFarAnchor for queries outside the image
    int box[4];               // min x, min y, max x, max y over the block
    int bad;
};
static_assert(kTlMaxS * kTlMaxS * kTlQ <= kTlQ * kTlWS, "the fallback's output tile fits in win");

// Phases A-D for the 8 x 8 block at (qy0, qx0) of batch item b at level lv, run by the whole
// workgroup (256 threads, all of which must call it).  `general` forces the per-query routine.
// The results leave through `emit`:
//   emit.general(t, qy, qx, q, v)   output t = i S + j of in-image query q = (qy, qx), fallback;
//   emit.column(qy, qx, q, i)       returns a callable (j, v) for outputs (i, 0 .. S-1), tiled.
// Nothing is emitted for queries outside the image.  Begins with a barrier after which sm is
// rewritten, so consecutive calls (levels) need none between them; the emitted values of one
// call are complete for the workgroup only after the caller's next barrier.
template <class Emit>
__device__ __forceinline__ void od_tiled_block(TlSmem &sm, const OdArgs &a, const OdLevel &lv, int b, int qy0,
                                               int qx0, bool general, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int S = a.S, R = (S - 1) / 2, K = S * S, S1 = S + 1, D4 = a.D4, N = a.N, W = a.W, H = a.H;
    const int Hl = lv.Hl, Wl = lv.Wl;

    // ---- A. anchors, regularity, bounding box ----
    if (tid == 0) {
        sm.box[0] = sm.box[1] = 0x7fffffff;
        sm.box[2] = sm.box[3] = -0x7fffffff;
        sm.bad = 0;
    }
    __syncthreads();
    if (tid < kTlQ) {
        const int qy = qy0 + (tid >> 3), qx = qx0 + (tid & 7);
        int ax = kFarAnchor, ay = kFarAnchor;
        float cxv = 0.f, cyv = 0.f;
        if (qy < H && qx < W) {
            const int n = qy * W + qx;
            cxv = a.coords[((size_t)b * 2 + 0) * N + n], cyv = a.coords[((size_t)b * 2 + 1) * N + n];
            const Axis x0 = tap_axis(cxv, lv.inv_scale, 0, R, Wl, lv.rdx);
            const Axis y0 = tap_axis(cyv, lv.inv_scale, 0, R, Hl, lv.rdy);
            ax = anchor_of(x0.f), ay = anchor_of(y0.f);
            bool ok = ax != kFarAnchor && ay != kFarAnchor;
            for (int t = 1; t < S && ok; ++t) {
                const Axis tx = tap_axis(cxv, lv.inv_scale, t, R, Wl, lv.rdx);
                const Axis ty = tap_axis(cyv, lv.inv_scale, t, R, Hl, lv.rdy);
                ok = tx.f == (float)(ax + t) && ty.f == (float)(ay + t);
            }
            if (!ok) {
                atomicOr(&sm.bad, 1);
            } else {
                atomicMin(&sm.box[0], ax), atomicMin(&sm.box[1], ay);
                atomicMax(&sm.box[2], ax + S), atomicMax(&sm.box[3], ay + S);
            }
        }
        sm.ax[tid] = ax, sm.ay[tid] = ay, sm.cx[tid] = cxv, sm.cy[tid] = cyv;
    }
    __syncthreads();
    const int minx = sm.box[0], miny = sm.box[1];
    const long long bw = (long long)sm.box[2] - minx + 1, bh = (long long)sm.box[3] - miny + 1;
    const bool tiled = !general && !sm.bad && bw * bh <= kTlCells;  // workgroup-uniform
    __syncthreads();  // everyone has read box / bad before u is reused

    if (!tiled) {
        // ---- general path for the block's queries; outputs [t][q] in win ----
        for (int q = w; q < kTlQ; q += kOdWaves) {
            const int qy = qy0 + (q >> 3), qx = qx0 + (q & 7);
            if (qy < H && qx < W)
                od_general_query(a, lv, b, qy * W + qx, sm.u.g.cell[w], sm.u.g.tap[w], &sm.win[q], kTlQ, lane);
        }
        __syncthreads();
        for (int idx = tid; idx < K * kTlQ; idx += 256) {
            const int t = idx >> 6, q = idx & 63;
            const int qy = qy0 + (q >> 3), qx = qx0 + (q & 7);
            if (qy < H && qx < W) emit.general(t, qy, qx, q, sm.win[t * kTlQ + q]);
        }
        return;
    }

    // ---- B. C = Q Cells^T ----
    const int ibw = (int)bw, ncell = (int)(bw * bh), NT = (ncell + 31) >> 5;
    const int nrows = kTlQ + 32 * NT;
    // this thread's staged pieces: row (query or box cell) and which 16 B of the chunk
    const f32x4 *src[kTlItems];
    int dst[kTlItems], kq[kTlItems];
#pragma unroll
    for (int i = 0; i < kTlItems; ++i) {
        const int idx = tid + 256 * i, row = idx >> 2;
        kq[i] = idx & 3;
        dst[i] = row < nrows ? row : -1;
        src[i] = nullptr;
        if (row < kTlQ) {
            const int qy = qy0 + (row >> 3), qx = qx0 + (row & 7);
            if (qy < H && qx < W) src[i] = a.F1 + ((size_t)b * N + qy * W + qx) * D4;
        } else if (row - kTlQ < ncell) {
            const int c = row - kTlQ, by = c / ibw, bx = c - by * ibw;
            const int y = miny + by, x = minx + bx;
            if ((unsigned)y < (unsigned)Hl && (unsigned)x < (unsigned)Wl) src[i] = lv.Pb + ((size_t)y * Wl + x) * D4;
        }
    }
    f32x4 stage[kTlItems];
    auto fetch = [&](int d0) {  // d0: first 16-B piece of the chunk
#pragma unroll
        for (int i = 0; i < kTlItems; ++i) {
            const int p = d0 + kq[i];
            stage[i] = (src[i] && p < D4) ? src[i][p] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    f32x16 acc[2][4];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[m][j][e] = 0.f;
    const int half = lane >> 5, l32 = lane & 31;
    fetch(0);
    for (int d0 = 0; d0 < D4; d0 += kTlDK / 4) {
        __syncthreads();  // the previous chunk's MFMAs have read xs
#pragma unroll
        for (int i = 0; i < kTlItems; ++i) {
            if (dst[i] >= 0) {
#pragma unroll
                for (int e = 0; e < 4; ++e) sm.u.xs[4 * kq[i] + e][dst[i]] = stage[i][e];
            }
        }
        __syncthreads();
        if (d0 + kTlDK / 4 < D4) fetch(d0 + kTlDK / 4);
#pragma unroll
        for (int kk = 0; kk < kTlDK / 2; ++kk) {
            const float *xk = sm.u.xs[2 * kk + half];
            const float a0 = xk[l32], a1 = xk[32 + l32];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int nt = w + 4 * j;
                if (nt < NT) {  // wave-uniform
                    const float bv = xk[kTlQ + 32 * nt + l32];
                    acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, bv, acc[0][j], 0, 0, 0);
                    acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, bv, acc[1][j], 0, 0, 0);
                }
            }
        }
    }
    // ---- C. accumulators -> the queries' own neighbourhoods ----
    // C[row = query 32 m + (e & 3) + 8 (e >> 2) + 4 half][col = cell 32 nt + l32]
#pragma unroll
    for (int m = 0; m < 2; ++m) {
        int qax[16], qay[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int q = 32 * m + (e & 3) + 8 * (e >> 2) + 4 * half;
            qax[e] = sm.ax[q], qay[e] = sm.ay[q];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int nt = w + 4 * j, c = 32 * nt + l32;
            if (nt < NT && c < ncell) {
                const int by = c / ibw, bx = c - by * ibw;
                const int y = miny + by, x = minx + bx;
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int q = 32 * m + (e & 3) + 8 * (e >> 2) + 4 * half;
                    const unsigned cy = (unsigned)(y - qay[e]), cx = (unsigned)(x - qax[e]);
                    if (cy <= (unsigned)S && cx <= (unsigned)S)
                        sm.win[q * kTlWS + cy * S1 + cx] = __fdiv_rn(acc[m][j][e], a.sqrtD);
                }
            }
        }
    }
    __syncthreads();
    // ---- D. taps: thread (q, i) -> outputs (i, 0 .. S-1) ----
    for (int it = tid; it < kTlQ * S; it += 256) {
        const int q = it & 63, i = it >> 6;
        const int qy = qy0 + (q >> 3), qx = qx0 + (q & 7);
        if (qy >= H || qx >= W) continue;
        const Axis tx = tap_axis(sm.cx[q], lv.inv_scale, i, R, Wl, lv.rdx);
        const float cyv = sm.cy[q];
        const float *col = &sm.win[q * kTlWS + i];
        auto o = emit.column(qy, qx, q, i);
        float c0 = col[0], c1 = col[1];
        for (int j = 0; j < S; ++j) {
            const Axis ty = tap_axis(cyv, lv.inv_scale, j, R, Hl, lv.rdy);
            const float n0 = col[(j + 1) * S1], n1 = col[(j + 1) * S1 + 1];
            float acc = __fmul_rn(c0, __fmul_rn(ty.lo, tx.lo));
            acc = __builtin_fmaf(c1, __fmul_rn(ty.lo, tx.hi), acc);
            acc = __builtin_fmaf(n0, __fmul_rn(ty.hi, tx.lo), acc);
            acc = __builtin_fmaf(n1, __fmul_rn(ty.hi, tx.hi), acc);
            o(j, acc);
            c0 = n0, c1 = n1;
        }
    }
}

}  // namespace
}  // namespace corr
