"""Shared helpers for the test-suite (fixture loading, parity metrics)."""
import os

import numpy as np
import torch

import prng

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# north_star: "fp32 correlation and lookup within 1e-4 relative", defined as the
# norm-relative error ||a - b||_inf / ||b||_inf.
REL_TOL = 1e-4

DEV = "cuda:0"


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False))


def golden_names(prefix="g_"):
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith(prefix) and f.endswith(".npz"))


def norm_rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin), "non-finite pattern differs"
    d = np.abs(a[fin] - b[fin]).max(initial=0.0)
    s = np.abs(b[fin]).max(initial=0.0)
    return d / s if s > 0 else d


def bit_equal(a, b):
    """Bitwise equality, treating every NaN as equal to every NaN."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    if not np.array_equal(na, nb):
        return False
    return np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb])


def voxel_edge_cases(g, kind):
    """Case names of g_voxel_edges.npz: kind "d" (VoxelGrid) or "m" (EventSequenceToVoxelGrid)."""
    pre = kind + "_ev_"
    return sorted(k[len(pre):] for k in g if k.startswith(pre))


def same_zero_nan_pattern(a, b):
    return np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a == 0, b == 0)


def voxel_norm_within_bar(n, ref):
    """The suite's bar for a normalised voxel grid, 1e-6 of max|v|, over the finite cells, and
    the same zero and NaN pattern."""
    fin = np.isfinite(ref)
    return same_zero_nan_pattern(n, ref) and \
        np.abs(n[fin] - ref[fin]).max(initial=0.0) <= 1e-6 * np.abs(ref[fin]).max(initial=0.0)


def tiled_levels(B, H, W, L, device, fill=None, NQ=None):
    """Separate tiled level tensors [B*NQ, map_floats(H_l, W_l)] (the library's value pyramid,
    include/corr_mi355x.h), optionally filled with `fill`."""
    import torch
    from eraft_amd.corr import map_floats
    BN = B * (H * W if NQ is None else NQ)
    out = []
    for l in range(L):
        t = torch.empty(BN, map_floats(H >> l, W >> l), dtype=torch.float32, device=device)
        if fill is not None:
            t.fill_(fill)
        out.append(t)
    return out


def export_levels(levels, H, W):
    """The tiled levels in the reference's layout, as numpy [BN, 1, H_l, W_l] arrays."""
    from eraft_amd import _lib
    return [p.cpu().numpy() for p in _lib.pyramid_export(levels, H, W)]


def build_level0(t1, t2, algo, ws=None):
    """Level 0 of one build (corr_build_ex), row-major numpy [B*N, H*W]."""
    from eraft_amd import _lib
    B, _, H, W = t2.shape
    lv = tiled_levels(B, H, W, 1, t1.device, NQ=t1.shape[2] * t1.shape[3])
    _lib.build(t1, t2, lv, algo, ws)
    return export_levels(lv, H, W)[0].reshape(-1, H * W)


def _bwd_case(T, B, H, W, L, r, seed):
    """T lookups' coords (mixed regular / pixel-grid / far taps) and upstream gradients."""
    K = (2 * r + 1) ** 2
    cs, gs = [], []
    for t in range(T):
        c = prng.lookup_coords(seed + t, B, H, W, 0.7 * t)
        if t % 3 == 1:  # integer grid: the general range-gather path
            ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
            c[:, 0], c[:, 1] = xs, ys
        if t % 5 == 2:  # far taps: the sequential scatter path
            c[0, 0, 1, :2] = [1048000.5, -3.25]
        c[0, :, 0, t % W] = np.float32(np.nan)
        cs.append(torch.from_numpy(c).to(DEV))
        gs.append(torch.from_numpy(prng.gauss(seed + 100 + t, (B, L * K, H, W))).to(DEV))
    return cs, gs


def cell_magnitude(coords_list, abs_grads_list, H, W, L, r):
    """M [B*NQ, 1, H, W]: the fp32 oracle's lookup_bwd over all lookups applied to |g|, then
    pool_bwd.  Bilinear weights are non-negative, so M is a sum of non-negative terms that bounds
    sum |contribution| of every level-0 cell of dC; a cell no window touches has M = 0.  The
    coords may be a query-row slab [B, 2, rows, Wq] of the (H, W) map."""
    from oracle import oracle
    B = coords_list[0].shape[0]
    NQ = int(np.prod(coords_list[0].shape[2:]))
    gp = [np.zeros((B * NQ, 1, h, w), np.float32) for h, w in oracle.level_shapes(H, W, L)]
    for c, g in zip(coords_list, abs_grads_list):
        oracle.lookup_bwd_rows(np.asarray(c, np.float32), np.abs(np.asarray(g, np.float32)), gp, H, W, r)
    oracle.pool_bwd(gp, H, W)
    return gp[0]


def cell_bound_k(T, L):
    """k of within_cell_bound.  Consecutive taps are 1 +- 1 ulp apart, so at most 3 taps per axis
    have their floor in {x - 1, x}: a cell collects at most 9 corner contributions per lookup and
    level.  T * L of those, L - 1 fold additions and 3 roundings inside a product give each path's
    first-order error <= (9 T L + L + 3) * 2^-24 * M; two such paths are compared, hence the 2."""
    return 2 * (9 * T * L + L + 3)


def cell_ratio(a, b, M):
    """max |a - b| / (2^-24 * M) over the finite cells with M > 0 (0.0 when there is none)."""
    a, b, M = (np.asarray(t, np.float64).reshape(-1) for t in (a, b, M))
    sel = np.isfinite(a) & np.isfinite(b) & (M > 0)
    return float((np.abs(a[sel] - b[sel]) / (2.0 ** -24 * M[sel])).max(initial=0.0))


def within_cell_bound(a, b, M, T, L):
    """|a - b| <= k * (2^-24 * M + 2^-149) in every cell, k = cell_bound_k(T, L) (the 2^-149 term:
    k denormal steps where products underflow); where M = 0 no window touches the cell, and a and b
    must be bit-identical there; a and b must have the same non-finite cells, which are not
    compared further.  M: cell_magnitude of the same lookups."""
    a32 = np.ascontiguousarray(a, np.float32).reshape(-1)
    b32 = np.ascontiguousarray(b, np.float32).reshape(-1)
    M = np.asarray(M, np.float64).reshape(-1)
    if not (a32.shape == b32.shape == M.shape):
        return False
    if not (np.array_equal(np.isnan(a32), np.isnan(b32)) and np.array_equal(np.isposinf(a32), np.isposinf(b32))
            and np.array_equal(np.isneginf(a32), np.isneginf(b32))):
        return False
    untouched = (M == 0) & ~np.isnan(b32)
    if not np.array_equal(a32.view(np.uint32)[untouched], b32.view(np.uint32)[untouched]):
        return False
    fin = np.isfinite(b32) & ~untouched
    d = np.abs(a32[fin].astype(np.float64) - b32[fin].astype(np.float64))
    return bool((d <= cell_bound_k(T, L) * (2.0 ** -24 * M[fin] + 2.0 ** -149)).all())
