"""Helpers of test_large_volume.py: the shapes that carry a correlation volume past the 2^31 and
2^32 addressing marks, the query rows worth sampling around those marks, and the comparison code
of the dense (every word, on the device) legs.  The comparison code takes tensors and callables
only, so test_large_helper.py runs it on the CPU against planted errors."""
import math

import numpy as np
import torch

import prng

TILE_W = 4


def map_floats(h, w):
    """Words of one query's tiled level map (include/corr_mi355x.h); restated here so that the
    CPU tests do not need the built library."""
    return ((h + 3) // 4) * ((w + TILE_W - 1) // TILE_W) * 4 * TILE_W


# Word indices counted from the start of a level: byte offsets 2^31 and 2^32, then the signed and
# the unsigned 32-bit element index.
MARKS = (2 ** 29, 2 ** 30, 2 ** 31, 2 ** 32)

# B, H, W, levels, radius; D = 16 everywhere.  `crosses`: level -> the marks the TILED level
# contains (a word index >= mark exists), as DESIGN.md's table claims them.
CASES = {
    "one-map": dict(B=1, H=181, W=257, L=4, r=4, crosses={0: 2 ** 31, 1: 2 ** 29}),
    "many-maps": dict(B=19, H=98, W=110, L=4, r=4, crosses={0: 2 ** 31}),
    "tiny-maps": dict(B=516, H=32, W=64, L=4, r=4, crosses={0: 2 ** 31}),
    "past-2^32": dict(B=1, H=207, W=318, L=2, r=4, crosses={0: 2 ** 32, 1: 2 ** 30}),
}
D = 16


def row_words(H, W, L, tiled):
    """Words of one query's map at every level, tiled (value pyramid) or row-major (gradients)."""
    return [map_floats(H >> l, W >> l) if tiled else (H >> l) * (W >> l) for l in range(L)]


def level_words(case, tiled):
    c = CASES[case]
    return [c["B"] * c["H"] * c["W"] * w for w in row_words(c["H"], c["W"], c["L"], tiled)]


def pyramid_bytes(case, tiled):
    return 4 * sum(level_words(case, tiled))


def sample_queries(B, NQ, row_words_per_level, spread=96):
    """Flat query indices (sorted, unique) worth taking to the host: the first and last two; for
    every mark inside every level (one entry of row_words_per_level per level and layout) the rows
    holding word mark - 1 and word mark, and their neighbours; the last query of a batch item and
    the first of the next at the batch boundary nearest each mark; a linspace over the rest."""
    BN = B * NQ
    q = {0, 1, BN - 2, BN - 1}
    for w in row_words_per_level:
        for m in MARKS:
            if m >= BN * w:
                continue
            lo, hi = (m - 1) // w, m // w
            q.update((lo - 1, lo, hi, hi + 1))
            b = min(max(int(round(hi / NQ)), 1), B - 1)  # nearest boundary between two batch items
            if B > 1:
                q.update((b * NQ - 1, b * NQ))
    q.update(int(v) for v in np.linspace(0, BN - 1, spread))
    return np.array(sorted(v for v in q if 0 <= v < BN), np.int64)


def case_sample(case):
    c = CASES[case]
    rows = row_words(c["H"], c["W"], c["L"], True) + row_words(c["H"], c["W"], c["L"], False)
    return sample_queries(c["B"], c["H"] * c["W"], rows)


def plant_coords(coords, sample):
    """Among the sampled queries of coords [B, 2, H, W] (numpy, modified in place): every fourth
    keeps its Gaussian flow, the others take special_coords' edge values, their own integer grid
    position, and (one in sixteen) NaN / inf."""
    B, _, H, W = coords.shape
    flat = coords.reshape(B, 2, H * W)
    sp = prng.special_coords(1, H, W).reshape(2, -1)[:, :16]
    bad = np.array([[np.nan, 3.0], [np.inf, 2.5], [1.5, -np.inf], [np.nan, np.nan]], np.float32)
    for k, qi in enumerate(sample):
        b, n = divmod(int(qi), H * W)
        if k % 16 == 7:
            flat[b, :, n] = bad[(k // 16) % len(bad)]
        elif k % 4 == 1:
            flat[b, :, n] = sp[:, (k // 4) % 16]
        elif k % 4 == 2:
            flat[b, :, n] = (n % W, n // W)
    return coords


def chunks(B, NQ, rows):
    """(b0, b1, r0, r1): batch items b0 .. b1 - 1, query rows r0 .. r1 - 1 of each, covering
    [B, NQ] once in pieces of about `rows` query rows; a piece holds whole batch items or a row
    range of one.  Its flat queries are [b0 * NQ + r0, (b1 - 1) * NQ + r1)."""
    rows = max(1, int(rows))
    if NQ > rows:
        for b in range(B):
            for r0 in range(0, NQ, rows):
                yield b, b + 1, r0, min(NQ, r0 + rows)
    else:
        nb = rows // NQ
        for b0 in range(0, B, nb):
            yield b0, min(B, b0 + nb), 0, NQ


def flat_range(c, NQ):
    b0, b1, r0, r1 = c
    return b0 * NQ + r0, (b1 - 1) * NQ + r1


def pool_restated(x):
    """avg_pool2d(2, 2) of [n, 1, H, W] in the oracle's order, ((a + b) + c) + d then * 0.25, as
    strided fp32 tensor adds (every step rounds to fp32 as the C does)."""
    Hr, Wr = 2 * (x.shape[2] // 2), 2 * (x.shape[3] // 2)
    a, b = x[:, :, 0:Hr:2, 0:Wr:2], x[:, :, 0:Hr:2, 1:Wr:2]
    c, d = x[:, :, 1:Hr:2, 0:Wr:2], x[:, :, 1:Hr:2, 1:Wr:2]
    return (((a + b) + c) + d) * 0.25


def same_bits(a, b):
    """Bitwise equality of two fp32 tensors, every NaN equal to every NaN; on the tensors' device."""
    if a.shape != b.shape:
        return False
    na, nb = torch.isnan(a), torch.isnan(b)
    ai = torch.where(na, torch.zeros_like(a), a).contiguous().view(torch.int32)
    bi = torch.where(nb, torch.zeros_like(b), b).contiguous().view(torch.int32)
    return bool(torch.equal(na, nb) and torch.equal(ai, bi))


def level0_ratio(got, f1, f2, c, algo, rel_tol):
    """Max error / bound of a chunk `got` [nb, R, N] of level 0 (row-major) against
    f1[b, :, rows]^T f2[b] / sqrt(D) in fp64 (f1 [B, D, NQ], f2 [B, D, N]).  bf16x6: element-wise,
    bound (3 + 6 ceil(D / 32)) 2^-24 sum |a||b| / sqrt(D) from a second matmul of magnitudes (an
    element whose bound is 0 must be exact: its ratio is inf otherwise).  f16x3 and fp32: per
    query row, max |err| / max |ref| against rel_tol.  The features are finite, so a word of `got`
    that is not (the likeliest content of a word no store reached) gives inf in either form."""
    b0, b1, r0, r1 = c
    Dd = f1.shape[1]
    if not bool(torch.isfinite(got).all()):
        return math.inf
    a = f1[b0:b1, :, r0:r1].double().transpose(1, 2)
    t = f2[b0:b1].double()
    ref = torch.matmul(a, t) / math.sqrt(Dd)
    err = (got.double() - ref).abs_()
    if algo == "bf16x6":
        bound = torch.matmul(a.abs(), t.abs()).mul_((3 + 6 * ((Dd + 31) // 32)) * 2.0 ** -24 / math.sqrt(Dd))
        ratio = torch.where(err <= bound, err / bound.clamp_min(1e-300), torch.full_like(err, math.inf))
        return float(ratio.max())
    scale = ref.abs_().amax(dim=-1)
    ratio = float((err.amax(dim=-1) / scale.clamp_min(1e-300)).max()) / rel_tol
    return ratio if math.isfinite(ratio) else math.inf


def sweep_level0(export_chunk, f1, f2, B, NQ, rows, algo, rel_tol):
    """The dense level-0 leg: max level0_ratio over every chunk; export_chunk(q0, q1) returns the
    row-major levels of flat queries [q0, q1) (a list, level 0 first).  Also checks levels >= 1
    bit for bit against pool_restated of the level below.  Returns (ratio, pooled_ok)."""
    worst, pooled = 0.0, True
    N = f2.shape[2]
    for c in chunks(B, NQ, rows):
        q0, q1 = flat_range(c, NQ)
        lv = export_chunk(q0, q1)
        ratio = level0_ratio(lv[0].reshape(c[1] - c[0], -1, N), f1, f2, c, algo, rel_tol)
        if not ratio <= worst:  # a NaN ratio stays (max() would drop it)
            worst = ratio
        for l in range(1, len(lv)):
            pooled = pooled and same_bits(pool_restated(lv[l - 1]), lv[l])
    return worst, pooled


def sweep_relocated(B, NQ, rows, big_slice, small_run):
    """The relocation leg: for every chunk of flat queries, small_run(q0, q1) (the same entry point
    on a fresh copy of the chunk's inputs) must give the bits of big_slice(q0, q1) (that chunk of
    the big call's result); both return a tensor or a list of tensors.  Returns the chunks that
    differ, as (q0, q1, index in the list)."""
    bad = []
    for c in chunks(B, NQ, rows):
        q0, q1 = flat_range(c, NQ)
        big, small = big_slice(q0, q1), small_run(q0, q1)
        if isinstance(big, torch.Tensor):
            big, small = [big], [small]
        for k, (x, y) in enumerate(zip(big, small)):
            if not same_bits(x.reshape(-1), y.reshape(-1)):
                bad.append((q0, q1, k))
    return bad


def gemm_reference(dc_chunk, f1, f2, B, NQ, rows):
    """fp64 dF1 [B, D, NQ] and dF2 [B, D, N] of autograd of corr.py:58-60 over dC read in chunks:
    dc_chunk(q0, q1) returns rows [q0, q1) of dC as [q1 - q0, N]."""
    Dd, N = f1.shape[1], f2.shape[2]
    d1 = torch.zeros(B, Dd, NQ, dtype=torch.float64, device=f1.device)
    d2 = torch.zeros(B, Dd, N, dtype=torch.float64, device=f1.device)
    s = math.sqrt(Dd)
    for c in chunks(B, NQ, rows):
        b0, b1, r0, r1 = c
        q0, q1 = flat_range(c, NQ)
        g = dc_chunk(q0, q1).double().reshape(b1 - b0, r1 - r0, N)
        d1[b0:b1, :, r0:r1] = torch.matmul(f2[b0:b1].double(), g.transpose(1, 2)) / s
        d2[b0:b1] += torch.matmul(f1[b0:b1, :, r0:r1].double(), g) / s
    return d1, d2


def norm_rel_t(a, b):
    """_util.norm_rel on the tensors' device: max |a - b| / max |b| over finite b; the non-finite
    patterns must agree (inf otherwise)."""
    a, b = a.double().reshape(-1), b.double().reshape(-1)
    fin = torch.isfinite(b)
    if not torch.equal(torch.isfinite(a), fin):
        return math.inf
    if not bool(fin.any()):
        return 0.0
    d, s = float((a[fin] - b[fin]).abs().max()), float(b[fin].abs().max())
    return d / s if s > 0 else d


def count_nonzero_rows(dc_chunk, B, NQ, rows):
    """count_nonzero of every query row of dC, [B * NQ] int64, read in chunks."""
    out = []
    for c in chunks(B, NQ, rows):
        q0, q1 = flat_range(c, NQ)
        out.append(torch.count_nonzero(dc_chunk(q0, q1).reshape(q1 - q0, -1), dim=1))
    return torch.cat(out)


def cell_bound_sweep(a_chunk, b_chunk, m_chunk, k, B, NQ, rows):
    """_util.within_cell_bound over every word, on the device in chunks: |a - b| <= k (2^-24 M +
    2^-149) where M > 0, the same bits where M = 0, the same non-finite cells; a_chunk / b_chunk /
    m_chunk(q0, q1) return rows [q0, q1) of the two dC and of M.  Returns (ok, the largest
    |a - b| / (2^-24 M) over the finite cells with M > 0)."""
    ok, worst = True, 0.0
    for c in chunks(B, NQ, rows):
        q0, q1 = flat_range(c, NQ)
        a, b, M = (f(q0, q1).reshape(-1) for f in (a_chunk, b_chunk, m_chunk))
        fin = torch.isfinite(b)
        zero = (M == 0) & fin
        live = fin & ~zero
        nil = torch.zeros_like(a)
        ok = ok and bool(torch.equal(torch.isfinite(a), fin)) and same_bits(torch.where(fin, nil, a), torch.where(fin, nil, b))
        ok = ok and same_bits(torch.where(zero, a, nil), torch.where(zero, b, nil))
        d = torch.where(live, (a.double() - b.double()).abs_(), nil.double())  # (no masked gathers: no syncs)
        m = M.double()
        ok = ok and bool((d <= k * (2.0 ** -24 * m + 2.0 ** -149)).all())
        worst = max(worst, float(torch.where(live & (m > 0), d / (2.0 ** -24 * m).clamp_min(1e-300), nil.double()).max()))
    return ok, worst
