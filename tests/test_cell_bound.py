"""CPU tests of the per-cell bound that the lookup-backward tests use (tests/_util.py:
cell_magnitude, within_cell_bound) and of oracle.lookup_bwd_rows.

norm_rel is max|a - b| / max|b| over the whole of dC, whose per-cell magnitude spans many decades:
a cell that a fold gets entirely wrong passes a 1e-6 norm-relative test whenever its magnitude is
below 1e-6 of the largest cell.  within_cell_bound scales the tolerance of every cell by
M = sum |contribution| of that cell, and these tests show that it notices what norm_rel cannot.
"""
import functools

import numpy as np
import pytest

import prng
from _coords import FAMILIES, _ulps, family_bwd_case
from _util import bit_equal, cell_bound_k, cell_magnitude, cell_ratio, norm_rel, within_cell_bound
from oracle import oracle

SHAPES = [(3, 12, 20, 4, 4), (1, 8, 8, 4, 4), (1, 17, 23, 3, 4), (2, 36, 48, 4, 4)]


def _zero_pyramid(BN, H, W, L):
    return [np.zeros((BN, 1, h, w), np.float32) for h, w in oracle.level_shapes(H, W, L)]


def _oracle_dc(cs, gs, H, W, L, r):
    gp = _zero_pyramid(cs[0].shape[0] * H * W, H, W, L)
    for c, g in zip(cs, gs):
        oracle.lookup_bwd(c, g, gp, r)
    return oracle.pool_bwd(gp, H, W)[0]


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("B,H,W,L,r", SHAPES)
def test_cell_magnitude_bounds_the_oracle(B, H, W, L, r, family):
    """M is finite and non-negative (NaN and infinite coordinates contribute nothing), bounds |dC|
    in every cell, and dC is exactly 0 wherever M is 0."""
    cs, gs = family_bwd_case(family, B, H, W, L, r)
    dc = _oracle_dc(cs, gs, H, W, L, r)
    M = cell_magnitude(cs, gs, H, W, L, r)
    assert M.shape == dc.shape and np.isfinite(M).all() and (M >= 0).all()
    assert np.isfinite(dc).all()
    # fp32 sums of the same terms in the same order: |sum| <= sum of |terms| holds for the rounded sums too
    assert (np.abs(dc) <= M).all()
    untouched = M == 0
    assert (dc.view(np.uint32)[untouched] == 0).all()
    print(f"{family} {(B, H, W, L, r)}: {untouched.mean():.1%} of cells untouched, "
          f"M spans {M[~untouched].min() / M.max():.1e}")
    assert (~untouched).any()


@functools.lru_cache(maxsize=1)
def _planted_case():
    B, H, W, L, r, T = 2, 36, 48, 4, 4, 3
    cs = [FAMILIES["sigma4"](B, H, W)] + [prng.lookup_coords(420 + t, B, H, W, 4.0) for t in range(1, T)]
    gs = [prng.gauss(430 + t, (B, L * (2 * r + 1) ** 2, H, W)) for t in range(T)]
    dc = _oracle_dc(cs, gs, H, W, L, r)
    M = cell_magnitude(cs, gs, H, W, L, r)
    for a in (dc, M):
        a.setflags(write=False)
    return dc, M, T, L


def _small_cell(dc, M):
    """The flat index of a cell with 0 < M < 1e-7 max M whose value is a large part of its M."""
    d, m = dc.reshape(-1), M.reshape(-1).astype(np.float64)
    small = (m > 0) & (m < 1e-7 * m.max())
    assert small.any()
    part = np.where(small, np.abs(d) / np.where(small, m, 1.0), 0.0)
    i = int(part.argmax())
    assert part[i] > 0.1, part[i]      # far above k * 2^-24 = 1.4e-5
    return i


@pytest.mark.parametrize("plant", ["lost", "moved"])
def test_within_cell_bound_sees_what_norm_rel_misses(plant):
    """A contribution lost (the cell zeroed) or put into the neighbouring cell, in a cell below
    1e-7 of the largest: the norm-relative metric stays within 1e-6, the per-cell bound fails."""
    dc, M, T, L = _planted_case()
    i = _small_cell(dc, M)
    bad = dc.copy().reshape(-1)
    if plant == "moved":
        j = i + 1 if (i + 1) % dc.shape[-1] else i - 1     # the neighbour in the same row
        bad[j] += bad[i]
    bad[i] = 0.0
    bad = bad.reshape(dc.shape)
    assert not bit_equal(bad, dc)
    e = norm_rel(bad, dc)
    print(f"planted |v| = {abs(float(dc.reshape(-1)[i])):.3e}, M = {float(M.reshape(-1)[i]):.3e}, "
          f"max M = {float(M.max()):.3e}: norm_rel {e:.2e}, cell ratio {cell_ratio(bad, dc, M):.3e}")
    assert e <= 1e-6
    assert not within_cell_bound(bad, dc, M, T, L)
    assert cell_ratio(bad, dc, M) > cell_bound_k(T, L)


def test_within_cell_bound_accepts_rounding():
    """dC passes against itself and against a copy with every value moved one ulp; an untouched
    cell (M = 0) that is not exactly equal fails, and so does another non-finite pattern."""
    dc, M, T, L = _planted_case()
    assert within_cell_bound(dc, dc, M, T, L)
    assert cell_ratio(dc, dc, M) == 0.0
    touched = (M > 0) & (dc != 0)
    for u in (1, -1):
        moved = np.where(touched, _ulps(dc, np.where(touched, u, 0)), dc)
        assert (moved != dc).sum() == touched.sum()
        assert within_cell_bound(moved, dc, M, T, L)
        assert cell_ratio(moved, dc, M) <= 2.0      # one ulp of |dC| <= M is at most 2^-23 M
    i = int(np.flatnonzero(M.reshape(-1) == 0)[0])
    for v in (np.float32(1e-45), np.float32(-0.0), np.float32(np.nan), np.float32(np.inf)):
        bad = dc.copy().reshape(-1)
        bad[i] = v
        assert not within_cell_bound(bad.reshape(dc.shape), dc, M, T, L), v
    j = int(M.argmax())
    bad = dc.copy().reshape(-1)
    bad[j] = np.inf
    assert not within_cell_bound(bad.reshape(dc.shape), dc, M, T, L)


@pytest.mark.parametrize("family", ["near_integer", "special", "sprinkled"])
@pytest.mark.parametrize("B,H,W,L,r", [(1, 17, 23, 3, 4), (2, 17, 20, 4, 4), (1, 16, 24, 3, 1)])
def test_oracle_lookup_bwd_rows(B, H, W, L, r, family):
    """oracle.lookup_bwd_rows on the full slab equals oracle.lookup_bwd bit for bit, and on the
    rows [h0, h1) it equals the corresponding queries of the full result."""
    cs, gs = family_bwd_case(family, B, H, W, L, r)
    full = _zero_pyramid(B * H * W, H, W, L)
    rows = _zero_pyramid(B * H * W, H, W, L)
    for c, g in zip(cs, gs):
        oracle.lookup_bwd(c, g, full, r)
        oracle.lookup_bwd_rows(c, g, rows, H, W, r)
    assert any(p.any() for p in full)
    for l in range(L):
        assert bit_equal(rows[l], full[l]), l
    for h0, h1 in ((3, 8), (0, 1), (H - 1, H), (8, H)):
        NQ = (h1 - h0) * W
        slab = _zero_pyramid(B * NQ, H, W, L)
        for c, g in zip(cs, gs):
            oracle.lookup_bwd_rows(c[:, :, h0:h1], g[:, :, h0:h1], slab, H, W, r)
        for l in range(L):
            want = full[l].reshape(B, H * W, H >> l, W >> l)[:, h0 * W:h1 * W]
            assert bit_equal(slab[l].reshape(want.shape), want), (h0, h1, l)
