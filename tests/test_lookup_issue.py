"""The lookup kernel's instruction-count changes (corr_lookup_block.h: the gather's per-query words
computed once per workgroup, both axes' taps as one packed chain, the workgroup's mode flags
reduced by ballots) at the smallest shapes where each can go wrong: S = 1, 3, 9 and 15 (more
than one load per lane and query), windows larger than the maps, a 1x1 level, ragged tile columns,
a partial last block (dead queries' words), the TIGHT gather (which keeps the per-wave words)
and 16 queries per workgroup; on coordinates that flag no lane, some lanes and every lane.
Every comparison is bit-exact against the oracle on the kernel's own exported pyramid (D = 8:
the build costs nothing).  Run on the GPU box: pytest -m gpu.
"""
import functools

import numpy as np
import pytest
import torch

import prng
from _coords import FAMILIES, _near_integer
from _util import bit_equal
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
D = 8


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eraft_amd import _lib
    _lib.load()  # the HIP library must be the thing under test (no fallback exists)


@functools.lru_cache(maxsize=2)
def _block(B, H, W, L, r):
    """CorrBlock and its exported pyramid (numpy, reference layout), shared by a shape's cases."""
    from eraft_amd import CorrBlock
    f1, f2 = prng.gauss(301, (B, D, H, W)), prng.gauss(302, (B, D, H, W))
    cb = CorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    return cb, [p.cpu().numpy() for p in cb.corr_pyramid]


SHAPES = [
    (1, 8, 8, 4, 4),      # a 1x1 level; windows larger than every map
    (3, 12, 20, 4, 4),    # level widths 20, 10, 5, 2: ragged tile columns; 240 queries: a partial last block
    (1, 17, 23, 3, 2),    # odd sizes: map rows and widths not multiples of 4
    (1, 16, 24, 3, 0),    # S = 1: no tap pair at all
    (1, 16, 24, 3, 1),    # S = 3: one pair plus the scalar remainder
    (1, 16, 24, 3, 4),
    (1, 16, 24, 3, 7),    # more than one load per lane and query
    (8, 48, 48, 4, 4),    # 18,432 queries: the TIGHT gather
    (10, 45, 45, 4, 4),   # 20,250 queries on a map of 2,025 cells: 16 queries per workgroup
]


def test_near_integer_family_covers_its_cases():
    """The family holds what it promises at the shapes above: both signs of every ulp step, cells
    outside the map on both sides, and magnitudes on both sides of 2^20."""
    for B, H, W in ((1, 8, 8), (1, 16, 24), (3, 12, 20)):
        c = _near_integer(B, H, W)
        g = prng.coords_grid(B, H, W)
        d = c - g
        assert (d > 0).any() and (d < 0).any() and (np.abs(d[d != 0]).min() < 1e-6)
        assert (c[:, 0] < 0).any() and (c[:, 0] >= W).any() and (c[:, 1] < 0).any() and (c[:, 1] >= H).any()
        assert (np.abs(c) > 2.0 ** 20).any() and (np.abs(c) == 2.0 ** 20 - 1).any()
        assert np.isfinite(c).all()


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("B,H,W,L,r", SHAPES)
def test_lookup_issue_vs_oracle(B, H, W, L, r, family):
    cb, pyr = _block(B, H, W, L, r)
    c = FAMILIES[family](B, H, W)
    out = cb(torch.from_numpy(c).to(DEV)).cpu().numpy()
    assert bit_equal(out, oracle.lookup(pyr, c, r))


def test_lookup_conv_selects_the_plain_lookup():
    """lookup_conv (the same lookup_block_v, feeding the fused 1x1 convolution) with one-hot weight
    rows, no bias and no ReLU: output channel o is lookup channel sel[o] bit for bit (x = hi + mid +
    lo is exact, the pieces times 1 and the zero products add without rounding).  Two selections
    cover the 243 channels; finite coordinates and levels of at least 2 x 2, so no NaN or infinity
    meets a zero weight.  The smallest shape with a partial last block (17 x 23, 3 levels)."""
    B, H, W, L, r = 1, 17, 23, 3, 4
    C = L * (2 * r + 1) ** 2
    cb, _ = _block(B, H, W, L, r)
    c = torch.from_numpy(prng.lookup_coords(312, B, H, W, 4.0)).to(DEV)
    plain = cb(c).cpu().numpy()
    assert np.isfinite(plain).all()
    bias = torch.zeros(256, device=DEV)
    seen = np.zeros(C, bool)
    for first in (0, C - 256):
        sel = (first + np.arange(256)) % C
        w = np.zeros((256, C, 1, 1), np.float32)
        w[np.arange(256), sel] = 1.0
        out = cb.lookup_conv(c, torch.from_numpy(w).to(DEV), bias, relu=False).cpu().numpy()
        assert bit_equal(out + np.float32(0.0), plain[:, sel] + np.float32(0.0))   # (+ 0: -0 and +0 are one value)
        seen[sel] = True
    assert seen.all()


def test_ondemand_matches_the_plain_lookup():
    """OnDemandCorrBlock (tap arithmetic shared through corr_taps.h) against CorrBlock on feature
    maps of small integers with D = 16: every correlation, pooled value and product sum is an exact
    dyadic number whatever the order of summation, so both blocks interpolate the same cells with the
    same taps and must agree bit for bit.  Its smallest shape with every level at least 2 x 2."""
    from eraft_amd import CorrBlock, OnDemandCorrBlock
    B, Dm, H, W, L, r = 1, 16, 16, 24, 3, 4
    f1 = np.rint(prng.gauss(321, (B, Dm, H, W), 1.5)).astype(np.float32)
    f2 = np.rint(prng.gauss(322, (B, Dm, H, W), 1.5)).astype(np.float32)
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    for fam in ("sigma4", "near_integer"):
        c = FAMILIES[fam](B, H, W)
        c = np.where(np.abs(c) < 1e5, c, np.float32(3.5)).astype(np.float32)   # finite, in-range coordinates
        ct = torch.from_numpy(c).to(DEV)
        with torch.no_grad():
            plain = CorrBlock(t1, t2, num_levels=L, radius=r)(ct).cpu().numpy()
            od = OnDemandCorrBlock(t1, t2, num_levels=L, radius=r)(ct).cpu().numpy()
        assert np.isfinite(plain).all()
        print(f"{fam}: ondemand vs plain: {(od.view(np.uint32) != plain.view(np.uint32)).sum()} of {od.size} words differ, "
              f"max |diff| {np.abs(od - plain).max():.3e}")
        assert bit_equal(od + np.float32(0.0), plain + np.float32(0.0)), fam
