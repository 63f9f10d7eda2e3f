"""The lookup's window gather (corr_lookup_block.h gather_window_tiled) at the smallest shapes where
each of its paths can go wrong: windows larger than the map, a 1x1 level, ragged tile columns,
partial last blocks, every window size (more than one load per lane and query from r = 6), the
TIGHT gather (>= 18,000 queries), 16 queries per workgroup, and a row slab of queries.  Every
comparison is bit-exact against the oracle on the kernel's own exported pyramid (D = 8: the build
costs nothing).  Run on the GPU box: pytest -m gpu.
"""
import functools

import numpy as np
import pytest
import torch

import prng
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


def _sprinkled(B, H, W):
    """A sigma = 3 flow with NaN, +-inf and huge coordinates over 64 entries."""
    c = prng.lookup_coords(314, B, H, W, 3.0)
    flat = c.reshape(-1)
    idx = (prng.uniform(315, (64,)) * flat.size).astype(np.int64)
    flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 3.0e38, -1e30, 1e6, -0.0, 2.0 ** 20], np.float32), 64)
    return c


FAMILIES = {
    "sigma0": lambda B, H, W: prng.lookup_coords(311, B, H, W, 0.0),
    "sigma4": lambda B, H, W: prng.lookup_coords(312, B, H, W, 4.0),
    "sigma25": lambda B, H, W: prng.lookup_coords(313, B, H, W, 25.0),
    "grid": prng.coords_grid,
    "special": prng.special_coords,
    "sprinkled": _sprinkled,
}

SHAPES = [
    (1, 8, 8, 4, 4),      # a 1x1 level; windows larger than every map
    (3, 12, 20, 4, 4),    # level widths 20, 10, 5, 2: ragged tile columns; 240 queries: a partial last block
    (1, 17, 23, 3, 2),    # odd sizes: map rows and widths not multiples of 4
    (2, 9, 13, 2, 1),
    (1, 16, 24, 3, 0),    # every other window size ...
    (1, 16, 24, 3, 1),
    (1, 16, 24, 3, 2),
    (1, 16, 24, 3, 3),
    (1, 16, 24, 3, 5),
    (1, 16, 24, 3, 6),    # ... from here more than one load per lane and query
    (1, 16, 24, 3, 7),
    (8, 48, 48, 4, 4),    # 18,432 queries: the TIGHT gather
    (10, 45, 45, 4, 4),   # 20,250 queries on a map of 2,025 cells: 16 queries per workgroup
]


@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("B,H,W,L,r", SHAPES)
def test_lookup_gather_vs_oracle(B, H, W, L, r, family):
    cb, pyr = _block(B, H, W, L, r)
    c = FAMILIES[family](B, H, W)
    out = cb(torch.from_numpy(c).to(DEV)).cpu().numpy()
    assert bit_equal(out, oracle.lookup(pyr, c, r))


@pytest.mark.parametrize("family", list(FAMILIES))
def test_lookup_gather_row_slab(family):
    """Query rows 4..11 of a 16 x 24 map, looked up from a pyramid built for those rows only:
    bit-equal to the same rows of the full lookup."""
    from eraft_amd import _lib
    from eraft_amd.sharded import HipRows
    B, H, W, L, r = 2, 16, 24, 4, 4
    h0, h1 = 4, 12
    K = (2 * r + 1) ** 2
    cb, pyr = _block(B, H, W, L, r)
    c = FAMILIES[family](B, H, W)
    ct = torch.from_numpy(c).to(DEV)
    full = cb(ct).cpu().numpy()
    assert bit_equal(full, oracle.lookup(pyr, c, r))
    f1 = torch.from_numpy(prng.gauss(301, (B, D, H, W))).to(DEV)
    f2 = torch.from_numpy(prng.gauss(302, (B, D, H, W))).to(DEV)
    levels_rows = HipRows.build(f1[:, :, h0:h1].contiguous(), f2, L)
    out = torch.empty(B, L * K, h1 - h0, W, device=DEV)
    _lib.lookup(levels_rows, ct[:, :, h0:h1].contiguous(), r, out, H, W)
    assert bit_equal(out.cpu().numpy(), full[:, :, h0:h1])
