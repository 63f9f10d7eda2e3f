"""The two voxel-grid kernels (csrc/corr_voxel.hip) where the bulk fixtures do not reach:
degenerate time windows, NaN / inf / beyond-int32 coordinates, corners and bins just outside the
grid, odd polarities, wrapped MVSEC indices, each branch of the normalisation, and a grid large
enough that the scan of the tile sums takes two values per thread.

tests/golden/g_voxel_edges.npz holds the reference's own answers (make_golden.py
case_voxel_edges); where the reference refuses the input, or the grid is too large to store,
the checker is the oracle, which tests/test_oracle.py pins to that fixture bit for bit.
"""
import types

import numpy as np
import pytest
import torch

import prng
from _util import bit_equal, load, voxel_edge_cases, voxel_norm_within_bar
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
G = load("g_voxel_edges")


def _dsec(ev, C, H, W, normalize):
    from eraft_amd import VoxelGrid
    evt = {k: torch.from_numpy(np.ascontiguousarray(ev[i])).to(DEV) for i, k in enumerate("xytp")}
    return VoxelGrid((C, H, W), normalize=normalize).convert(evt).cpu().numpy()


def _mvsec(ev, C, H, W, normalize):
    from eraft_amd import EventSequenceToVoxelGrid
    seq = types.SimpleNamespace(features=ev, image_width=W, image_height=H)
    return EventSequenceToVoxelGrid(C, normalize=normalize)(seq).cpu().numpy()


def _check_case(run, kind, tag):
    M, C, H, W = (int(v) for v in G[f"{kind}_meta_{tag}"])
    ev, ref_raw, ref_nrm = G[f"{kind}_ev_{tag}"], G[f"{kind}_raw_{tag}"], G[f"{kind}_norm_{tag}"]
    raw = run(ev, C, H, W, False)
    print(f"{kind}/{tag}: raw nonzero {np.count_nonzero(raw)} (ref {np.count_nonzero(ref_raw)}), "
          f"NaN {int(np.isnan(raw).sum())} (ref {int(np.isnan(ref_raw).sum())})")
    assert bit_equal(raw, ref_raw)
    nrm = run(ev, C, H, W, True)
    assert voxel_norm_within_bar(nrm, ref_nrm)
    if tag in ("one_cell", "equal_cells"):
        assert ref_raw.any() and not nrm.any()
    assert bit_equal(run(ev, C, H, W, False), raw) and bit_equal(run(ev, C, H, W, True), nrm)


@pytest.mark.parametrize("tag", voxel_edge_cases(G, "d"))
def test_voxel_grid_edge_case_vs_reference_golden(tag):
    """corr_voxel_grid through the drop-in VoxelGrid on one case of g_voxel_edges: raw grid
    bit-identical to the reference, normalised grid within 1e-6 of max|v| with the reference's
    zero and NaN pattern (exactly zero for one_cell / equal_cells), repeat runs identical."""
    _check_case(_dsec, "d", tag)


@pytest.mark.parametrize("tag", voxel_edge_cases(G, "m"))
def test_voxel_grid_tbilinear_edge_case_vs_reference_golden(tag):
    """corr_voxel_grid_tbilinear through the drop-in EventSequenceToVoxelGrid: same bars."""
    _check_case(_mvsec, "m", tag)


def test_voxel_grid_empty_window_is_zero():
    """DSEC with M = 0 (the reference indexes t[0] and raises): zeros over a pre-filled out,
    raw and normalised, as the oracle."""
    from eraft_amd import _lib
    C, H, W = 5, 6, 8
    e = torch.empty(0, dtype=torch.float32, device=DEV)
    for normalize in (False, True):
        o = torch.full((C, H, W), 7.0, device=DEV)
        _lib.voxel_grid(e, e, e, e, o, normalize)
        got = o.cpu().numpy()
        assert not got.any()
        assert bit_equal(got, oracle.voxel_grid(np.empty((4, 0), np.float32), C, H, W, normalize))


def test_voxel_grid_tbilinear_drops_what_the_reference_refuses():
    """MVSEC events with a NaN or +-inf x or y, or a flat index outside the grid (index_add_
    raises in the reference): kernel and oracle both drop them, so the grid is the oracle's and
    equals the grid of the remaining events (first and last stamp kept)."""
    C, H, W = 5, 6, 8
    nan, inf = np.nan, np.inf
    good = [(0.0, 1, 1, 1), (90.0, 2, 3, 0), (130.0, 2, 3, 1), (210.0, 7, 5, 1), (330.0, 0, 0, 0), (400.0, 3, 5, 1)]
    bad = [(50.0, nan, 3, 1), (100.0, 2, nan, 1), (150.0, inf, 3, 0), (180.0, -inf, 3, 1), (200.0, 2, inf, 1),
           (220.0, 2, -inf, 0), (10.0, -60, 0, 1),      # row 0: flat indices -60 (bin 0) and -12 (bin 1)
           (390.0, 1, H + 2, 1),                        # left vote in bin 3 lands inside bin 4, the right one beyond
           (400.0, 0, H, 1),                            # last bin, row H: one past the end
           (250.0, 1e300, 1, 1), (260.0, 1, -1e300, 0), (270.0, 3e9, 1, 1), (280.0, 9.3e18, 0, 1)]
    rows = [good[0]]
    for k, b in enumerate(bad):
        rows.append(b)
        rows.append(good[1 + k % 4])
    rows.append(good[-1])
    ev = np.ascontiguousarray(np.array(rows, np.float64))
    keep = np.ascontiguousarray(np.array([r for r in rows if r not in bad or r[0] == 390.0], np.float64))
    for normalize in (False, True):
        ref = oracle.voxel_grid_tbilinear(ev, C, H, W, normalize)
        assert np.isfinite(ref).all()
        got = _mvsec(ev, C, H, W, normalize)
        assert bit_equal(got, ref)
        only = oracle.voxel_grid_tbilinear(keep, C, H, W, normalize)
        assert bit_equal(ref, only)


# A grid just over 2^23 cells that is no multiple of the scan's 8192-cell tile: 1026 tiles, so
# the one-workgroup scan of the tile sums takes two per thread (the carry crosses threads at
# tiles 511/512 and 1023/1024, thread 513 onward is clipped) and the last tile has 200 cells.
BIG = (9, 1000, 933)
TILE = 8192


def _big_regions():
    n = BIG[0] * BIG[1] * BIG[2]
    tiles = -(-n // TILE)
    assert n > 1 << 23 and n % TILE and tiles == 1026 and -(-tiles // 1024) == 2
    b1, b2, last = 512 * TILE, 1024 * TILE, (tiles - 1) * TILE
    return n, {"first_tile": [0, 5, TILE - 1], "tiles_511_512": [b1 - 1, b1], "tiles_1023_1024": [b2 - 1, b2],
               "last_tile": [last, n - 1]}


def _big_dsec_events():
    """About 20 000 events over the whole grid (stamps past the last one reach the last bin),
    a few hundred of them forced onto the regions of _big_regions and onto one hot pixel."""
    C, H, W = BIG
    M = 20000
    u = prng.uniform(91, (4, M))
    x = (u[0] * (W + 2) - 1.0).astype(np.float32)
    y = (u[1] * (H + 2) - 1.0).astype(np.float32)
    t = (u[2] * 1.12).astype(np.float32)
    p = (u[3] > 0.5).astype(np.float32)
    _, regions = _big_regions()
    k = 100
    for cells in regions.values():
        for c in cells:
            tl, yl, xl = c // (H * W), (c % (H * W)) // W, c % W
            for j in range(30):                     # base corner on the cell, varied fractions
                x[k] = xl + (0.0, 0.25, 0.5)[j % 3]
                y[k] = yl + (0.0, 0.375)[j % 2]
                t[k] = (tl + 0.03125 * (j % 8)) / (C - 1)
                p[k] = 1.0
                k += 7
    x[3000:6000:10], y[3000:6000:10] = 100.25, 200.5   # 300 events on one pixel: long buckets
    t[0], t[-1] = 0.0, 1.0
    return np.stack([x, y, t, p])


def _big_mvsec_events():
    C, H, W = BIG
    M = 20000
    u = prng.uniform(92, (4, M)).astype(np.float64)
    t = np.sort(u[2] * 50000.0)
    t[0], t[-1] = 0.0, 50000.0
    ev = np.stack([t, np.floor(u[0] * W), np.floor(u[1] * H), (u[3] > 0.5).astype(np.float64)], 1)
    _, regions = _big_regions()
    k = 100
    for cells in regions.values():
        for c in cells:
            tl, yl, xl = c // (H * W), (c % (H * W)) // W, c % W
            for j in range(30):                     # bin tl by the left vote, or by the right one of bin tl - 1
                b = tl if (j % 2 == 0 and tl < C - 1) or tl == 0 else tl - 1
                ev[k] = ((b + 0.25 + 0.0625 * (j % 4)) * 50000.0 / (C - 1), xl, yl, 1.0)
                k += 7
    ev[3000:6000:10, 1:3] = (100.0, 200.0)
    return np.ascontiguousarray(ev)


def _assert_regions_populated(ref):
    n, regions = _big_regions()
    flat = ref.reshape(-1)
    assert flat.size == n
    for name, cells in regions.items():
        for c in cells:
            assert flat[c] != 0.0, (name, c)
    assert np.count_nonzero(flat[:TILE]) >= 3 and np.count_nonzero(flat[(n // TILE) * TILE:]) >= 2
    assert np.count_nonzero(flat) > 20000


def test_voxel_grid_large_grid_vs_oracle():
    """DSEC entry point on the 9 x 1000 x 933 grid: the oracle's grid is populated in the first
    tile, either side of both thread boundaries of the tile-sum scan, in the last partial tile
    and on the hot pixel; the raw grid is bit-identical to it, a repeat run is identical, the
    normalised grid is within 1e-6 of max|v|."""
    C, H, W = BIG
    ev = _big_dsec_events()
    ref = oracle.voxel_grid(ev, C, H, W, False)
    _assert_regions_populated(ref)
    assert np.count_nonzero(ref[:, 200:202, 100:102]) >= 4 * (C - 1)
    raw = _dsec(ev, C, H, W, False)
    assert bit_equal(raw, ref)
    assert bit_equal(_dsec(ev, C, H, W, False), raw)
    nref = oracle.voxel_grid(ev, C, H, W, True)
    assert voxel_norm_within_bar(_dsec(ev, C, H, W, True), nref)


def test_voxel_grid_tbilinear_large_grid_vs_oracle():
    """The same grid once through the MVSEC entry point: bit-identical to the oracle."""
    C, H, W = BIG
    ev = _big_mvsec_events()
    ref = oracle.voxel_grid_tbilinear(ev, C, H, W, False)
    _assert_regions_populated(ref)
    assert bit_equal(_mvsec(ev, C, H, W, False), ref)
