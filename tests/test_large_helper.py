"""CPU tests of tests/_large.py: the case table and the sampled rows of test_large_volume.py, and
its dense comparison code, which has to flag planted errors on an 18x23 volume made by the oracle."""
import math

import numpy as np
import pytest
import torch

import _large
import prng
from _large import CASES, MARKS
from _util import REL_TOL
from oracle import oracle


@pytest.mark.parametrize("case", list(CASES))
def test_sample_has_both_sides_of_every_mark(case):
    c = CASES[case]
    NQ = c["H"] * c["W"]
    sample = set(_large.case_sample(case).tolist())
    assert {0, 1, c["B"] * NQ - 2, c["B"] * NQ - 1} <= sample
    assert 100 <= len(sample) <= 500
    seen = 0
    for tiled in (True, False):
        for w, total in zip(_large.row_words(c["H"], c["W"], c["L"], tiled), _large.level_words(case, tiled)):
            for m in MARKS:
                if m < total:
                    seen += 1
                    lo, hi = (m - 1) // w, m // w
                    assert lo * w <= m - 1 < (lo + 1) * w and hi * w <= m < (hi + 1) * w
                    assert {lo - 1, lo, hi, hi + 1} <= sample, (tiled, w, m)
    assert seen >= 6  # three marks in level 0 of either layout at the least
    if c["B"] > 1:  # the batch boundary nearest each mark: the last query of an item, the first of the next
        for tiled in (True, False):
            for w, total in zip(_large.row_words(c["H"], c["W"], c["L"], tiled), _large.level_words(case, tiled)):
                for m in MARKS:
                    if m < total:
                        row = m // w
                        b = min(range(1, c["B"]), key=lambda bb: abs(bb * NQ - row))
                        assert {b * NQ - 1, b * NQ} <= sample, (tiled, w, m, b)


def test_case_table_matches_map_floats():
    from eraft_amd import _lib
    for h in range(1, 40):
        for w in range(1, 40):
            assert _large.map_floats(h, w) == _lib.map_floats(h, w)
    log2 = {"one-map": 31.05, "many-maps": 31.10, "tiny-maps": 31.01, "past-2^32": 32.03}
    gb = {"one-map": 8.9, "many-maps": 9.2, "tiny-maps": 8.7, "past-2^32": 17.5}
    for case, c in CASES.items():
        words = _large.level_words(case, True)
        assert words[0] == c["B"] * c["H"] * c["W"] * _lib.map_floats(c["H"], c["W"])
        assert abs(math.log2(words[0]) - log2[case]) < 0.006, (case, math.log2(words[0]))
        assert abs(words[0] * 4 / 1e9 - gb[case]) < 0.06, (case, words[0] * 4 / 1e9)
        for l, m in c["crosses"].items():
            assert m < words[l] and (2 * m >= words[l] or m == MARKS[-1]), (case, l)
        # the row-major gradient level 0 crosses the same mark as the tiled one
        assert _large.level_words(case, False)[0] > c["crosses"][0]
        assert c["B"] * c["H"] * c["W"] < 2 ** 31 and c["H"] * c["W"] <= 2 ** 30  # what the API accepts
    c = CASES["many-maps"]
    assert c["B"] * c["H"] * c["W"] >= 18000 and c["H"] * c["W"] > 2048      # QB 32, TIGHT
    c = CASES["tiny-maps"]
    assert c["B"] * c["H"] * c["W"] >= 20000 and c["H"] * c["W"] <= 2048     # QB 16
    c = CASES["past-2^32"]  # pool_bwd_kernel<size_t>: the pooled region of level 0 holds 2^32 cells
    assert c["H"] * c["W"] * (2 * (c["H"] // 2)) * (2 * (c["W"] // 2)) >= 2 ** 32


def test_workspace_sizes_past_2_31_bytes_reach_python_whole():
    """The f16x3 corr_backward workspace of one-map and many-maps is more than 2^31 bytes: the
    binding must type every size-returning export as size_t (typed as int, 2,176,252,184 bytes came
    back negative and _lib.backward passed a 4-byte workspace, which the library refused)."""
    import ctypes
    from eraft_amd import _lib
    lib = _lib.load()
    for name in _lib.EXPORTS:
        if name.endswith(("_workspace", "_bytes")) or name == "corr_map_floats":
            assert getattr(lib, name).restype is ctypes.c_size_t, name
    for case in ("one-map", "many-maps"):
        c = CASES[case]
        N = c["H"] * c["W"]
        need = lib.corr_backward_workspace(_lib.BUILD_F16X3, c["B"], _large.D, N, c["H"], c["W"], c["r"])
        assert 2 ** 31 < need < 2 ** 33, (case, need)
        assert need >= lib.corr_build_bwd_ex_workspace(_lib.BUILD_F16X3, c["B"], _large.D, N, c["H"], c["W"])
    # the other algorithms' sizes are unchanged by the flag bits and stay positive
    c = CASES["past-2^32"]
    assert 0 < lib.corr_backward_workspace(_lib.BUILD_BF16X6, 1, _large.D, c["H"] * c["W"], c["H"], c["W"], 4) < 2 ** 40


def test_chunks_cover_once():
    for B, NQ, rows in ((1, 414, 100), (3, 414, 1000), (5, 7, 14), (4, 10, 3), (2, 5, 5)):
        seen = np.zeros(B * NQ, int)
        for c in _large.chunks(B, NQ, rows):
            q0, q1 = _large.flat_range(c, NQ)
            assert q1 - q0 == (c[1] - c[0]) * (c[3] - c[2]) or c[1] - c[0] == 1
            seen[q0:q1] += 1
        assert (seen == 1).all()


@pytest.mark.parametrize("shape", [(5, 1, 17, 23), (3, 1, 9, 6), (2, 1, 2, 3)])
def test_pool_restatement_is_the_oracle(shape):
    x = prng.gauss(41, shape) * (10.0 ** (6 * prng.uniform(42, shape) - 3)).astype(np.float32)
    ref = oracle.avg_pool2x2(x)
    got = _large.pool_restated(torch.from_numpy(x))
    assert got.dtype == torch.float32 and tuple(got.shape) == ref.shape
    assert _large.same_bits(got, torch.from_numpy(ref))
    assert not _large.same_bits(got, torch.from_numpy(ref) * (1 + 2.0 ** -23))


def _small_volume():
    B, H, W, L, r = 2, 18, 23, 3, 4
    f1, f2 = prng.gauss(51, (B, _large.D, H, W)), prng.gauss(52, (B, _large.D, H, W))
    pyr = [torch.from_numpy(p) for p in oracle.build_pyramid(f1, f2, L)]
    t1 = torch.from_numpy(f1).reshape(B, _large.D, H * W)
    t2 = torch.from_numpy(f2).reshape(B, _large.D, H * W)
    return B, H, W, L, r, t1, t2, pyr


@pytest.mark.parametrize("algo", ["bf16x6", "fp32"])
@pytest.mark.parametrize("rows", [100, 1000])
def test_level0_sweep_flags_planted_errors(algo, rows):
    B, H, W, L, r, t1, t2, pyr = _small_volume()
    NQ = H * W

    def sweep(levels):
        return _large.sweep_level0(lambda q0, q1: [p[q0:q1] for p in levels], t1, t2, B, NQ, rows, algo, REL_TOL)

    ratio, pooled = sweep(pyr)
    assert ratio <= 1 and pooled, ratio
    word = [p.clone() for p in pyr]      # a word stored one place to the side
    word[0][NQ + 37, 0, 5, 8] = word[0][NQ + 37, 0, 5, 7]
    swap = [p.clone() for p in pyr]      # two query rows of level 0 exchanged
    swap[0][[200, 201]] = swap[0][[201, 200]]
    ratio_w, pooled_w = sweep(word)
    ratio_s, pooled_s = sweep(swap)
    assert ratio_w > 1 and not pooled_w, ratio_w
    assert ratio_s > 1 and not pooled_s, ratio_s
    nan = [p.clone() for p in pyr]       # a word no store reached, pooled into the levels above as the build would
    nan[0][NQ + 37, 0, 5, 8] = float("nan")
    for l in (1, 2):
        nan[l] = _large.pool_restated(nan[l - 1])
    ratio_n, pooled_n = sweep(nan)
    assert ratio_n == math.inf and pooled_n
    inf = [p.clone() for p in pyr]
    inf[0][3, 0, 0, 0] = float("inf")
    assert sweep(inf)[0] == math.inf
    low = [p.clone() for p in pyr]       # a wrong word in a pooled level only
    low[2][5, 0, 1, 2] *= 1 + 2.0 ** -23
    ratio_l, pooled_l = sweep(low)
    assert ratio_l <= 1 and not pooled_l


def test_relocation_sweep_flags_planted_errors():
    B, H, W, L, r, t1, t2, pyr = _small_volume()
    NQ = H * W
    pn = [p.numpy() for p in pyr]
    coords = prng.lookup_coords(53, B, H, W, 3.0)
    big = torch.from_numpy(oracle.lookup(pn, coords, r)).permute(1, 0, 2, 3).reshape(-1, B * NQ)
    cf = coords.transpose(1, 0, 2, 3).reshape(2, B * NQ)

    def small_run(q0, q1):
        out = oracle.lookup_rows([p[q0:q1] for p in pn], cf[None, :, q0:q1, None], H, W, r)
        return torch.from_numpy(out).reshape(-1, q1 - q0)

    def sweep(res):
        return _large.sweep_relocated(B, NQ, 100, lambda q0, q1: res[:, q0:q1], small_run)

    assert sweep(big) == []
    word = big.clone()
    word[17, 430] = word[17, 431]
    assert sweep(word) == [(414 + 0, 414 + 100, 0)]
    swap = big.clone()
    swap[:, [99, 100]] = swap[:, [100, 99]]
    assert sweep(swap) == [(0, 100, 0), (100, 200, 0)]


def test_untouched_cell_count_flags_a_stray_store():
    B, H, W, L, r, t1, t2, pyr = _small_volume()
    NQ, K = H * W, 81
    coords = prng.lookup_coords(54, B, H, W, 3.0)
    touched = np.array([0, 5, NQ - 1, NQ, 2 * NQ - 1])
    g = np.zeros((B, L * K, NQ), np.float32)
    for q in touched:
        g[q // NQ, :, q % NQ] = prng.gauss(55 + int(q), (L * K,))
    gp = [np.zeros((B * NQ, 1, h, w), np.float32) for h, w in oracle.level_shapes(H, W, L)]
    oracle.lookup_bwd(coords, g.reshape(B, L * K, H, W), gp, r)
    oracle.pool_bwd(gp, H, W)
    dc = torch.from_numpy(gp[0])
    counts = _large.count_nonzero_rows(lambda q0, q1: dc[q0:q1], B, NQ, 100)
    assert int(counts.sum()) == int(counts[touched].sum()) > 0
    dc[300, 0, 4, 4] = 1e-30  # a store into a row that no gradient reaches
    counts = _large.count_nonzero_rows(lambda q0, q1: dc[q0:q1], B, NQ, 100)
    assert int(counts.sum()) == int(counts[touched].sum()) + 1


def test_cell_bound_sweep_is_within_cell_bound():
    from _util import cell_bound_k, within_cell_bound
    n, k = 400, cell_bound_k(1, 4)
    M = np.abs(prng.gauss(58, (n, 50))).astype(np.float32)
    M[::7] = 0
    b = (prng.gauss(59, (n, 50)) * M).astype(np.float32)
    a = (b.astype(np.float64) + 0.4 * k * 2.0 ** -24 * M * prng.gauss(60, (n, 50)).clip(-2, 2)).astype(np.float32)
    a[M == 0] = b[M == 0] = 0.0  # (not the -0.0 of a negative draw times 0)
    b[5, 5] = a[5, 5] = np.inf

    def sweep(x):
        t = [torch.from_numpy(v) for v in (x, b, M)]
        return _large.cell_bound_sweep(*[lambda q0, q1, v=v: v[q0:q1] for v in t], k, 2, n // 2, 60)

    ok, worst = sweep(a)
    assert ok and within_cell_bound(a, b, M, 1, 4) and 0 < worst <= k
    for i, j, v in ((9, 3, None), (7, 2, 1e-30), (5, 5, 1.0)):  # past the bound; a store where M = 0; a lost inf
        x = a.copy()
        x[i, j] = b[i, j] + 3 * k * 2.0 ** -24 * M[i, j] if v is None else v
        assert not sweep(x)[0] and not within_cell_bound(x, b, M, 1, 4), (i, j)


def test_gemm_reference_and_norm_rel():
    B, H, W, L, r, t1, t2, pyr = _small_volume()
    NQ = H * W
    gc = prng.gauss(56, (B * NQ, NQ))
    d1, d2 = oracle.corr_bwd(gc.reshape(B * NQ, 1, H, W), t1.numpy().reshape(B, -1, H, W), t2.numpy().reshape(B, -1, H, W))
    g = torch.from_numpy(gc)
    for rows in (100, 1000):
        r1, r2 = _large.gemm_reference(lambda q0, q1: g[q0:q1], t1, t2, B, NQ, rows)
        assert _large.norm_rel_t(torch.from_numpy(d1), r1.reshape(d1.shape)) < 1e-6
        assert _large.norm_rel_t(torch.from_numpy(d2), r2.reshape(d2.shape)) < 1e-6
    bad = g.clone()
    bad[[3, 4]] = bad[[4, 3]]
    r1, r2 = _large.gemm_reference(lambda q0, q1: bad[q0:q1], t1, t2, B, NQ, 100)
    assert _large.norm_rel_t(torch.from_numpy(d1), r1.reshape(d1.shape)) > REL_TOL
    assert _large.norm_rel_t(torch.tensor([1.0, math.inf]), torch.tensor([1.0, 2.0])) == math.inf


def test_planted_coords_hold_every_family():
    c = CASES["many-maps"]
    sample = _large.case_sample("many-maps")
    coords = _large.plant_coords(prng.lookup_coords(57, c["B"], c["H"], c["W"], 3.0), sample)
    flat = coords.reshape(c["B"], 2, -1)
    picked = np.stack([flat[q // flat.shape[2], :, q % flat.shape[2]] for q in sample])
    assert np.isnan(picked).any() and np.isinf(picked).any()
    assert (picked == 1e4).any() and (picked == -0.5).any()          # special_coords' values
    grid = (picked == np.round(picked)).all(axis=1) & np.isfinite(picked).all(axis=1)
    assert grid.sum() >= len(sample) // 4
    rest = np.ones(c["B"] * flat.shape[2], bool)
    rest[sample] = False
    assert np.isfinite(flat.transpose(0, 2, 1).reshape(-1, 2)[rest]).all()
