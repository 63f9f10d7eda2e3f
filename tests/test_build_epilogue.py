"""The bf16x6 build's epilogue (corr_build_bf16.hip: the accumulator merge, the lane-swap pooling
trades, the interior / edge store sections) at the smallest shapes that reach each of its paths.

Shape (B, D, H, W), D = 32      what it reaches
(1, 32, 8, 16)                  one interior patch, one full query group: the unpredicated path alone
(1, 32, 12, 16)                 the 4-row body; N = 192: a wave whose queries all lie past NQ
(2, 32, 10, 12)                 H % 4 != 0 (padded tile rows are stored), N = 120 ends inside a 16-query
                                block, tile columns past W, two batch items, H >> 3 = 1
(1, 32, 20, 24)                 two patch columns, the second half outside the map; 4-row body last
(1, 32, 16, 18)                 W % 4 != 0
(1, 32, 16, 32), 3 and 2 levels the epilogue with a runtime level count

Bounds.  Level 0: the build's documented a-priori bound (3 + 6 S) u sum_k |a_k b_k| / sqrt(D) against
an fp64 product, u = 2^-24, S = ceil(D / 32) (tests/test_gpu_parity.py::test_build_bf16x6_error_bound).
Levels 1-3 of a build with finite features are checked bit for bit against avg_pool2d of level 0.
With non-finite features the finite cells of level l are held to the bound carried through the
pools: a pool ((a + b) + c) + d) * 1/4 rounds three times (the scale is exact), so
E_l = pool(E_{l-1}) + 3 u' pool(M_{l-1} + E_{l-1}),  M_l = pool(M_{l-1}),  M_0 = sum |a b| / sqrt(D) >= |exact|,
with u' = 2^-24 (1 + 2^-20) covering the second-order terms."""
import functools

import numpy as np
import pytest
import torch

import prng
from _util import bit_equal, export_levels, tiled_levels
from oracle import oracle

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 2.0 ** -24

# (shape, levels, target-row regions of the corr_build_region check: y0 a multiple of 8)
CASES = {
    "8x16": ((1, 32, 8, 16), 4, [(0, 8)]),  # a single patch row: one region is all there is
    "12x16": ((1, 32, 12, 16), 4, [(0, 8), (8, 12)]),
    "b2_10x12": ((2, 32, 10, 12), 4, [(0, 8), (8, 10)]),
    "20x24": ((1, 32, 20, 24), 4, [(0, 8), (8, 20)]),
    "16x18": ((1, 32, 16, 18), 4, [(0, 8), (8, 16)]),
    "16x32_L3": ((1, 32, 16, 32), 3, [(0, 8), (8, 16)]),
    "16x32_L2": ((1, 32, 16, 32), 2, [(0, 8), (8, 16)]),
}


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eraft_amd import _lib
    _lib.load()


def _fp64(f1, f2):
    """The fp64 product [B, N, N] / sqrt(D) and the product of magnitudes (the bound's sum |a b|)."""
    B, D, H, W = f1.shape
    a, b = f1.reshape(B, D, H * W).astype(np.float64), f2.reshape(B, D, H * W).astype(np.float64)
    with np.errstate(invalid="ignore"):
        ref = np.einsum("bdn,bdm->bnm", a, b) / np.sqrt(np.float64(D))
        mag = np.einsum("bdn,bdm->bnm", np.abs(a), np.abs(b)) / np.sqrt(np.float64(D))
    return ref, mag


@functools.lru_cache(maxsize=None)
def _built(name):
    """One full bf16x6 build of a case, shared by its tests (read-only): inputs, the tiled levels'
    export, the fp64 reference."""
    from eraft_amd import _lib
    (B, D, H, W), L, _ = CASES[name]
    f1, f2 = prng.gauss(81, (B, D, H, W)), prng.gauss(82, (B, D, H, W))
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    lv = tiled_levels(B, H, W, L, DEV, fill=float("nan"))
    _lib.build(t1, t2, lv, _lib.BUILD_BF16X6)
    torch.cuda.synchronize()
    return f1, f2, t1, t2, export_levels(lv, H, W)


@pytest.mark.parametrize("name", list(CASES))
def test_levels_pool_bitexact(name):
    """Levels 1-3 (the lane-swap trades and in-register pools) equal avg_pool2d of the exported
    level 0 bit for bit, and no cell inside a map is left unwritten."""
    *_, ex = _built(name)
    assert all(np.isfinite(e).all() for e in ex)
    for l in range(1, len(ex)):
        assert bit_equal(oracle.avg_pool2x2(ex[l - 1]), ex[l]), l


@pytest.mark.parametrize("name", list(CASES))
def test_level0_within_bound(name):
    f1, f2, _, _, ex = _built(name)
    B, D, H, W = f1.shape
    ref, mag = _fp64(f1, f2)
    err = np.abs(ex[0].reshape(B, H * W, H * W).astype(np.float64) - ref)
    bound = (3 + 6 * ((D + 31) // 32)) * U * mag
    print(f"{name}: max |err| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()


@pytest.mark.parametrize("name", list(CASES))
def test_region_build_matches_full(name):
    """corr_build_region over the case's row regions writes the full build's pyramid bit for bit."""
    from eraft_amd import _lib
    (B, D, H, W), L, regions = CASES[name]
    _, _, t1, t2, ex = _built(name)
    reg = tiled_levels(B, H, W, L, DEV, fill=float("nan"))
    ws = _lib.build_workspace(t1, t2, _lib.BUILD_BF16X6)
    ws.fill_(0x5A)
    for k, (y0, y1) in enumerate(regions):
        _lib.build_region(t1, t2[:, :, y0:y1].contiguous(), y0, y1, H, reg, ws, k == 0)
    torch.cuda.synchronize()
    er = export_levels(reg, H, W)
    for l in range(L):
        assert bit_equal(ex[l], er[l]), l


def _pool64(x):
    """2x2 mean over the last two axes (floor sizes), fp64."""
    h, w = x.shape[-2] // 2 * 2, x.shape[-1] // 2 * 2
    x = x[..., :h, :w]
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) * 0.25


@pytest.mark.parametrize("name", ["8x16", "12x16"])
def test_nonfinite_features_match_fp32(name):
    """+inf, -inf and NaN query features placed so that, inside one workgroup (128 queries: wave w
    holds queries 32 w .. 32 w + 31), wave 0 holds infinite accumulators, wave 2 NaN ones without an
    infinity, and waves 1 and 3 finite ones: the per-element merge and the plain merge both run in
    one launch (12x16: also in the 4-row body and in the second query group).  Query 5's infinite
    feature (channel 3) meets targets that are exact in bf16 in that channel — their mid and lo pieces
    are 0, so the small sum is inf * 0 = NaN while hi * hi is infinite — a zero target (inf * 0 = NaN in
    fp32 as well), query 9 holds opposite infinities, and query 18's -inf meets one-signed targets, so
    every level keeps infinities (mixed signs pool to NaN).  On all levels: the NaN cells, the
    infinities and their signs of the fp32-operand build; finite cells within the bound (module
    docstring)."""
    from eraft_amd import _lib
    (B, D, H, W), L, _ = CASES[name]
    f1, f2 = prng.gauss(83, (B, D, H, W)), prng.gauss(84, (B, D, H, W))
    f1[0, 3, 0, 5] = np.inf          # query 5 (wave 0)
    f1[0, 7, 1, 2] = -np.inf         # query 18 (wave 0)
    f1[0, 9, 0, 9] = np.inf          # query 9: opposite infinities
    f1[0, 10, 0, 9] = -np.inf
    f1[0, 4, 5, 1] = np.nan          # query 81 (wave 2): NaN, no infinity
    if H > 8:
        f1[0, 6, 8, 3] = -np.inf     # query 131: wave 0 of the second query group (its wave 1 stays finite)
    f2[0, 3, :, 8:] = torch.from_numpy(f2[0, 3, :, 8:]).bfloat16().float().numpy()  # exact in bf16
    f2[0, 3, 2, 3] = 0.0             # inf * 0
    f2[0, 7] = np.abs(f2[0, 7]) + np.float32(0.1)  # one-signed: query 18 is -inf on every level
    assert (f2[0, 3, :, 8:] != 0).all()
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    out = {}
    for algo in (_lib.BUILD_BF16X6, _lib.BUILD_FP32):
        lv = tiled_levels(B, H, W, L, DEV, fill=float("nan"))
        _lib.build(t1, t2, lv, algo)
        torch.cuda.synchronize()
        out[algo] = export_levels(lv, H, W)
    ref, mag = _fp64(f1, f2)
    N = H * W
    ref, mag = ref.reshape(N, 1, H, W), mag.reshape(N, 1, H, W)
    bound = (3 + 6 * ((D + 31) // 32)) * U * mag
    u1 = U * (1 + 2.0 ** -20)
    with np.errstate(invalid="ignore"):
        for l in range(L):
            if l > 0:
                bound = _pool64(bound) + 3 * u1 * _pool64(mag + bound)
                ref, mag = _pool64(ref), _pool64(mag)
            a, b = out[_lib.BUILD_BF16X6][l], out[_lib.BUILD_FP32][l]
            assert np.isinf(b).any() and np.isnan(b).any() and np.isfinite(b).any(), l
            assert np.array_equal(np.isnan(a), np.isnan(b)), l
            assert np.array_equal(np.isinf(a), np.isinf(b)), l
            inf = np.isinf(b)
            assert np.array_equal(np.signbit(a[inf]), np.signbit(b[inf])), l
            fin = np.isfinite(b)
            assert np.isfinite(ref[fin]).all(), l
            err = np.abs(a[fin].astype(np.float64) - ref[fin])
            print(f"{name} level {l}: max |err| / bound = {(err / bound[fin]).max():.3f}")
            assert (err <= bound[fin]).all(), l
    # the finite waves' queries stayed finite, the infinite feature's targets are infinite or NaN
    lvl0 = out[_lib.BUILD_BF16X6][0]
    assert np.isfinite(lvl0[32:64]).all() and np.isfinite(lvl0[96:128]).all()
    assert np.isinf(lvl0[5, 0, :, 8:]).all() and np.isnan(lvl0[5, 0, 2, 3]) and np.isnan(lvl0[81]).all()
