"""The precision modes of the all-pairs correlation build (corr_build_ex_prec, corr_build_region_prec,
include/corr_mi355x_build_prec.h; eraft_amd/precision.py's resolve_corr, the config key
`corr_precision`, CorrBlock(precision=...)).

CPU: the exports, the knob's resolution, the argument checks through the C ABI (an unknown precision
is refused before every other check and before any HIP call).  GPU: which piece products each mode
keeps, bit for bit, on inputs whose every output is one exact product (tests/_corr_precision.py);
precision 0 against the old entry points; an a-priori element-wise bound against fp64; the pyramid;
region builds; non-finite features; determinism and graph replay; CorrBlock; and the end-to-end flow
against the same mode emulated on the reference (tests/golden/corr_precision_reference.npz,
make_golden_corr_precision.py).
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bf16x6 as bx
import _corr_precision as cp
import _precision as pm
import prng
from _util import bit_equal, load

DEV = cp.DEV
F32, F64 = np.float32, np.float64
REDUCED = cp.REDUCED
NEW = ("corr_build_ex_prec", "corr_build_region_prec")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "corr_mi355x_build_prec.h")
EINVAL, EUNSUPPORTED = -1, -2
# (shape key, pyramid levels): levels 4 is the kernels' FAST form, 2 the general one
CASES = [("d256", 4), ("d256", 2), ("d40", 4), ("d96", 2)]
CASE_IDS = [f"{k}-L{l}" for k, l in CASES]


# ----------------------------------------------------------------------------------------------
# CPU: exports, the knob, the argument checks
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def test_exports(lib):
    from eraft_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(corr_[a-z_]+)\s*\(", src)))
    assert sorted(_lib.BUILD_PREC_EXPORTS) == declared == sorted(NEW)
    others = set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.ENC_PREC_EXPORTS) | set(_lib.TRAIN_HEAD_EXPORTS)
    assert not set(NEW) & others
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.corr_version() == 202


def test_resolve_corr(monkeypatch):
    from eraft_amd import precision
    monkeypatch.delenv(precision.CORR_ENV, raising=False)
    assert precision.CORR_ENV == "ERAFT_AMD_CORR_PRECISION"
    assert precision.resolve_corr(None) == precision.resolve_corr({}) == "bf16x6"
    assert precision.resolve_corr({"corr_precision": True}) == "bf16x3"
    assert precision.resolve_corr({"corr_precision": False}) == "bf16x6"
    assert precision.resolve_corr({"corr_precision": "BF16"}) == "bf16"
    # the other knobs' keys and variables do not reach it
    assert precision.resolve_corr({"mixed_precision": True, "encoder_precision": "bf16"}) == "bf16x6"
    monkeypatch.setenv(precision.ENV, "bf16")
    monkeypatch.setenv(precision.ENCODER_ENV, "bf16")
    assert precision.resolve_corr({}) == "bf16x6"
    # the variable overrides the key; set but empty counts as unset; an unknown name raises
    monkeypatch.setenv(precision.CORR_ENV, "bf16x3")
    assert precision.resolve_corr({"corr_precision": "bf16"}) == "bf16x3"
    assert precision.resolve(None) == "bf16" and precision.resolve_encoder(None) == "bf16"
    monkeypatch.setenv(precision.CORR_ENV, "")
    assert precision.resolve_corr({"corr_precision": "bf16"}) == "bf16"
    monkeypatch.setenv(precision.CORR_ENV, "fp8")
    with pytest.raises(ValueError):
        precision.resolve_corr({})
    monkeypatch.delenv(precision.CORR_ENV)
    with pytest.raises(ValueError):
        precision.resolve_corr({"corr_precision": "tf32"})
    with pytest.raises(ValueError):
        precision.resolve_corr({"corr_precision": 3})


def test_mixed_precision_leaves_the_build_alone(monkeypatch):
    """The reference casts the feature maps to fp32 before CorrBlock, outside its autocast: the
    model's mixed_precision=True must not reduce the build."""
    from eraft_amd import precision
    from eraft_amd.model import ERAFT
    for v in (precision.ENV, precision.ENCODER_ENV, precision.CORR_ENV):
        monkeypatch.delenv(v, raising=False)
    m = ERAFT({"subtype": "standard", "mixed_precision": True}, n_first_channels=3)
    assert (m.precision, m.corr_precision) == ("bf16x3", "bf16x6")
    m = ERAFT({"subtype": "standard", "corr_precision": "bf16"}, n_first_channels=3)
    assert (m.precision, m.encoder_precision, m.corr_precision) == ("bf16x6", "bf16x6", "bf16")
    monkeypatch.setenv(precision.CORR_ENV, "bf16x3")
    assert ERAFT({"subtype": "standard"}, n_first_channels=3).corr_precision == "bf16x3"


def test_reduced_mode_needs_the_bf16_build(monkeypatch):
    from eraft_amd import corr, precision
    monkeypatch.delenv(precision.CORR_ENV, raising=False)
    monkeypatch.delenv("ERAFT_AMD_BUILD", raising=False)
    assert corr._build_precision(None, False) == "bf16x6"
    assert corr._build_precision("bf16", False) == "bf16"
    assert corr._build_precision("bf16", True) == "bf16x6"      # recorded for autograd
    monkeypatch.setenv(precision.CORR_ENV, "bf16x3")
    assert corr._build_precision(None, False) == "bf16x3"
    with pytest.raises(ValueError):
        corr._build_precision("fp16", False)
    for algo in ("fp32", "f16x3"):
        monkeypatch.setenv("ERAFT_AMD_BUILD", algo)
        assert corr._build_precision("bf16x6", False) == "bf16x6"
        for mode in REDUCED:
            with pytest.raises(ValueError, match="bf16x6 build"):
                corr._build_precision(mode, False)
            assert corr._build_precision(mode, True) == "bf16x6"   # recorded for autograd: nothing reduced runs


class _StubRows:
    """A backend that is not HipRows (no precision argument anywhere)."""

    @staticmethod
    def build(f1_rows, f2, num_levels):
        return ["built"]


def test_sharded_block_refuses_other_backends(monkeypatch):
    """RowShardedCorrBlock: a reduced mode raises for a backend that is not HipRows, before any
    build; the default mode reaches such a backend without a precision argument."""
    import torch.distributed as dist
    from eraft_amd import precision, sharded
    monkeypatch.delenv(precision.CORR_ENV, raising=False)
    monkeypatch.delenv("ERAFT_AMD_BUILD", raising=False)
    monkeypatch.setattr(dist, "get_world_size", lambda group=None: 1)
    monkeypatch.setattr(dist, "get_rank", lambda group=None: 0)
    f = torch.zeros(1, 8, 16, 20)
    blk = sharded.RowShardedCorrBlock(f, f, num_levels=2, backend=_StubRows, broadcast=False)
    assert blk.precision == "bf16x6" and blk._levels == ["built"]
    for mode in REDUCED:
        with pytest.raises(ValueError, match="HipRows"):
            sharded.RowShardedCorrBlock(f, f, num_levels=2, backend=_StubRows, broadcast=False, precision=mode)
    monkeypatch.setenv(precision.CORR_ENV, "bf16")
    with pytest.raises(ValueError, match="HipRows"):
        sharded.RowShardedCorrBlock(f, f, num_levels=2, backend=_StubRows, broadcast=False)
    with pytest.raises(ValueError):
        sharded.RowShardedCorrBlock(f, f, num_levels=2, backend=_StubRows, broadcast=False, precision="fp8")


def test_abi_refusals(lib):
    """An unknown precision is CORR_EINVAL although every other argument is invalid too; a reduced
    one with CORR_BUILD_FP32 / _F16X3 is CORR_EUNSUPPORTED; then the counterparts' own checks speak.
    Without a GPU any HIP call would fail differently."""
    pyr = (ctypes.c_void_p * 4)(256, 256, 256, 256)
    for bad in (-1, 3, 7, 1 << 20):
        rc = lib.corr_build_ex_prec(77, None, -5, None, 0, 0, 0, 0, 99, None, 3, 0, bad, None)
        assert rc == EINVAL and "precision" in lib.corr_last_error().decode(), bad
        rc = lib.corr_build_region_prec(77, None, -5, None, 3, 1, 0, 0, 0, 0, 99, None, 3, 0, 0, bad, None)
        assert rc == EINVAL and "precision" in lib.corr_last_error().decode(), bad
    ok = lambda algo, prec, wsb=1 << 40: lib.corr_build_ex_prec(  # noqa: E731
        algo, 256, 4800, 256, 1, 256, 60, 80, 4, pyr, 256, wsb, prec, None)
    for prec in (1, 2):
        for algo in (0, 1, 1 | 0x100, 0 | 0x200):
            assert ok(algo, prec) == EUNSUPPORTED and "CORR_BUILD_BF16X6" in lib.corr_last_error().decode()
            rc = lib.corr_build_region_prec(algo, 256, 4800, 256, 0, 16, 1, 256, 60, 80, 4, pyr, 256, 1 << 40, 1, prec, None)
            assert rc == EUNSUPPORTED
        # the phase flags may be OR-ed in; the counterpart's checks follow
        for algo in (2, 2 | 0x100, 2 | 0x200):
            assert ok(algo, prec, wsb=16) == EINVAL and "workspace" in lib.corr_last_error().decode()
        assert ok(2 | 0x300, prec) == EINVAL and "unknown algorithm" in lib.corr_last_error().decode()
        rc = lib.corr_build_region_prec(2, 256, 4800, 256, 4, 16, 1, 256, 60, 80, 4, pyr, 256, 1 << 40, 1, prec, None)
        assert rc == EINVAL and "y0" in lib.corr_last_error().decode()
    # precision 0 keeps every refusal of the old entry points
    assert ok(7, 0) == EINVAL and "unknown algorithm" in lib.corr_last_error().decode()
    assert ok(1, 0, wsb=16) == EINVAL and "workspace" in lib.corr_last_error().decode()


# ----------------------------------------------------------------------------------------------
# GPU 1: which products each mode keeps
# ----------------------------------------------------------------------------------------------
def _run_onehot(plan, mode, L):
    B, D, H, W = plan.shape
    outs = []
    for r in range(plan.R):
        f1, f2 = plan.inputs(r)
        outs.append(cp.build(f1, f2, L, mode)[0])
    big = torch.cat(outs, 0)
    from eraft_amd import _lib
    return _lib.pyramid_export([big], H, W)[0].cpu().numpy().reshape(plan.R, B * plan.N, plan.N)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("cls,hot", [("A", "q"), ("B", "t")])
@pytest.mark.parametrize("key,L", CASES, ids=CASE_IDS)
def test_kept_products(key, L, cls, hot, mode):
    """Class A (dense full-mantissa targets, one power-of-two query feature per pixel) and class B
    (the mirror): every output is one product, exact in every piece product.  Level 0 equals, bit for
    bit, the product with lo (bf16x3) or mid and lo (bf16) removed from both operands, and differs
    from the bf16x6 build's.  Over the launches every (pixel position of a 128-tile, k) pair of the
    one-hot operand is observed against every pixel of the dense one."""
    shape = cp.SHAPES[key]
    D = shape[1]
    plan = cp.OneHot(cls, shape, hot, range(D), seed=400 + D)
    assert plan.seen.all()
    got = _run_onehot(plan, mode, L)
    differs = 0
    for r in range(plan.R):
        want = plan.kept_product(r, mode)
        assert bit_equal(want, plan.expected(r, mode))   # the kernel's order gives the same bits
        assert bit_equal(got[r], want), (r, mode)
        differs += int((want != plan.expected(r, "bf16x6")).sum())
    assert differs > got.size // 2


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("key,L", CASES, ids=CASE_IDS)
def test_class_c_three_products(key, L, mode):
    """Both operands (hi, mid, 0): bf16x3 gives th qh + tm qh + th qm — not the four-product sum,
    which is the exact product (tm qm absent); bf16 gives th qh."""
    shape = cp.SHAPES[key]
    D = shape[1]
    plan = cp.OneHot("C", shape, "q", [0, D // 3, D - 1, 31], seed=500 + D)
    got = _run_onehot(plan, mode, L)
    for r in range(plan.R):
        want = plan.expected(r, mode)
        t, q = plan.pairs(r)
        four = ((t.astype(F64) * q.astype(F64)).astype(F32) * cp.inv_sqrt(D)).astype(F32).reshape(want.shape)
        assert (want != four).mean() > 0.9
        assert bit_equal(got[r], want), (r, mode)


# ----------------------------------------------------------------------------------------------
# GPU 2-7: random inputs
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rand(key):
    B, D, H, W = cp.SHAPES[key]
    return prng.gauss(61 + D, (B, D, H, W)), prng.gauss(62 + D, (B, D, H, W))


@functools.lru_cache(maxsize=None)
def _pyramid(key, L, mode):
    """The exported pyramid (numpy levels) and the raw tiled levels (cpu) of one build in `mode`,
    into levels pre-filled with NaN."""
    f1, f2 = (cp.gpu(a) for a in _rand(key))
    _, _, H, W = f2.shape
    lv = cp.build(f1, f2, L, mode, fill=float("nan"))
    return cp.export(lv, H, W), [t.cpu().numpy() for t in lv]


@pytest.mark.gpu
@pytest.mark.parametrize("key,L", CASES, ids=CASE_IDS)
def test_precision_0_is_the_old_entry_point(key, L):
    from eraft_amd import _lib
    f1, f2 = (cp.gpu(a) for a in _rand(key))
    B, D, H, W = f2.shape
    ws = _lib.build_workspace(f1, f2, _lib.BUILD_BF16X6)
    old = cp.levels_for(B, H * W, H, W, L, fill=float("nan"))
    cp.raw_build(f1, f2, old, ws)
    new = cp.levels_for(B, H * W, H, W, L, fill=float("nan"))
    cp.raw_build(f1, f2, new, ws, precision=0)
    for a, b in zip(old, new):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for mode in REDUCED:
        red = cp.levels_for(B, H * W, H, W, L, fill=float("nan"))
        cp.raw_build(f1, f2, red, ws, precision=pm.CODE[mode])
        frac = (red[0] != old[0]).float().mean().item()
        print(f"{key} L{L} {mode}: {frac:.3f} of level 0 differs from bf16x6")
        assert frac > 0.5, mode


@pytest.mark.gpu
@pytest.mark.parametrize("H,split,D", [(16, 8, 256), (12, 8, 40)], ids=["16=8+8-d256", "12=8+4-d40"])
def test_region_precision_0_is_the_old_entry_point(H, split, D):
    """corr_build_region_prec at precision 0 against corr_build_region, both straight through
    ctypes, over a partition of the target rows; the reduced modes differ from them."""
    from eraft_amd import _lib
    B, W, L = 2, 20, 3
    f1, f2 = cp.gpu(prng.gauss(81, (B, D, H, W))), cp.gpu(prng.gauss(82, (B, D, H, W)))
    ws = _lib.build_workspace(f1, f2, _lib.BUILD_BF16X6)
    out = {}
    for prec in (None, 0, 1, 2):
        lv = cp.levels_for(B, H * W, H, W, L, fill=float("nan"))
        for k, (y0, y1) in enumerate(((0, split), (split, H))):
            cp.raw_region(f1, f2[:, :, y0:y1].contiguous(), y0, y1, H, lv, ws, k == 0, precision=prec)
        out[prec] = lv
    one = cp.levels_for(B, H * W, H, W, L, fill=float("nan"))
    cp.raw_build(f1, f2, one, ws)
    for a, b, c in zip(out[None], out[0], one):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        assert torch.equal(a.view(torch.int32), c.view(torch.int32))
    for prec in (1, 2):
        assert (out[prec][0] != out[None][0]).float().mean().item() > 0.5, prec


@pytest.mark.gpu
@pytest.mark.parametrize("key", list(cp.SHAPES))
def test_error_bound(key):
    """|out - fp64| <= A + COEF(mode) sum_k |f1_k| |f2_k| / sqrt(D) element-wise, with
    A = (3 + 6 S) 2^-24 sum_k |f1_k| |f2_k| / sqrt(D) the accumulation allowance of
    test_gpu_parity.py::test_build_bf16x6_error_bound (a reduced mode issues fewer MFMAs) and COEF
    from the split (|x - hi| <= 2^-9 |x|, |x - hi - mid| <= 2^-18 |x|: tests/_precision.py).  Each
    mode's max |err| / (sum |f1||f2| / sqrt(D)) must exceed the next finer mode's tenfold."""
    f1, f2 = _rand(key)
    B, D, H, W = f1.shape
    N, S = H * W, (D + 31) // 32
    a, b = f1.reshape(B, D, N).astype(F64), f2.reshape(B, D, N).astype(F64)
    ref = np.einsum("bkq,bkt->bqt", a, b) / np.sqrt(F64(D))
    mag = np.einsum("bkq,bkt->bqt", np.abs(a), np.abs(b)) / np.sqrt(F64(D))
    A = (3 + 6 * S) * 2.0 ** -24 * mag
    r = {}
    for mode in pm.MODES:
        got = _pyramid(key, 1, mode)[0][0].reshape(B, N, N).astype(F64)
        err, bound = np.abs(got - ref), pm.COEF[mode] * mag + A
        r[mode] = (err / mag).max()
        print(f"bound {key} {mode}: max |err| / bound = {(err / bound).max():.4f}, "
              f"max |err| / (sum |f1||f2| / sqrt D) = 2^{np.log2(r[mode]):.2f}")
        assert np.isfinite(got).all()
        assert (err <= bound).all(), mode
    print(f"ratios {key}: bf16x3 / bf16x6 = {r['bf16x3'] / r['bf16x6']:.1f}, bf16 / bf16x3 = {r['bf16'] / r['bf16x3']:.1f}")
    assert r["bf16x3"] >= 10 * r["bf16x6"]
    assert r["bf16"] >= 10 * r["bf16x3"]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", pm.MODES)
@pytest.mark.parametrize("key,L", CASES, ids=CASE_IDS)
def test_pyramid(key, L, mode):
    """Levels 1.. are avg_pool2d of the launch's own level 0, bit for bit.  The padding cells of the
    tiled level-0 maps are zero (products with the zero-padded target records); at the pooled levels
    a padding cell is the pool of its partly padded window or is not written at all (the levels
    start as NaN), exactly where the default build leaves it so: nothing reads them."""
    from eraft_amd.corr import map_floats
    lv, raw = _pyramid(key, L, mode)
    _, _, H, W = cp.SHAPES[key]
    cur = torch.from_numpy(lv[0])
    assert np.isfinite(lv[0]).all()
    for l in range(1, L):
        cur = F.avg_pool2d(cur, 2, stride=2)
        assert bit_equal(lv[l], cur.numpy()), (mode, l)
    # padding cells: those the re-imported pyramid holds as zero (no Gaussian product is exactly zero)
    from eraft_amd import _lib
    again = cp.levels_for(cp.SHAPES[key][0], H * W, H, W, L, fill=float("nan"))
    _lib.pyramid_import([torch.from_numpy(a).to(DEV) for a in lv], again, H, W)
    for l in range(L):
        z = again[l].cpu().numpy()
        assert z.shape[1] == map_floats(H >> l, W >> l)
        pad = z == 0
        assert bit_equal(raw[l][~pad], z[~pad]) and np.isfinite(z).all(), (mode, l)
        if l == 0:
            assert (raw[0][pad] == 0).all() and (pad.any() or (H % 4 == 0 and W % 4 == 0)), mode
        # the untouched (still NaN) padding cells are the default build's
        assert np.array_equal(np.isnan(raw[l]), np.isnan(_pyramid(key, L, "bf16x6")[1][l])), (mode, l)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", pm.MODES)
@pytest.mark.parametrize("H,split", [(16, 8), (12, 8)], ids=["16=8+8", "12=8+4"])
def test_region_and_slab_builds(H, split, mode):
    """Region builds over a partition of the target rows, and a row-slab build (NQ = whole query
    rows), give the bits of the one-call build."""
    from eraft_amd import _lib
    B, D, W, L = 2, 64, 20, 3
    f1, f2 = cp.gpu(prng.gauss(71, (B, D, H, W))), cp.gpu(prng.gauss(72, (B, D, H, W)))
    one = cp.build(f1, f2, L, mode)
    ws = _lib.build_workspace(f1, f2, _lib.BUILD_BF16X6)
    reg = cp.levels_for(B, H * W, H, W, L, fill=float("nan"))
    for k, (y0, y1) in enumerate(((0, split), (split, H))):
        _lib.build_region(f1, f2[:, :, y0:y1].contiguous(), y0, y1, H, reg, ws, k == 0, precision=pm.CODE[mode])
    want = cp.export(one, H, W)
    for a, b in zip(cp.export(reg, H, W), want):
        assert bit_equal(a, b), mode
    rows = 5
    slab = cp.build(f1[:, :, 3:3 + rows].contiguous(), f2, L, mode)
    for a, b in zip(cp.export(slab, H, W), want):
        full = b.reshape(B, H * W, *b.shape[1:])[:, 3 * W:(3 + rows) * W]
        assert bit_equal(a.reshape(full.shape), full), mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_non_finite_features(mode):
    """A +inf, a -inf and a NaN feature: the non-finite cells of every level, and their values, are
    where the bf16x6 build puts them."""
    f1, f2 = (a.copy() for a in _rand("d96"))
    f1[0, 5, 2, 3], f1[0, 7, 4, 9], f2[0, 11, 1, 1], f2[0, 90, 7, 15] = np.inf, -np.inf, np.nan, np.inf
    B, D, H, W = f1.shape
    a = cp.export(cp.build(cp.gpu(f1), cp.gpu(f2), 2, "bf16x6"), H, W)
    b = cp.export(cp.build(cp.gpu(f1), cp.gpu(f2), 2, mode), H, W)
    for x, y in zip(a, b):
        bad = ~np.isfinite(x)
        assert bad.any() and np.array_equal(bad, ~np.isfinite(y))
        assert np.array_equal(np.isnan(x), np.isnan(y))
        assert np.array_equal(x[np.isinf(x)], y[np.isinf(y)])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("key,L", CASES[:1] + CASES[3:], ids=CASE_IDS[:1] + CASE_IDS[3:])
def test_determinism_and_graph_replay(key, L, mode):
    f1, f2 = (cp.gpu(a) for a in _rand(key))
    B, D, H, W = f2.shape
    # (NaN-filled levels: the padding cells that no build writes then agree too)
    first = [t.clone() for t in cp.build(f1, f2, L, mode, fill=float("nan"))]
    second = cp.build(f1, f2, L, mode, fill=float("nan"))
    for a, b in zip(first, second):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    lv = cp.levels_for(B, H * W, H, W, L, fill=0.0)
    from eraft_amd import _lib
    ws = _lib.build_workspace(f1, f2, _lib.BUILD_BF16X6)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _lib.build(f1, f2, lv, _lib.BUILD_BF16X6, ws, precision=pm.CODE[mode])
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        _lib.build(f1, f2, lv, _lib.BUILD_BF16X6, ws, precision=pm.CODE[mode])
    for t in lv:
        t.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, lv):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # and the mode is not the default's arithmetic
    base = cp.build(f1, f2, L, "bf16x6", fill=float("nan"))
    assert not torch.equal(base[0].view(torch.int32), lv[0].view(torch.int32))


# ----------------------------------------------------------------------------------------------
# GPU 8: CorrBlock
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", pm.MODES)
def test_corr_block(monkeypatch, mode):
    from eraft_amd import CorrBlock, _lib, precision
    monkeypatch.delenv(precision.CORR_ENV, raising=False)
    monkeypatch.delenv("ERAFT_AMD_BUILD", raising=False)
    B, D, H, W = 1, 96, 12, 20
    f1, f2 = (cp.gpu(a) for a in _rand("d96"))
    blk = CorrBlock(f1, f2, num_levels=4, radius=4, precision=mode)
    assert blk.precision == mode
    want = cp.export(cp.build(f1, f2, 4, mode), H, W)
    for a, b in zip(blk.corr_pyramid, want):
        assert bit_equal(a.cpu().numpy(), b)
    coords = cp.gpu(prng.gauss(5, (B, 2, H, W)) * 3 + np.stack(np.meshgrid(np.arange(W), np.arange(H)))[None])
    # the same lookups on an imported copy of that pyramid (a default block whose pyramid is assigned)
    other = CorrBlock(f1, f2, num_levels=4, radius=4)
    assert other.precision == "bf16x6"
    other.corr_pyramid = [torch.from_numpy(a).to(DEV) for a in want]
    assert torch.equal(blk(coords).view(torch.int32), other(coords).view(torch.int32))
    w = cp.gpu(prng.gauss(6, (256, 4 * 81, 1, 1)) * 0.1)
    bias = cp.gpu(prng.gauss(7, (256,)))
    assert torch.equal(blk.lookup_conv(coords, w, bias).view(torch.int32),
                       other.lookup_conv(coords, w, bias).view(torch.int32))
    # the variable alone selects the mode (how bench.py is run in one)
    monkeypatch.setenv(precision.CORR_ENV, mode)
    env = CorrBlock(f1, f2, num_levels=4, radius=4)
    assert env.precision == mode
    assert torch.equal(env(coords).view(torch.int32), blk(coords).view(torch.int32))
    monkeypatch.delenv(precision.CORR_ENV)
    # recorded for autograd: the default's arithmetic, and the attribute says so
    g1 = f1.clone().requires_grad_(True)
    tr = CorrBlock(g1, f2, num_levels=4, radius=4, precision=mode)
    assert tr.precision == "bf16x6"
    base = CorrBlock(f1, f2, num_levels=4, radius=4)
    with torch.no_grad():
        assert torch.equal(tr(coords).view(torch.int32), base(coords).view(torch.int32))
    if mode != "bf16x6":
        assert not torch.equal(blk(coords).view(torch.int32), base(coords).view(torch.int32))
        monkeypatch.setenv("ERAFT_AMD_BUILD", "fp32")
        with pytest.raises(ValueError):
            CorrBlock(f1, f2, num_levels=4, radius=4, precision=mode)


# ----------------------------------------------------------------------------------------------
# GPU 9: end to end
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e(mode):
    """[cold low-res, cold full-res, warm low-res, warm full-res] EPE against the reference's fp32
    golden of a model with corr_precision = `mode` (None: the key absent)."""
    from eraft_amd.model import ERAFT
    from test_e2e import _epe
    from test_precision import _base_state
    g = load("g_e2e_dsec")
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    config = {"subtype": "warm_start"}
    if mode is not None:
        config["corr_precision"] = mode
    model = ERAFT(config, n_first_channels=bins).eval()
    model.load_state_dict(_base_state(bins))
    model = model.to(DEV)
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W))).to(DEV)
    finit = torch.from_numpy(g["flow_init"]).to(DEV)
    with torch.no_grad():
        low, ups = model(im1, im2, iters=iters)
        low_w, ups_w = model(im1, im2, iters=iters, flow_init=finit)
    names = (model.precision, model.encoder_precision, model.corr_precision)
    return names, np.array([_epe(low.cpu().numpy(), g["low"]), _epe(ups[-1][..., ::4, ::4].cpu().numpy(), g["up_sub"]),
                            _epe(low_w.cpu().numpy(), g["low_warm"]),
                            _epe(ups_w[-1][..., ::4, ::4].cpu().numpy(), g["up_warm_sub"])])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_e2e_against_the_emulated_reference(monkeypatch, mode):
    """g_e2e_dsec's inputs and weights, all four fusion switches on, the other two knobs at their
    default.  The cold and warm EPE against the reference's fp32 flow is strictly above the bf16x6
    path's in the same run, and at most 1.5 x the same mode emulated on the reference
    (corr_precision_reference.npz; the margin of test_precision.py's end-to-end test)."""
    from eraft_amd import precision
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    for v in (precision.ENV, precision.ENCODER_ENV, precision.CORR_ENV, "ERAFT_AMD_BUILD"):
        monkeypatch.delenv(v, raising=False)
    monkeypatch.setattr(SepConvGRU, "fused", True)
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", True)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", True)
    fx = load("corr_precision_reference")
    assert list(fx["meta"]) == list(load("g_e2e_dsec")["meta"])
    names0, base = _e2e(None)
    names, errs = _e2e(mode)
    assert names0 == ("bf16x6",) * 3 and names == ("bf16x6", "bf16x6", mode)
    emu = fx["emu_" + mode]
    fmt = lambda v: " / ".join(f"{e:.3e}" for e in v)
    print(f"e2e corr {mode} EPE cold low / up, warm low / up: {fmt(errs)} px; bf16x6 {fmt(base)}; "
          f"emulated {fmt(emu)}; GPU / emulated {fmt(errs / emu)}")
    assert np.isfinite(errs).all()
    assert (errs > base).all()
    assert (errs <= 1.5 * emu).all()
