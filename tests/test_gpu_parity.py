"""Parity of the HIP path (eraft_amd -> libcorr_mi355x.so) against the reference's golden
vectors and the oracle, on an MI355X.  Run on the GPU box: pytest -m gpu.

Bars (north_star): correlation within 1e-4 norm-relative; pooling and lookup BIT-EXACT on
identical inputs; backward within 1e-4 norm-relative.
"""
import functools

import numpy as np
import pytest
import torch

import prng
from _util import (REL_TOL, _bwd_case, bit_equal, build_level0, cell_bound_k, cell_magnitude, cell_ratio, export_levels,
                   golden_names, load, norm_rel, tiled_levels, within_cell_bound)
from oracle import oracle

pytestmark = pytest.mark.gpu

BUILD_CASES = [n for n in golden_names() if not n.startswith(("g_bwd", "g_dsec", "g_e2e", "g_splat", "g_voxel"))]
DEV = "cuda:0"


@pytest.fixture(scope="module", autouse=True)
def _native():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from eraft_amd import _lib
    _lib.load()  # the HIP library must be the thing under test (no fallback exists)


def _cb():
    from eraft_amd import CorrBlock
    return CorrBlock


def _fmaps(meta, dev=DEV):
    seed, B, D, H, W = (int(v) for v in meta[:5])
    f1 = prng.gauss(seed, (B, D, H, W))
    f2 = prng.gauss(seed + 1, (B, D, H, W))
    return f1, f2, torch.from_numpy(f1).to(dev), torch.from_numpy(f2).to(dev)


ALGOS = ["bf16x6", "f16x3", "fp32"]


@functools.lru_cache(maxsize=8)
def _bwd_case_magnitude(T, B, H, W, L, r, seed):
    """cell_magnitude (the per-cell scale of within_cell_bound) of _bwd_case's lookups, computed on
    the CPU oracle once per case."""
    cs, gs = _bwd_case(T, B, H, W, L, r, seed)
    return cell_magnitude([c.cpu().numpy() for c in cs], [g.cpu().numpy() for g in gs], H, W, L, r)


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", BUILD_CASES)
def test_build_matches_reference(name, algo, monkeypatch):
    monkeypatch.setenv("ERAFT_AMD_BUILD", algo)
    g = load(name)
    L, r = int(g["meta"][5]), int(g["meta"][6])
    _, _, t1, t2 = _fmaps(g["meta"])
    cb = _cb()(t1, t2, num_levels=L, radius=r)
    torch.cuda.synchronize()
    assert len(cb.corr_pyramid) == L
    gpu = [p.cpu().numpy() for p in cb.corr_pyramid]
    for l in range(L):
        assert gpu[l].shape == g[f"pyr{l}"].shape
        assert norm_rel(gpu[l], g[f"pyr{l}"]) < REL_TOL, l
    # fused in-register pyramid is bit-identical to avg_pool2d of the kernel's own level 0
    for l in range(1, L):
        assert bit_equal(oracle.avg_pool2x2(gpu[l - 1]), gpu[l]), l


@pytest.mark.parametrize("algo", ["bf16x6", "f16x3"])
@pytest.mark.parametrize("shape", [(1, 256, 60, 80), (8, 256, 36, 48), (3, 256, 36, 44), (2, 200, 17, 23),
                                   (1, 64, 9, 130), (2, 96, 20, 46), (1, 128, 16, 32), (2, 40, 7, 5),
                                   (1, 300, 12, 16)])
def test_split_build_shapes_deterministic(shape, algo, monkeypatch):
    """The split builds at shapes that exercise their padding (query count not a multiple of 128,
    H not a multiple of 8, W not a multiple of 16 / 4 / 2, K not a multiple of 32, D > 256: the
    runtime K loop): level 0 within tolerance of the oracle on sampled queries, levels 1-3
    bit-identical to avg_pool2d of the kernel's own level 0 (16-B, 8-B and element stores), and
    two runs bit-identical."""
    B, D, H, W = shape
    if algo == "f16x3" and D > 256:
        pytest.skip("f16x3 supports D <= 1024 through the same loop; covered at D <= 256")
    monkeypatch.setenv("ERAFT_AMD_BUILD", algo)
    f1, f2 = prng.gauss(11, (B, D, H, W)), prng.gauss(12, (B, D, H, W))
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    L = min(4, int(np.log2(min(H, W))) + 1)
    pyrs = []
    for _ in range(2):
        cb = _cb()(t1, t2, num_levels=L, radius=4)
        torch.cuda.synchronize()
        pyrs.append([p.cpu().numpy() for p in cb.corr_pyramid])
    for l in range(L):
        assert bit_equal(pyrs[0][l], pyrs[1][l]), l
    N = H * W
    for qi in np.unique(np.linspace(0, B * N - 1, 40).astype(int)):
        b, n = divmod(int(qi), N)
        row = oracle.corr_rows(f1[b:b + 1], f2[b:b + 1], n, n + 1)[0, 0]
        assert norm_rel(pyrs[0][0][qi, 0].ravel(), row) < REL_TOL, qi
    for l in range(1, L):
        assert bit_equal(oracle.avg_pool2x2(pyrs[0][l - 1]), pyrs[0][l]), l


@pytest.mark.parametrize("algo", ["bf16x6", "f16x3"])
@pytest.mark.parametrize("shape", [(1, 256, 60, 80), (2, 200, 17, 23)])
def test_split_build_phases_compose(shape, algo):
    """The measurement flags CORR_BUILD_ONLY_PACK then CORR_BUILD_ONLY_MFMA (bench.py times the
    two kernels separately with them) write the same pyramid, bit for bit, as one full build."""
    from eraft_amd import _lib
    A = _lib._ALGOS[algo]
    B, D, H, W = shape
    t1 = torch.from_numpy(prng.gauss(21, (B, D, H, W))).to(DEV)
    t2 = torch.from_numpy(prng.gauss(22, (B, D, H, W))).to(DEV)
    L = min(4, int(np.log2(min(H, W))) + 1)
    full = tiled_levels(B, H, W, L, DEV)
    split = tiled_levels(B, H, W, L, DEV, fill=float("nan"))
    ws = _lib.build_workspace(t1, t2, A)
    _lib.build(t1, t2, full, A, ws)
    ws.zero_()
    _lib.build(t1, t2, split, A | _lib.BUILD_ONLY_PACK, ws)
    _lib.build(t1, t2, split, A | _lib.BUILD_ONLY_MFMA, ws)
    torch.cuda.synchronize()
    ef, es = export_levels(full, H, W), export_levels(split, H, W)
    for l in range(L):
        assert bit_equal(ef[l], es[l]), l


@pytest.mark.parametrize("shape,regions", [
    ((1, 256, 60, 80), [(0, 16), (16, 32), (32, 48), (48, 60)]),
    ((1, 256, 60, 80), [(32, 60), (0, 8), (8, 32)]),          # any order: queries packed by the first call
    ((8, 256, 36, 48), [(0, 8), (8, 24), (24, 36)]),
    ((2, 200, 17, 23), [(0, 8), (8, 16), (16, 17)]),          # D % 32 != 0, H % 8 != 0, W % 16 != 0
    ((1, 300, 20, 32), [(0, 16), (16, 20)]),                  # D > 256: the runtime K loop
    ((3, 64, 24, 40), [(0, 24)]),
])
def test_build_region_matches_full(shape, regions):
    """corr_build_region over a partition of the target rows, each call reading only its slab of
    fmap2 ([B, D, y1 - y0, W]), writes the pyramid of one corr_build_ex call bit for bit (the
    chunked fmap2 broadcast of the row-sharded path builds this way)."""
    from eraft_amd import _lib
    B, D, H, W = shape
    t1 = torch.from_numpy(prng.gauss(61, (B, D, H, W))).to(DEV)
    t2 = torch.from_numpy(prng.gauss(62, (B, D, H, W))).to(DEV)
    L = min(4, int(np.log2(min(H, W))) + 1)
    full = tiled_levels(B, H, W, L, DEV)
    reg = tiled_levels(B, H, W, L, DEV, fill=float("nan"))
    _lib.build(t1, t2, full, _lib.BUILD_BF16X6)
    ws = _lib.build_workspace(t1, t2, _lib.BUILD_BF16X6)
    ws.fill_(0x5A)
    for k, (y0, y1) in enumerate(regions):
        _lib.build_region(t1, t2[:, :, y0:y1].contiguous(), y0, y1, H, reg, ws, k == 0)
    torch.cuda.synchronize()
    ef, er = export_levels(full, H, W), export_levels(reg, H, W)
    for l in range(L):
        assert bit_equal(ef[l], er[l]), l


@pytest.mark.parametrize("name", BUILD_CASES)
def test_lookup_bitexact_on_reference_pyramid(name):
    g = load(name)
    L, r = int(g["meta"][5]), int(g["meta"][6])
    _, _, t1, t2 = _fmaps(g["meta"])
    cb = _cb()(t1, t2, num_levels=L, radius=r)
    # feed the kernel the reference's own pyramid (installed through corr_pyramid_import): output
    # must match bit for bit
    cb.corr_pyramid = [torch.from_numpy(g[f"pyr{l}"]).to(DEV) for l in range(L)]
    keys = [k[len("coords"):] for k in g if k.startswith("coords")]
    for k in keys:
        out = cb(torch.from_numpy(g["coords" + k]).to(DEV)).cpu().numpy()
        assert out.shape == g["look" + k].shape
        assert bit_equal(out, g["look" + k]), k


def test_corr_staticmethod_shape_and_values():
    g = load("g_b2_d64_16x20_L2r3")
    _, _, t1, t2 = _fmaps(g["meta"])
    vol = _cb().corr(t1, t2)
    assert tuple(vol.shape) == tuple(g["corr_shape"])
    B, H, W = vol.shape[0], vol.shape[1], vol.shape[2]
    assert norm_rel(vol.reshape(B * H * W, 1, H, W).cpu().numpy(), g["pyr0"]) < REL_TOL


def _ref_autograd(f1n, f2n, L, r, coords, grads, pyr_grads=None, vol_grad=None):
    """fp64 torch-CPU autograd of the reference composition (oracle/torch_ops.py restates
    model/corr.py:13-60 op by op): lookups with upstream gradients `grads`, plus optional loss
    terms on the pyramid levels (corr_pyramid) and on the static corr volume."""
    from oracle import torch_ops
    a = torch.from_numpy(f1n).double().requires_grad_(True)
    b = torch.from_numpy(f2n).double().requires_grad_(True)
    loss = 0.0
    if L:
        lv = torch_ops.cpu_build(a, b, L)
        for c, g in zip(coords, grads):
            loss = loss + (torch_ops.cpu_lookup(lv, torch.from_numpy(c).double(), r) * torch.from_numpy(g).double()).sum()
        for l, g in (pyr_grads or {}).items():
            loss = loss + (lv[l] * torch.from_numpy(g).double()).sum()
    if vol_grad is not None:
        B, D, H, W = f1n.shape
        vol = torch.matmul(a.reshape(B, D, H * W).transpose(1, 2), b.reshape(B, D, H * W)) / np.sqrt(D)
        loss = loss + (vol.reshape(vol_grad.shape) * torch.from_numpy(vol_grad).double()).sum()
    loss.backward()
    return a.grad.numpy(), b.grad.numpy()


@pytest.mark.parametrize("which", ["both", "fmap1", "fmap2"])
def test_corr_staticmethod_is_differentiable(which):
    """CorrBlock.corr (model/corr.py:52-60, a torch matmul) passes gradients to the
    feature maps it requires them for, within the north_star's 1e-4 of fp64 autograd."""
    B, D, H, W = 2, 48, 12, 16
    f1n, f2n = prng.gauss(91, (B, D, H, W)), prng.gauss(92, (B, D, H, W))
    G = prng.gauss(93, (B, H, W, 1, H, W))
    t1 = torch.from_numpy(f1n).to(DEV).requires_grad_(which in ("both", "fmap1"))
    t2 = torch.from_numpy(f2n).to(DEV).requires_grad_(which in ("both", "fmap2"))
    vol = _cb().corr(t1, t2)
    assert vol.requires_grad and tuple(vol.shape) == (B, H, W, 1, H, W)
    (vol * torch.from_numpy(G).to(DEV)).sum().backward()
    r1, r2 = _ref_autograd(f1n, f2n, 0, 0, [], [], vol_grad=G)
    for t, ref in ((t1, r1), (t2, r2)):
        if t.requires_grad:
            assert norm_rel(t.grad.cpu().numpy(), ref) < REL_TOL
        else:
            assert t.grad is None
    with torch.no_grad():  # and no graph under no_grad
        assert not _cb().corr(t1, t2).requires_grad


@pytest.mark.parametrize("lookups", [False, True])
def test_corr_pyramid_gradients_match_reference(lookups):
    """gradients that reach the exported corr_pyramid view (alone, and mixed with
    lookups) match fp64 autograd of the reference composition (matmul / sqrt(D), avg_pool2d,
    grid_sample) within 1e-4 — not only the per-lookup path."""
    B, D, H, W, L, r = 1, 32, 16, 20, 3, 3
    f1n, f2n = prng.gauss(94, (B, D, H, W)), prng.gauss(95, (B, D, H, W))
    N = H * W
    pg = {0: prng.gauss(96, (B * N, 1, H, W)), 2: prng.gauss(97, (B * N, 1, H >> 2, W >> 2))}
    K = (2 * r + 1) ** 2
    cs = [prng.lookup_coords(98 + t, B, H, W, 2.0) for t in range(2)] if lookups else []
    gs = [prng.gauss(100 + t, (B, L * K, H, W)) for t in range(2)] if lookups else []
    t1 = torch.from_numpy(f1n).to(DEV).requires_grad_(True)
    t2 = torch.from_numpy(f2n).to(DEV).requires_grad_(True)
    cb = _cb()(t1, t2, L, r)
    loss = sum((cb.corr_pyramid[l] * torch.from_numpy(g).to(DEV)).sum() for l, g in pg.items())
    for c, g in zip(cs, gs):
        loss = loss + (cb(torch.from_numpy(c).to(DEV)) * torch.from_numpy(g).to(DEV)).sum()
    loss.backward()
    r1, r2 = _ref_autograd(f1n, f2n, L, r, cs, gs, pyr_grads=pg)
    assert norm_rel(t1.grad.cpu().numpy(), r1) < REL_TOL
    assert norm_rel(t2.grad.cpu().numpy(), r2) < REL_TOL


def test_corr_pyramid_view_follows_grad_mode():
    """a corr_pyramid first read under no_grad is re-exported for a later
    grad-enabled read (which then carries gradients); an assigned pyramid makes later lookups
    constant, as in the reference, and assigning levels that require grad raises."""
    B, D, H, W, L, r = 1, 16, 12, 16, 2, 2
    t1 = torch.from_numpy(prng.gauss(111, (B, D, H, W))).to(DEV).requires_grad_(True)
    t2 = torch.from_numpy(prng.gauss(112, (B, D, H, W))).to(DEV).requires_grad_(True)
    cb = _cb()(t1, t2, L, r)
    with torch.no_grad():
        v0 = cb.corr_pyramid
    assert not v0[0].requires_grad
    v1 = cb.corr_pyramid
    assert v1[0].requires_grad and bit_equal(v1[0].detach().cpu().numpy(), v0[0].cpu().numpy())
    v1[0].sum().backward()
    assert t1.grad is not None and t2.grad is not None
    c = torch.from_numpy(prng.lookup_coords(113, B, H, W, 1.0)).to(DEV)
    before = cb(c).detach()
    cb.corr_pyramid = [2 * v.detach() for v in v1]
    after = cb(c)
    assert not after.requires_grad  # reads the assigned (constant) tensors
    assert bit_equal(after.cpu().numpy(), (2 * before).cpu().numpy())
    with pytest.raises(NotImplementedError):
        cb.corr_pyramid = [v.detach().requires_grad_(True) for v in v1]


def test_short_level_buffers_are_refused():
    """a caller handing the library reference-layout (ABI-104) [B*N, 1, H_l, W_l]
    value levels — smaller than the tiled maps when H_l or W_l is not a multiple of 4 — gets a
    ValueError before any device access."""
    from eraft_amd import _lib
    B, D, H, W, L, r = 1, 16, 30, 40, 2, 2
    f1 = torch.from_numpy(prng.gauss(121, (B, D, H, W))).to(DEV)
    short = [torch.empty(B * H * W, 1, H >> l, W >> l, device=DEV) for l in range(L)]  # 30 x 40: level 1 15 x 20
    with pytest.raises(ValueError, match="map_floats"):
        _lib.build(f1, f1, short)
    c = torch.from_numpy(prng.lookup_coords(122, B, H, W, 1.0)).to(DEV)
    out = torch.empty(B, L * (2 * r + 1) ** 2, H, W, device=DEV)
    with pytest.raises(ValueError, match="map_floats"):
        _lib.lookup(short, c, r, out)


@pytest.mark.parametrize("name", golden_names("g_bwd"))
def test_backward_matches_reference(name):
    g = load(name)
    seed, B, D, H, W, L, r, iters = (int(v) for v in g["meta"])
    t1 = torch.from_numpy(prng.gauss(seed, (B, D, H, W))).to(DEV).requires_grad_(True)
    t2 = torch.from_numpy(prng.gauss(seed + 1, (B, D, H, W))).to(DEV).requires_grad_(True)
    cb = _cb()(t1, t2, num_levels=L, radius=r)
    K = (2 * r + 1) ** 2
    loss = 0.0
    for t in range(iters):
        c = torch.from_numpy(prng.lookup_coords(seed + 200 + t, B, H, W, 2.0 + t)).to(DEV)
        gr = torch.from_numpy(prng.gauss(seed + 300 + t, (B, L * K, H, W))).to(DEV)
        loss = loss + (cb(c) * gr).sum()
    loss.backward()
    assert norm_rel(t1.grad.cpu().numpy(), g["df1"]) < REL_TOL
    assert norm_rel(t2.grad.cpu().numpy(), g["df2"]) < REL_TOL


def test_dsec_shape_against_reference_slices():
    g = load("g_dsec_spot")
    seed, B, D, H, W, L, r = (int(v) for v in g["meta"])
    _, _, t1, t2 = _fmaps(g["meta"])
    cb = _cb()(t1, t2, num_levels=L, radius=r)
    q = torch.from_numpy(g["q"]).to(DEV)
    for l in range(L):
        rows = cb.corr_pyramid[l][q].cpu().numpy()
        assert norm_rel(rows, g[f"pyr{l}_rows"]) < REL_TOL
        full = cb.corr_pyramid[l].double()
        s, a = float(full.sum()), float(full.abs().sum())
        assert abs(s - g[f"pyr{l}_sum"][0]) <= 1e-4 * g[f"pyr{l}_sum"][1]
        assert abs(a - g[f"pyr{l}_sum"][1]) <= 1e-4 * g[f"pyr{l}_sum"][1]
    c = torch.from_numpy(prng.lookup_coords(seed + 100, B, H, W, 8.0)).to(DEV)
    o = cb(c)
    oq = o.reshape(B, -1, H * W)[:, :, q].cpu().numpy()
    assert norm_rel(oq, g["look_q"]) < REL_TOL
    assert abs(float(o.double().abs().sum()) - g["look_sum"][1]) <= 1e-4 * g["look_sum"][1]


@pytest.mark.parametrize("B,D,H,W,L,r", [
    (1, 256, 60, 80, 4, 4),     # DSEC 480x640
    (2, 256, 36, 44, 4, 4),     # MVSEC padded (B reduced for oracle time)
    (1, 20, 17, 23, 3, 2),      # odd sizes, D not a multiple of the k-chunk, scalar paths
    (3, 7, 9, 13, 2, 1),
    (1, 33, 8, 8, 4, 4),        # smallest legal 4-level map (level 3 is 1x1 -> NaN lookups)
])
@pytest.mark.parametrize("algo", ALGOS)
def test_gpu_pyramid_and_lookup_vs_oracle(B, D, H, W, L, r, algo, monkeypatch):
    monkeypatch.setenv("ERAFT_AMD_BUILD", algo)
    f1 = prng.gauss(B * 1000 + D, (B, D, H, W))
    f2 = prng.gauss(B * 1000 + D + 1, (B, D, H, W))
    cb = _cb()(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    gpu = [p.cpu().numpy() for p in cb.corr_pyramid]
    N = H * W
    sel = np.unique(np.linspace(0, B * N - 1, 24).astype(int))
    for qi in sel:
        b, n = divmod(int(qi), N)
        row = oracle.corr_rows(f1[b:b + 1], f2[b:b + 1], n, n + 1)[0, 0]
        assert norm_rel(gpu[0][qi, 0].ravel(), row) < REL_TOL
    for l in range(1, L):
        assert bit_equal(oracle.avg_pool2x2(gpu[l - 1]), gpu[l])
    for k, sig in enumerate([0.0, 4.0, 25.0]):
        c = prng.lookup_coords(7 + k, B, H, W, sig)
        out = cb(torch.from_numpy(c).to(DEV)).cpu().numpy()
        assert bit_equal(out, oracle.lookup(gpu, c, r))
    c = prng.special_coords(B, H, W)
    assert bit_equal(cb(torch.from_numpy(c).to(DEV)).cpu().numpy(), oracle.lookup(gpu, c, r))


@pytest.mark.parametrize("B,H,W", [(1, 120, 160), (2, 90, 104)])
def test_lookup_tight_gather_vs_oracle(B, H, W):
    """>= 18,000 queries: the lookup gathers only the window rows / 16-B chunks its taps touch
    (corr_lookup.hip launch_lookup_qb; TIGHT in corr_lookup_block.h).  Bit-exact against the oracle on the exported
    pyramid for random flows, the integer grid (every tap on a cell: the window's extra row and
    column unused), the special coordinates (borders, far outside, half pixels) and NaN / inf /
    huge coordinates sprinkled over the map."""
    D, L, r = 32, 4, 4
    f1, f2 = prng.gauss(91, (B, D, H, W)), prng.gauss(92, (B, D, H, W))
    cb = _cb()(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    pyr = [p.cpu().numpy() for p in cb.corr_pyramid]
    cases = [prng.lookup_coords(93, B, H, W, 6.0), prng.coords_grid(B, H, W), prng.special_coords(B, H, W)]
    c = prng.lookup_coords(94, B, H, W, 3.0)
    flat = c.reshape(-1)
    idx = (prng.uniform(95, (64,)) * flat.size).astype(np.int64)
    flat[idx] = np.resize(np.array([np.nan, np.inf, -np.inf, 3.0e38, -1e30, 1e6, -0.0, 2.0 ** 20], np.float32), 64)
    cases.append(c)
    for c in cases:
        out = cb(torch.from_numpy(c).to(DEV)).cpu().numpy()
        assert bit_equal(out, oracle.lookup(pyr, c, r))


@pytest.mark.parametrize("case", ["channel_scales", "pixel_scales", "zeros", "tiny", "huge"])
def test_build_f16x3_dynamic_range(case):
    """The f16 split keeps fp32 accuracy over wide feature ranges: per-channel scales over
    6 decades with the two maps' channel scales anti-correlated (the small features of one map
    meet the large of the other), per-pixel scales over 20 decades, all-zero pixels, tiny and
    near-overflow magnitudes.  (The split's floor: features below 2^-38 of their pixel's
    largest flush to zero — 11+ decades, include/corr_mi355x.h.)  Bar: the north_star's 1e-4 (norm-relative per query row, against
    the fp64 oracle), and the fp32-operand MFMA build on the same inputs."""
    from eraft_amd import _lib
    B, D, H, W = 1, 96, 12, 16
    f1 = prng.gauss(11, (B, D, H, W)).astype(np.float64)
    f2 = prng.gauss(12, (B, D, H, W)).astype(np.float64)
    if case == "channel_scales":
        s = 10.0 ** np.linspace(-3, 3, D)[None, :, None, None]
        f1, f2 = f1 * s, f2 * s[:, ::-1]
    elif case == "pixel_scales":
        s = 10.0 ** np.linspace(-10, 10, H * W).reshape(1, 1, H, W)
        f1, f2 = f1 * s, f2 * s[..., ::-1, ::-1]
    elif case == "zeros":
        f1[:, :, ::3] = 0.0
        f2[:, :, :, ::5] = 0.0
    elif case == "tiny":
        f1, f2 = f1 * 1e-15, f2 * 1e-16
    elif case == "huge":
        f1, f2 = f1 * 1e17, f2 * 1e17
    f1, f2 = f1.astype(np.float32), f2.astype(np.float32)
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    ref = oracle.corr_rows(f1, f2).reshape(B * H * W, H * W)
    outs = {}
    for algo in (_lib.BUILD_F16X3, _lib.BUILD_FP32):
        outs[algo] = build_level0(t1, t2, algo)
    for algo, o in outs.items():
        assert np.isfinite(o).all() == np.isfinite(ref).all()
        scale = np.abs(ref).max(axis=1)
        err = np.abs(o - ref).max(axis=1)
        ok = scale > 0
        assert (err[ok] / scale[ok]).max() < REL_TOL, (algo, (err[ok] / scale[ok]).max())
        assert (err[~ok] == 0).all()


def _fp64_rows(f1, f2, rows):
    """fp64 restatement of corr.py:58-60 for query pixels `rows` of batch item 0: [len, N]."""
    B, D, H, W = f1.shape
    a = f1[0].reshape(D, H * W).astype(np.float64)[:, rows]
    b = f2[0].reshape(D, H * W).astype(np.float64)
    return (a.T @ b) / np.sqrt(np.float64(D))


def _dyn_range_inputs(case, B=1, D=96, H=12, W=16):
    f1 = prng.gauss(11, (B, D, H, W)).astype(np.float64)
    f2 = prng.gauss(12, (B, D, H, W)).astype(np.float64)
    if case == "channel_scales":  # the small features of one map meet the large of the other
        s = 10.0 ** np.linspace(-3, 3, D)[None, :, None, None]
        f1, f2 = f1 * s, f2 * s[:, ::-1]
    elif case == "pixel_scales":
        s = 10.0 ** np.linspace(-10, 10, H * W).reshape(1, 1, H, W)
        f1, f2 = f1 * s, f2 * s[..., ::-1, ::-1]
    elif case == "zeros":
        f1[:, :, ::3] = 0.0
        f2[:, :, :, ::5] = 0.0
    elif case == "tiny":
        f1, f2 = f1 * 1e-15, f2 * 1e-16
    elif case == "huge":
        f1, f2 = f1 * 1e17, f2 * 1e17
    elif case == "cancel":  # dot products that cancel to ~1e-4 of their terms
        f2[:, 1::2] = -f2[:, 0::2] * (1 + 1e-4 * prng.gauss(13, f2[:, 1::2].shape))
        f1[:, 1::2] = f1[:, 0::2]
    return f1.astype(np.float32), f2.astype(np.float32)


BF16_CASES = ["gauss", "channel_scales", "pixel_scales", "zeros", "tiny", "huge", "dsec"]


@pytest.mark.parametrize("case", BF16_CASES + ["cancel"])
def test_build_bf16x6_error_bound(case):
    """Element-wise a-priori bound of the bf16x6 build: |C - C64| <= (3 + 6 S) u sum_k |a_k b_k| / sqrt(D)
    (u = 2^-24, S = ceil(D / 32)): 2u for the dropped piece products, one rounding per MFMA into
    the accumulator (6 S of them), one for the output.  An fp32 fmaf chain's bound is D u sum|ab|
    (Higham's gamma_D) — 256 u at D = 256 against 51 u here — so the split is provably no
    narrower.  Includes a cancelling case (results ~1e-4 of their terms), where only such a bound
    is meaningful."""
    from eraft_amd import _lib
    if case == "dsec":
        f1, f2 = prng.gauss(31, (1, 256, 60, 80)), prng.gauss(32, (1, 256, 60, 80))
        rows = np.unique(np.linspace(0, 4799, 48).astype(int))
    else:
        f1, f2 = _dyn_range_inputs(case)
        rows = np.arange(f1.shape[2] * f1.shape[3])
    B, D, H, W = f1.shape
    S = (D + 31) // 32
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    o = build_level0(t1, t2, _lib.BUILD_BF16X6)[rows].astype(np.float64)
    ref = _fp64_rows(f1, f2, rows)
    a = np.abs(f1[0].reshape(D, H * W).astype(np.float64)[:, rows])
    b = np.abs(f2[0].reshape(D, H * W).astype(np.float64))
    mag = (a.T @ b) / np.sqrt(np.float64(D))
    bound = (3 + 6 * S) * 2.0 ** -24 * mag
    ratio = np.abs(o - ref) / np.maximum(bound, 1e-300)
    print(f"{case}: max |err| / bound = {ratio.max():.3f}")
    assert (np.abs(o - ref) <= bound).all()


@pytest.mark.parametrize("case", BF16_CASES)
def test_build_bf16x6_not_narrower_than_fp32(case):
    """The bf16x6 build (three exact bf16 pieces per feature, six piece products) is no narrower
    than the exact-fp32 MFMA build (the arithmetic of the reference's fp32 matmul, corr.py:58):
    on every query row its max error against an fp64 restatement is at most the fp32 build's
    plus one fp32 ulp of the row's largest value (both round their results to fp32), and over
    all rows its worst and its mean row error are at most the fp32 build's."""
    from eraft_amd import _lib
    if case == "dsec":
        f1, f2 = prng.gauss(31, (1, 256, 60, 80)), prng.gauss(32, (1, 256, 60, 80))
        rows = np.unique(np.linspace(0, 4799, 96).astype(int))
    else:
        f1, f2 = _dyn_range_inputs(case)
        rows = np.arange(f1.shape[2] * f1.shape[3])
    B, D, H, W = f1.shape
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    ref = _fp64_rows(f1, f2, rows)
    err = {}
    for algo in (_lib.BUILD_BF16X6, _lib.BUILD_FP32):
        o = build_level0(t1, t2, algo)[rows].astype(np.float64)
        assert np.isfinite(o).all()
        err[algo] = np.abs(o - ref).max(axis=1)
    scale = np.abs(ref).max(axis=1)
    ulp = scale * 2.0 ** -23
    bf, f32 = err[_lib.BUILD_BF16X6], err[_lib.BUILD_FP32]
    ok = scale > 0
    rel_bf, rel_f32 = bf[ok] / scale[ok], f32[ok] / scale[ok]
    print(f"{case}: bf16x6 row error max {rel_bf.max():.3e} mean {rel_bf.mean():.3e}; "
          f"fp32 max {rel_f32.max():.3e} mean {rel_f32.mean():.3e}")
    assert (bf[~ok] == 0).all()
    assert (bf <= f32 + ulp).all(), np.max((bf - f32) / np.maximum(scale, 1e-300))
    assert rel_bf.max() <= rel_f32.max()
    assert rel_bf.mean() <= rel_f32.mean()


def _bwd_fp64(gc, f1, f2):
    """fp64 restatement of autograd of corr.py:58-60: dF1 = F2 dC^T / sqrt(D), dF2 = F1 dC / sqrt(D)
    and the same products of magnitudes (the a-priori error bound's sum |a b|)."""
    B, D, H, W = f2.shape
    N = H * W
    c = gc.reshape(B, N, N).astype(np.float64)
    a1, a2 = f1.reshape(B, D, N).astype(np.float64), f2.reshape(B, D, N).astype(np.float64)
    s = np.sqrt(np.float64(D))
    ct = np.swapaxes(c, 1, 2)
    d1 = np.matmul(a2, ct) / s             # [b][d][n] = sum_m F2[d][m] dC[n][m]
    d2 = np.matmul(a1, c) / s              # [b][d][m] = sum_n F1[d][n] dC[n][m]
    m1 = np.matmul(np.abs(a2), np.abs(ct)) / s
    m2 = np.matmul(np.abs(a1), np.abs(c)) / s
    return d1, d2, m1, m2


@pytest.mark.parametrize("case", ["gauss", "row_scales", "train", "dsec"])
def test_build_bwd_bf16x6_not_narrower_than_fp32(case):
    """The backward GEMMs on bf16x6 (the default for the bf16x6 build: both operands split
    exactly into three bf16 pieces while staging, six piece products, one accumulator) against
    the fp32-operand MFMA GEMMs, both vs an fp64 restatement: every element is within the
    a-priori bound (3 + 6 ceil(K/16) + 16) u sum|ab| (dropped piece products, one rounding per
    MFMA, the split-K sum, the output) — about 0.38 K u against the K u of an fp32 fmaf chain —
    and over the output rows (feature d) the worst and the mean row error are at most the fp32
    GEMMs'.  Unlike the build (two accumulators), single rows are not dominated: with one
    accumulator per register budget the per-row errors are two draws of similar rounding noise
    (6 vs 8 roundings per 16 k), so a row can land above fp32's; the fraction is printed."""
    from eraft_amd import _lib
    # dsec: 494 GEMM workgroups, more than one round, so dF1's sum runs as its own launch instead
    # of riding in dF2's grid (the other cases)
    B, D, H, W = {"gauss": (2, 64, 24, 32), "row_scales": (1, 96, 20, 24), "train": (1, 256, 36, 48),
                  "dsec": (1, 256, 60, 80)}[case]
    N = H * W
    f1, f2 = prng.gauss(171, (B, D, H, W)), prng.gauss(172, (B, D, H, W))
    gc = prng.gauss(173, (B * N, N))
    if case == "row_scales":  # dC rows and columns over 1e-6..1e6, feature rows over 1e-3..1e3
        gc *= (10.0 ** ((prng.uniform(174, (B * N, 1)) - 0.5) * 12)).astype(np.float32)
        gc *= (10.0 ** ((prng.uniform(175, (1, N)) - 0.5) * 12)).astype(np.float32)
        f1 *= (10.0 ** ((prng.uniform(176, (B, D, 1, 1)) - 0.5) * 6)).astype(np.float32)
        f2 *= (10.0 ** ((prng.uniform(177, (B, D, 1, 1)) - 0.5) * 6)).astype(np.float32)
    d1, d2, m1, m2 = _bwd_fp64(gc, f1, f2)
    tg, t1, t2 = (torch.from_numpy(x).to(DEV) for x in (gc, f1, f2))
    out = {algo: [g.cpu().numpy().reshape(B, D, N).astype(np.float64) for g in _lib.build_bwd(tg, t1, t2, algo)]
           for algo in (_lib.BUILD_BF16X6, _lib.BUILD_FP32)}
    u = 2.0 ** -24
    for k, (ref, mag) in enumerate(((d1, m1), (d2, m2))):
        bf, f32 = out[_lib.BUILD_BF16X6][k], out[_lib.BUILD_FP32][k]
        assert np.isfinite(bf).all()
        K = N
        bound = (3 + 6 * ((K + 15) // 16) + 16) * u * mag
        assert (np.abs(bf - ref) <= bound).all(), (k, (np.abs(bf - ref) / np.maximum(bound, 1e-300)).max())
        e_bf = np.abs(bf - ref).max(axis=2).ravel()
        e_32 = np.abs(f32 - ref).max(axis=2).ravel()
        scale = np.abs(ref).max(axis=2).ravel()
        ok = scale > 0
        rb, r32 = e_bf[ok] / scale[ok], e_32[ok] / scale[ok]
        print(f"{case} dF{k + 1}: bf16x6 row error max {rb.max():.3e} mean {rb.mean():.3e}; "
              f"fp32 max {r32.max():.3e} mean {r32.mean():.3e}")
        dom = float(np.mean(e_bf <= e_32 + scale * 2.0 ** -23))
        print(f"  rows at or below fp32's (+1 ulp): {dom:.3f}")
        assert rb.max() <= r32.max() and rb.mean() <= r32.mean()


@pytest.mark.parametrize("D,H,W", [(16, 8, 12), (32, 8, 12), (64, 32, 48)])
def test_build_bwd_bf16x6_inf_matches_fp32(D, H, W):
    """Non-finite inputs of the bf16x6 backward GEMMs give the fp32 reference's results
    (include/corr_mi355x.h, corr_build_bwd_ex): the split makes every output an infinite element
    reaches NaN (inf * 0 pieces), and the split-K reduces recompute exactly those as the
    reference does, so +-inf land where the fp32-operand GEMMs put them and NaN (inf * 0 in the
    fp32 sum, a NaN element) stays NaN.  Shapes: D 16 (one split, sqrt(D) a power of two), D 32
    (one split, the reduce kernel / dF2's tail), D 64 at 32x48 (split-K).
    Every finite output matches the fp32-operand GEMMs within 1e-6 of the scale."""
    from eraft_amd import _lib
    B = 1
    N = H * W
    f1, f2 = prng.gauss(181, (B, D, H, W)), prng.gauss(182, (B, D, H, W))
    gc = prng.gauss(183, (B * N, N))
    gc[5, 17] = np.inf     # +inf in dC: dF1 column 5, dF2 column 17
    gc[9, 3] = -np.inf     # -inf
    f2[0, 2].flat[17] = 0  # F2[2][17] = 0 meets dC[5][17] = inf: fp32 gives NaN at dF1[2][5]
    gc[20, 40] = np.nan    # a NaN element: NaN outputs as in fp32
    f1[0, 3].flat[30] = np.inf  # an infinite feature: dF2 row 3
    tg, t1, t2 = (torch.from_numpy(x).to(DEV) for x in (gc, f1, f2))
    d1, d2 = (g.cpu().numpy().reshape(B, D, N) for g in _lib.build_bwd(tg, t1, t2, _lib.BUILD_BF16X6))
    e1, e2 = (g.cpu().numpy().reshape(B, D, N) for g in _lib.build_bwd(tg, t1, t2, _lib.BUILD_FP32))
    for a, b in ((d1, e1), (d2, e2)):
        assert np.isnan(b).any() and np.isposinf(b).any() and np.isneginf(b).any()
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert np.array_equal(np.isposinf(a), np.isposinf(b)) and np.array_equal(np.isneginf(a), np.isneginf(b))
        ok = np.isfinite(b)
        assert np.abs(a[ok] - b[ok]).max() <= 1e-6 * np.abs(b[ok]).max()
    assert np.isnan(d1[0, 2, 5])  # inf * 0 in the fp32 sum


def _bf16_to_f32(u16):
    return (u16.astype(np.uint32) << 16).view(np.float32)


def test_bf16x6_pack_is_exact_split():
    """The bf16x6 operand pack (CORR_BUILD_ONLY_PACK) writes every fp32 feature as three bf16
    pieces whose sum is the feature EXACTLY (checked in fp64, bit for bit), hi = bf16_rn(x), and
    the special values as documented: +-inf -> (inf, 0, 0), NaN -> NaN hi, |x| near FLT_MAX ->
    a finite truncated hi, fp32 subnormals -> within the bf16 subnormal floor.  Padding is zero."""
    from eraft_amd import _lib
    B, D, H, W = 2, 40, 9, 21
    f1 = prng.gauss(41, (B, D, H, W)) * np.float32(3.0)
    f2 = prng.gauss(42, (B, D, H, W)) * np.float32(1e-20)
    sp = np.array([np.inf, -np.inf, np.nan, 3.4028235e38, -3.3961e38, 3.3895e38, 1e-40, -3e-39, 1.2e-38,
                   0.0, -0.0, 1.0 + 2.0 ** -23, 2.0 ** -100, 65504.0, 1e30], np.float32)
    f1.reshape(-1)[7:7 + sp.size] = sp
    f2.reshape(-1)[100:100 + sp.size] = sp
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    ws = _lib.build_workspace(t1, t2, _lib.BUILD_BF16X6)
    ws.fill_(0xAB)
    lvl = tiled_levels(B, H, W, 1, DEV)
    _lib.build(t1, t2, lvl, _lib.BUILD_BF16X6 | _lib.BUILD_ONLY_PACK, ws)
    w = ws.cpu().numpy()
    N, S = H * W, (D + 31) // 32
    NQp = (N + 127) // 128 * 128
    Hp, CB = (H + 7) // 8 * 8, (W + 15) // 16
    nq = B * S * NQp * 192
    toff = (nq + 255) // 256 * 256
    # record layout: [piece 3][grp 4][ci 16][j 8] bf16; k = 32 s + 8 grp + j
    q = w[:nq].view(np.uint16).reshape(B, S, NQp // 16, 3, 4, 16, 8)
    q = _bf16_to_f32(q).transpose(0, 3, 1, 4, 6, 2, 5).reshape(B, 3, S * 32, NQp)
    # target records are 4x4 tiles (tile row ty, tile column tx of 4 CB per row), pixel ci at
    # (4 ty + ci // 4, 4 tx + ci % 4)
    t = w[toff:toff + B * S * Hp * CB * 16 * 192].view(np.uint16).reshape(B, S, Hp // 4, 4 * CB, 3, 4, 4, 4, 8)
    t = _bf16_to_f32(t).transpose(0, 4, 1, 5, 8, 2, 6, 3, 7).reshape(B, 3, S * 32, Hp, CB * 16)
    for img, x in ((q[..., :N].reshape(B, 3, S * 32, H, W), f1), (t[..., :H, :W], f2)):
        hi, mid, lo = (img[:, c, :D] for c in range(3))
        fin = np.isfinite(x)
        big = fin & (np.abs(x) >= 2.0 ** -100)
        tot = hi.astype(np.float64) + mid + lo
        assert np.array_equal(tot[big], x[big].astype(np.float64))
        assert np.all(np.abs(tot[fin] - x[fin]) <= 2.0 ** -133)
        rn = torch.from_numpy(x).to(torch.bfloat16).float().numpy()
        okrn = big & np.isfinite(rn)
        assert np.array_equal(hi[okrn].view(np.uint32), rn[okrn].view(np.uint32))
        inf = np.isinf(x)
        assert np.array_equal(hi[inf], x[inf]) and (mid[inf] == 0).all() and (lo[inf] == 0).all()
        assert np.isnan(hi[np.isnan(x)]).all()
        assert np.isfinite(hi[fin]).all()
        # padding (k >= D, pixels past the map) is zero
        assert (img[:, :, D:] == 0).all()
    assert (q[..., N:] == 0).all() and (t[..., H:, :] == 0).all() and (t[..., W:] == 0).all()


@pytest.mark.parametrize("algo_name", ["BUILD_BF16X6", "LOOKUP_CONV"])
def test_bf16x6_infinite_features_match_fp32(algo_name):
    """Infinite features through the three-piece split: +-inf splits as (inf, 0, 0), so the small
    piece products hold inf * 0 = NaN; the result keeps the leading hi*hi sum when that is infinite
    (corr_common.h split_sum), giving fp32's inf where fp32 gives inf, and NaN exactly where fp32
    gives NaN (inf * 0 against a zero feature, opposite infinities).  Checked against the
    fp32-operand build on the full 4-level pyramid: same NaN cells, same infinities with the same
    signs, finite cells within 1e-5 of the row scale.  LOOKUP_CONV: the fused lookup + 1x1 conv,
    whose corr operand then holds the infinities, against the plain lookup + an fp64 conv."""
    from eraft_amd import _lib
    B, D, H, W, L = 1, 64, 16, 24, 4
    f1, f2 = prng.gauss(61, (B, D, H, W)), prng.gauss(62, (B, D, H, W))
    f1[0, 3, 0, 5] = np.inf
    f1[0, 10, 2, 7] = -np.inf
    f1[0, 20, 5, 5] = np.inf
    f1[0, 21, 5, 5] = -np.inf        # pixel (5,5): opposite infinities against any nonzero pair
    if algo_name == "BUILD_BF16X6":
        f2[0, 3, 4, 4] = 0.0         # inf * 0 for query (0,5) at target (4,4)
        f2[0, 10, 1, 1] = np.inf     # -inf * inf for query (2,7) at (1,1)
        f2[0, 3, 9, 9] = -np.inf     # inf * -inf for query (0,5) at (9,9)
    else:
        # one-signed infinite rows for the conv: query (0,5) +inf, (2,7) -inf, (5,5) NaN everywhere
        for c in (3, 10, 20, 21):
            f2[0, c] = np.abs(f2[0, c]) + np.float32(0.1)
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    out = {}
    for algo in (_lib.BUILD_BF16X6, _lib.BUILD_FP32):
        lv = tiled_levels(B, H, W, L, DEV)
        _lib.build(t1, t2, lv, algo)
        out[algo] = lv
    if algo_name == "BUILD_BF16X6":
        pairs = zip(export_levels(out[_lib.BUILD_BF16X6], H, W), export_levels(out[_lib.BUILD_FP32], H, W))
        got = [(a.reshape(B * H * W, -1), b.reshape(B * H * W, -1)) for a, b in pairs]
    else:
        # the fused lookup's corr operand is the bf16x6 pyramid split again: feed it the fp32 build
        # (same infinities) and compare with the unfused lookup + fp64 conv
        r = 4
        C = L * (2 * r + 1) ** 2
        coords = torch.from_numpy(prng.lookup_coords(63, B, H, W, 3.0)).to(DEV)
        # positive weights keep the +-inf lookups infinite through the conv (mixed signs: NaN);
        # the weights' mid / lo pieces are nonzero, so the small products meet inf * lo terms
        w = torch.from_numpy(np.abs(prng.gauss(64, (256, C), 0.05)) + np.float32(1e-3)).to(DEV)
        bias = torch.from_numpy(prng.gauss(65, (256,), 0.1)).to(DEV)
        lk = torch.empty(B, C, H, W, device=DEV)
        _lib.lookup(out[_lib.BUILD_FP32], coords, r, lk)
        lk = lk.cpu().numpy().astype(np.float64)
        assert np.isinf(lk).any()
        with np.errstate(invalid="ignore"):
            ref = np.einsum("oc,bchw->bohw", w.cpu().numpy().astype(np.float64), lk)
        ref = ref + bias.cpu().numpy()[None, :, None, None]
        fused = torch.empty(B, 256, H, W, device=DEV)
        _lib.lookup_conv(out[_lib.BUILD_FP32], coords, r, _lib.lookup_conv_weights(w), bias, fused, relu=False)
        fused = fused.cpu().numpy()
        got = [(fused.reshape(256, -1).T, ref.astype(np.float32).reshape(256, -1).T)]
    for a, b in got:
        assert np.array_equal(np.isnan(a), np.isnan(b))
        inf = np.isinf(b)
        assert inf.any() and np.array_equal(np.isinf(a), inf) and np.array_equal(a[inf], b[inf])
        fin = np.isfinite(b)
        scale = np.where(fin, np.abs(b), 0).max(axis=1, keepdims=True)
        assert (np.abs(np.where(fin, a, 0) - np.where(fin, b, 0)) <= 1e-5 * scale + 1e-30).all()


def test_lookup_nan_and_inf_coords():
    B, D, H, W, L, r = 1, 16, 16, 16, 3, 4
    f1, f2 = prng.gauss(1, (B, D, H, W)), prng.gauss(2, (B, D, H, W))
    cb = _cb()(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    c = prng.lookup_coords(3, B, H, W, 2.0)
    c[0, 0, 0, :4] = [np.nan, np.inf, -np.inf, 3.0e38]
    c[0, 1, 1, :3] = [np.nan, -np.inf, 1e30]
    gpu = [p.cpu().numpy() for p in cb.corr_pyramid]
    assert bit_equal(cb(torch.from_numpy(c).to(DEV)).cpu().numpy(), oracle.lookup(gpu, c, r))


@pytest.mark.parametrize("kind", ["random", "grid", "huge"])
@pytest.mark.parametrize("B,D,H,W,L,r", [(2, 16, 18, 24, 4, 4), (1, 8, 17, 23, 3, 3), (1, 256, 60, 80, 4, 4)])
def test_lookup_bwd_bitexact_vs_oracle(B, D, H, W, L, r, kind):
    """One lookup's input-gradient from a zeroed pyramid: same tap / corner order as the
    oracle -> bit-identical; then the avg-pool backward fold, also bit-identical.
    kind: random coords (regular taps: closed-form gather), the integer pixel grid (the
    cold-start first iteration; tap floors jitter -> general range gather), and a few
    coordinates near 2^20 (taps outside the neighbourhood -> sequential scatter path)."""
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    K = (2 * r + 1) ** 2
    c = prng.lookup_coords(5, B, H, W, 3.0)
    if kind == "grid":
        ys, xs = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
        c[:, 0], c[:, 1] = xs, ys
        c[:, :, 1::3, ::2] += np.float32(0.5)
    elif kind == "huge":
        c[0, 0, 1, :3] = [1048000.5, -1048001.25, 1048575.0]
        c[0, 1, 2, :2] = [1047999.75, 3.0]
    c[0, :, 0, :3] = np.float32(np.nan)  # NaN coords contribute nothing
    go = prng.gauss(6, (B, L * K, H, W))
    ref = oracle.lookup_bwd(c, go, [np.zeros((B * H * W, 1, h, w), np.float32)
                                    for h, w in oracle.level_shapes(H, W, L)], r)
    like = torch.empty(1, device=DEV)
    gl = _alloc_grad_pyramid(B, H, W, L, like, zero=True)
    _lib.lookup_bwd(torch.from_numpy(c).to(DEV), torch.from_numpy(go).to(DEV), r, gl)
    for l in range(L):
        assert bit_equal(gl[l].cpu().numpy(), ref[l]), l
    oracle.pool_bwd(ref, H, W)
    _lib.pool_bwd(gl, H, W)
    for l in range(L):
        assert bit_equal(gl[l].cpu().numpy(), ref[l]), l


@pytest.mark.parametrize("T", [0, 1, 3, 12, 40])
@pytest.mark.parametrize("B,H,W,L,r", [(2, 18, 24, 4, 4), (1, 17, 23, 3, 3)])
def test_lookup_bwd_multi_and_fold_bitexact(T, B, H, W, L, r):
    """corr_lookup_bwd_multi (all lookups in one launch, chunks of 32, overwriting the pyramid)
    == zero + corr_lookup_bwd per lookup, bit for bit; corr_pool_fold's level 0 == corr_pool_bwd's."""
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    like = torch.empty(1, device=DEV)
    cs, gs = _bwd_case(T, B, H, W, L, r, 700)
    ref = _alloc_grad_pyramid(B, H, W, L, like, zero=True)
    for c, g in zip(cs, gs):
        _lib.lookup_bwd(c, g, r, ref)
    got = _alloc_grad_pyramid(B, H, W, L, like)
    for p in got:
        p.fill_(float("nan"))  # the multi-lookup kernel must overwrite every cell
    if T:
        _lib.lookup_bwd_multi(cs, gs, r, got)
    else:
        _lib.lookup_bwd_multi([torch.zeros(B, 2, H, W, device=DEV)], [torch.zeros(B, L * (2 * r + 1) ** 2, H, W,
                              device=DEV)], r, got)
    for l in range(L):
        assert bit_equal(got[l].cpu().numpy(), ref[l].cpu().numpy()), l
    _lib.pool_bwd(ref, H, W)
    _lib.pool_fold(got, B, H, W)
    assert bit_equal(got[0].cpu().numpy(), ref[0].cpu().numpy())


@pytest.mark.parametrize("exact", [True, False])
@pytest.mark.parametrize("algo", ["bf16x6", "f16x3", "fp32"])
@pytest.mark.parametrize("B,D,H,W,L,r,T", [(2, 32, 18, 24, 4, 4, 5), (1, 20, 17, 23, 3, 3, 2), (1, 16, 17, 23, 4, 4, 3),
                                           (8, 64, 36, 48, 4, 4, 12),
                                           # the lean fold's edges: odd H (last level-0 row unpooled), W / 4 odd
                                           # (last level-2 column unpooled), W / 8 = 2
                                           (2, 16, 17, 20, 4, 4, 4),
                                           (1, 16, 12, 16, 4, 4, 33), (1, 16, 60, 80, 4, 4, 3),
                                           (1, 16, 64, 96, 5, 2, 2), (1, 8, 120, 160, 4, 4, 2)])
def test_corr_backward_matches_staged_path(algo, B, D, H, W, L, r, T, exact):
    """corr_backward against the staged path (lookup_bwd per lookup, pool_bwd, build_bwd with its
    own absmax).  Covers the fused LDS-resident kernel, whose query count per workgroup depends on
    the radius alone (FusedStage<S>::BQ: 4 at r = 4, 8 at r = 2 and 3), up to 60x80, and the
    multi-lookup + fold fallback (33 lookups > one launch's table; 5 levels; 120x160, whose
    workgroup image exceeds the 160 KiB of LDS), and a ragged last query group (17x23 at r = 4: the
    quad-transposed gradient loads of a partial group).  exact (CORR_BACKWARD_EXACT_FOLD):
    bit-identical.  Default: the fused fold's separable closed form at r = 4 (the same per-tap
    weights, another rounding order): dC within 1e-6 norm-relative of the staged path (the
    verdict's bar; seen ~1e-7) and within the per-cell bound of _util.within_cell_bound (norm_rel
    alone cannot see a wrong cell below 1e-6 of the largest; at 120x160, whose dC is 1.5 GB, the
    fallback's dC is bit-identical instead), and dfmap1 / dfmap2 within 1e-6; the other radii and the
    fallback stay bit-identical."""
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    f1 = torch.from_numpy(prng.gauss(61, (B, D, H, W))).to(DEV)
    f2 = torch.from_numpy(prng.gauss(62, (B, D, H, W))).to(DEV)
    cs, gs = _bwd_case(T, B, H, W, L, r, 800)
    ref = _alloc_grad_pyramid(B, H, W, L, f1, zero=True)
    for c, g in zip(cs, gs):
        _lib.lookup_bwd(c, g, r, ref)
    _lib.pool_bwd(ref, H, W)
    r1, r2 = _lib.build_bwd(ref[0].reshape(B * H * W, H * W), f1, f2, _lib._ALGOS[algo])
    got = _alloc_grad_pyramid(B, H, W, L, f1)
    g1, g2 = _lib.backward(cs, gs, r, got, f1, f2, _lib._ALGOS[algo], exact=exact)
    pairs = ((got[0], ref[0]), (g1, r1), (g2, r2))
    if exact or r != 4 or T > 32 or L > 4:
        for a, b in pairs:
            assert bit_equal(a.cpu().numpy(), b.cpu().numpy())
    else:
        for k, (a, b) in enumerate(pairs):
            e = norm_rel(a.cpu().numpy(), b.cpu().numpy())
            print(f"{'dC dF1 dF2'.split()[k]}: {e:.2e}")
            assert e <= 1e-6, (k, e)
        if H * W <= 60 * 80:
            M = _bwd_case_magnitude(T, B, H, W, L, r, 800)
            a, b = got[0].cpu().numpy(), ref[0].cpu().numpy()
            print(f"dC: max |a - b| / (2^-24 M) = {cell_ratio(a, b, M):.3f} (k = {cell_bound_k(T, L)})")
            assert within_cell_bound(a, b, M, T, L)
        else:  # the staged fallback: identical words pass the bound whatever M is (compared on the GPU)
            assert torch.equal(got[0].view(torch.int32), ref[0].view(torch.int32))


@pytest.mark.parametrize("exact", [True, False])
def test_corr_backward_infinite_upstream_gradients(exact):
    """Infinite upstream gradients (on regular, integer-grid and far windows) give dC the staged
    path's inf / NaN cells exactly — the separable fold's general form for irregular windows
    multiplies every candidate tap, so a wave holding a non-finite gradient replays its irregular
    windows by the range form instead — and its finite cells within 1e-6 (bit-identical when
    exact)."""
    from eraft_amd import _lib
    from eraft_amd.corr import _alloc_grad_pyramid
    B, D, H, W, L, r, T = 2, 16, 18, 24, 4, 4, 3
    f1 = torch.from_numpy(prng.gauss(63, (B, D, H, W))).to(DEV)
    f2 = torch.from_numpy(prng.gauss(64, (B, D, H, W))).to(DEV)
    cs, gs = _bwd_case(T, B, H, W, L, r, 820)
    K = (2 * r + 1) ** 2
    for t, g in enumerate(gs):  # +inf at a few (tap, query) points of each lookup, every level
        for l in range(L):
            g[0, l * K + (7 * t + 3) % K, 5, 7 + t] = float("inf")
            g[1, l * K + 40, 11, 3 * t] = float("inf")
    ref = _alloc_grad_pyramid(B, H, W, L, f1, zero=True)
    for c, g in zip(cs, gs):
        _lib.lookup_bwd(c, g, r, ref)
    _lib.pool_bwd(ref, H, W)
    got = _alloc_grad_pyramid(B, H, W, L, f1)
    _lib.backward(cs, gs, r, got, f1, f2, _lib._ALGOS["bf16x6"], exact=exact)
    a, b = got[0].cpu().numpy(), ref[0].cpu().numpy()
    assert np.isnan(b).any() and np.isinf(b).any()
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isposinf(a), np.isposinf(b))
    assert np.array_equal(np.isneginf(a), np.isneginf(b))
    fin = np.isfinite(b)
    if exact:
        assert bit_equal(a[fin], b[fin])
    else:
        assert norm_rel(a[fin], b[fin]) <= 1e-6


def test_lookup_only_loss_runs_one_backward_call(monkeypatch):
    """a loss that reaches the pyramid only through lookups makes no zero-filled
    pyramid gradient (materialize_grads off) and no per-lookup kernel: the build's backward is
    ONE corr_backward call (and nothing of the staged path)."""
    from eraft_amd import _lib
    calls = {"backward": 0, "lookup_bwd": 0, "pool_bwd": 0, "build_bwd": 0}
    for name in calls:
        orig = getattr(_lib, name)

        def spy(*a, _o=orig, _n=name, **k):
            calls[_n] += 1
            return _o(*a, **k)
        monkeypatch.setattr(_lib, name, spy)
    monkeypatch.setenv("ERAFT_AMD_FUSED_BWD", "1")
    B, D, H, W, L, r = 2, 32, 24, 32, 4, 4
    t1 = torch.from_numpy(prng.gauss(91, (B, D, H, W))).to(DEV).requires_grad_(True)
    t2 = torch.from_numpy(prng.gauss(92, (B, D, H, W))).to(DEV).requires_grad_(True)
    cb = _cb()(t1, t2, L, r)
    cs, gs = _bwd_case(4, B, H, W, L, r, 950)
    sum((cb(c) * g).sum() for c, g in zip(cs, gs)).backward()
    assert calls == {"backward": 1, "lookup_bwd": 0, "pool_bwd": 0, "build_bwd": 0}, calls
    assert t1.grad is not None and t2.grad is not None


def test_autograd_separable_fold_close_to_per_lookup(monkeypatch):
    """CorrBlock autograd with the default fused fold (separable closed form) against the
    per-lookup path (ERAFT_AMD_FUSED_BWD=0, the reference's scatter order): fmap gradients within
    1e-6 norm-relative at the train shape's width (36x48, 12 lookups, the first on the integer
    grid as at a cold start); and the dC that each path hands to its GEMMs (corr_backward's level
    0, build_bwd's argument) within the per-cell bound of _util.within_cell_bound."""
    from eraft_amd import _lib
    B, D, H, W, L, r, T = 2, 64, 36, 48, 4, 4, 12
    f1n, f2n = prng.gauss(73, (B, D, H, W)), prng.gauss(74, (B, D, H, W))
    cs, gs = _bwd_case(T, B, H, W, L, r, 910)
    res, dc = {}, {}
    fused, staged = _lib.backward, _lib.build_bwd

    def spy_backward(coords_list, grad_list, radius, grad_levels, *a, **k):
        out = fused(coords_list, grad_list, radius, grad_levels, *a, **k)
        dc["1"] = grad_levels[0].cpu().numpy()
        return out

    def spy_build_bwd(grad_c, *a, **k):
        dc["0"] = grad_c.cpu().numpy()
        return staged(grad_c, *a, **k)
    monkeypatch.setattr(_lib, "backward", spy_backward)
    monkeypatch.setattr(_lib, "build_bwd", spy_build_bwd)
    monkeypatch.setenv("ERAFT_AMD_EXACT_FOLD", "0")
    for mode in ("1", "0"):
        monkeypatch.setenv("ERAFT_AMD_FUSED_BWD", mode)
        t1 = torch.from_numpy(f1n).to(DEV).requires_grad_(True)
        t2 = torch.from_numpy(f2n).to(DEV).requires_grad_(True)
        cb = _cb()(t1, t2, L, r)
        sum((cb(c) * g).sum() for c, g in zip(cs, gs)).backward()
        res[mode] = (t1.grad.cpu().numpy(), t2.grad.cpu().numpy())
    for k, (a, b) in enumerate(zip(res["1"], res["0"])):
        e = norm_rel(a, b)
        print(f"dF{k + 1}: {e:.2e}")
        assert e <= 1e-6, (k, e)
    assert sorted(dc) == ["0", "1"] and dc["1"].shape == dc["0"].shape
    M = _bwd_case_magnitude(T, B, H, W, L, r, 910)
    print(f"dC: max |a - b| / (2^-24 M) = {cell_ratio(dc['1'], dc['0'], M):.3f} (k = {cell_bound_k(T, L)})")
    assert within_cell_bound(dc["1"], dc["0"], M, T, L)


def test_autograd_fused_backward_equals_per_lookup(monkeypatch):
    """CorrBlock autograd: the stash + corr_backward path with the bit-exact fold
    (ERAFT_AMD_EXACT_FOLD=1) and ERAFT_AMD_FUSED_BWD=0's per-lookup path give bit-identical fmap
    gradients, also when a direct pyramid gradient is present."""
    B, D, H, W, L, r = 2, 32, 24, 32, 4, 4
    f1n, f2n = prng.gauss(71, (B, D, H, W)), prng.gauss(72, (B, D, H, W))
    cs, gs = _bwd_case(6, B, H, W, L, r, 900)
    res = {}
    monkeypatch.setenv("ERAFT_AMD_EXACT_FOLD", "1")  # the fused fold's bit-exact replay
    for mode in ("1", "0"):
        for direct in (False, True):
            monkeypatch.setenv("ERAFT_AMD_FUSED_BWD", mode)
            t1 = torch.from_numpy(f1n).to(DEV).requires_grad_(True)
            t2 = torch.from_numpy(f2n).to(DEV).requires_grad_(True)
            cb = _cb()(t1, t2, L, r)
            loss = sum((cb(c) * g).sum() for c, g in zip(cs, gs))
            if direct:
                loss = loss + cb.corr_pyramid[2].square().sum()
            loss.backward()
            res[mode, direct] = (t1.grad.cpu().numpy(), t2.grad.cpu().numpy())
    for direct in (False, True):
        for a, b in zip(res["1", direct], res["0", direct]):
            assert bit_equal(a, b), direct


@pytest.mark.parametrize("B,D,H,W", [(1, 256, 60, 80), (2, 200, 16, 24), (2, 32, 18, 24), (1, 20, 17, 23), (8, 16, 12, 16)])
@pytest.mark.parametrize("algo", ["bf16x6", "f16x3", "fp32"])
@pytest.mark.parametrize("spread", [False, True])
def test_build_bwd_vs_oracle(B, D, H, W, algo, spread):
    """Backward GEMMs (both algorithms) vs the fp64-accumulating oracle.  spread: rows and
    columns of dC and the fmap rows scaled over 1e-6..1e6 (the f16 split rescales per row /
    column; the norm-relative bar is the north_star's 1e-4)."""
    from eraft_amd import _lib
    N = H * W
    f1, f2 = prng.gauss(11, (B, D, H, W)), prng.gauss(12, (B, D, H, W))
    gc = prng.gauss(13, (B * N, N))
    if spread:
        gc *= (10.0 ** ((prng.uniform(14, (B * N, 1)) - 0.5) * 12)).astype(np.float32)
        gc *= (10.0 ** ((prng.uniform(15, (1, N)) - 0.5) * 6)).astype(np.float32)
        f1 *= (10.0 ** ((prng.uniform(16, (B, D, 1, 1)) - 0.5) * 6)).astype(np.float32)
    if B * N * N * D > 3e9:
        pytest.skip("oracle too slow")
    d1, d2 = oracle.corr_bwd(gc.reshape(B * N, 1, H, W), f1, f2)
    g1, g2 = _lib.build_bwd(torch.from_numpy(gc).to(DEV), torch.from_numpy(f1).to(DEV),
                            torch.from_numpy(f2).to(DEV), _lib._ALGOS[algo])
    assert norm_rel(g1.cpu().numpy(), d1) < REL_TOL
    assert norm_rel(g2.cpu().numpy(), d2) < REL_TOL


@pytest.mark.parametrize("algo,tiny", [("f16x3", 1e-36), ("bf16x6", 1e-30), ("bf16x6", 1e150)])
def test_build_bwd_special_rows_vs_oracle(algo, tiny):
    """Special rows through the backward GEMMs.  f16x3: waves that stage a row whose max is below
    2^-112 (shift > 127: 2^s is not a float, so the split keeps ldexp) or whose max is inf (the
    lo-half guard) take the exact staging path; the others the fast one-multiply split.
    bf16x6: no scales at all — dC rows / columns and feature rows at 1e-30 (above the split's
    absolute floor of ~2^-110, where `lo` would leave the bf16 subnormal range), or (tiny > 1)
    dC rows / columns at 1e18 with feature rows at 1e-20.  One inf and a few NaN entries in dC,
    against the fp64 oracle: the same non-finite
    pattern, and every finite output column / row within 1e-5 of its OWN scale (so the tiny
    outputs are checked, not hidden under the global max)."""
    from eraft_amd import _lib
    B, D, H, W = 1, 64, 12, 16
    N = H * W
    f1, f2 = prng.gauss(21, (B, D, H, W)), prng.gauss(22, (B, D, H, W))
    gc = prng.gauss(23, (B * N, N))
    sg, sf = (np.float32(tiny), np.float32(tiny)) if tiny < 1 else (np.float32(1e18), np.float32(1e-20))
    gc[[5, 77, 150]] *= sg                    # scaled dC rows (dF1 columns)
    gc[:, [9, 100]] *= sg                     # scaled dC columns (dF2 columns)
    f1[0, 3] *= sf                            # scaled feature rows of both operands
    f2[0, 7] *= sf
    gc[40, 60] = np.float32(np.inf)
    gc[120, [3, 4]] = np.float32(np.nan)
    d1, d2 = oracle.corr_bwd(gc.reshape(B * N, 1, H, W), f1, f2)
    g1, g2 = _lib.build_bwd(torch.from_numpy(gc).to(DEV), torch.from_numpy(f1).to(DEV),
                            torch.from_numpy(f2).to(DEV), _lib._ALGOS[algo])
    g1, g2 = g1.cpu().numpy().reshape(D, N), g2.cpu().numpy().reshape(D, N)
    r1, r2 = np.asarray(d1).reshape(D, N), np.asarray(d2).reshape(D, N)
    for got, ref in ((g1, r1), (g2, r2)):
        assert np.array_equal(np.isfinite(got), np.isfinite(ref))
        fin = np.isfinite(ref)
        ref_f, got_f = np.where(fin, ref, 0.0), np.where(fin, got.astype(np.float64), 0.0)
        for axis in (0, 1):  # per output column (query / target pixel), then per feature row
            scale = np.abs(ref_f).max(axis=axis)
            err = np.abs(got_f - ref_f).max(axis=axis)
            ok = (scale == 0) | (err <= 1e-5 * scale)
            assert ok.all(), (axis, np.flatnonzero(~ok)[:8], (err / np.maximum(scale, 1e-300)).max())


def test_training_shape_backward_vs_oracle():
    """BASELINE config 4 shape (36x48 fmaps), B and D reduced so the C oracle stays fast."""
    B, D, H, W, L, r = 2, 32, 36, 48, 4, 4
    f1, f2 = prng.gauss(21, (B, D, H, W)), prng.gauss(22, (B, D, H, W))
    K = (2 * r + 1) ** 2
    cs = [prng.lookup_coords(30 + t, B, H, W, 1.0 + t) for t in range(4)]
    gs = [prng.gauss(40 + t, (B, L * K, H, W)) for t in range(4)]
    d1, d2 = oracle.fmap_grads(f1, f2, cs, gs, L, r)
    t1 = torch.from_numpy(f1).to(DEV).requires_grad_(True)
    t2 = torch.from_numpy(f2).to(DEV).requires_grad_(True)
    cb = _cb()(t1, t2, L, r)
    loss = sum((cb(torch.from_numpy(c).to(DEV)) * torch.from_numpy(g).to(DEV)).sum() for c, g in zip(cs, gs))
    loss.backward()
    assert norm_rel(t1.grad.cpu().numpy(), d1) < REL_TOL
    assert norm_rel(t2.grad.cpu().numpy(), d2) < REL_TOL


def test_determinism():
    B, D, H, W = 1, 64, 24, 32
    f1 = torch.from_numpy(prng.gauss(1, (B, D, H, W))).to(DEV).requires_grad_(True)
    f2 = torch.from_numpy(prng.gauss(2, (B, D, H, W))).to(DEV).requires_grad_(True)
    c = torch.from_numpy(prng.lookup_coords(3, B, H, W, 5.0)).to(DEV)
    res = []
    for _ in range(2):
        f1.grad = f2.grad = None
        cb = _cb()(f1, f2)
        o = cb(c)
        (o * o).sum().backward()
        res.append((o.detach().cpu().numpy(), f1.grad.cpu().numpy(), f2.grad.cpu().numpy()))
    for a, b in zip(res[0], res[1]):
        assert bit_equal(a, b)


def test_errors_fail_loudly():
    CB = _cb()
    f = torch.zeros(1, 8, 16, 16)
    with pytest.raises(RuntimeError):
        CB(f, f)  # CPU tensors: no fallback
    g = torch.zeros(1, 8, 8, 8, device=DEV)
    with pytest.raises(RuntimeError):
        CB(g[:, :, :1, :], g[:, :, :1, :], num_levels=4)  # too small for 4 levels
    cb = CB(g, g, num_levels=2)
    with pytest.raises(ValueError):
        cb(torch.zeros(1, 2, 4, 4, device=DEV))


def _splat_flows():
    g = load("g_splat")
    cases = [(g[f"flow_{t}"], g[f"splat_{t}"]) for t in "ab"]
    e = load("g_e2e_dsec")
    cases.append((e["low"], e["flow_init"]))
    return cases


def test_forward_splat_bitexact_vs_reference_golden():
    """corr_forward_splat vs the reference's own forward_interpolate_pytorch outputs."""
    from eraft_amd import forward_interpolate_pytorch
    for flow, ref in _splat_flows():
        out = forward_interpolate_pytorch(torch.from_numpy(flow).to(DEV))
        assert bit_equal(out.cpu().numpy(), ref)


@pytest.mark.parametrize("B,H,W,sigma", [(3, 36, 48, 2.0), (1, 120, 160, 8.0), (2, 7, 5, 30.0)])
def test_forward_splat_bitexact_vs_oracle(B, H, W, sigma):
    """Random flows (dense collisions at sigma 2, far-out points at sigma 30) + integer and NaN
    displacements, repeat runs identical (no float atomics)."""
    from eraft_amd import forward_interpolate_pytorch
    f = prng.gauss(41, (B, 2, H, W), sigma)
    f[:, :, ::3, ::2] = np.round(f[:, :, ::3, ::2])
    f[0, :, 0, :2] = np.float32(np.nan)
    t = torch.from_numpy(f).to(DEV)
    out = forward_interpolate_pytorch(t).cpu().numpy()
    assert bit_equal(out, oracle.forward_splat(f))
    assert bit_equal(forward_interpolate_pytorch(t).cpu().numpy(), out)


@pytest.mark.parametrize("N,h,w,scale", [(1, 60, 80, 1.0), (2, 7, 9, 30.0)])
def test_convex_upsample_vs_reference_formula(N, h, w, scale):
    """corr_convex_upsample vs the reference's upsample_flow composition (eraft.py:75-86)
    evaluated in float64 on the host: |diff| <= 1e-5 of max|out| (large logits: softmax
    saturation)."""
    import torch.nn.functional as F
    from eraft_amd import _lib
    flow = prng.gauss(51, (N, 2, h, w), 3.0)
    mask = prng.gauss(52, (N, 576, h, w), scale)
    f64, m64 = torch.from_numpy(flow).double(), torch.from_numpy(mask).double()
    m = torch.softmax(m64.view(N, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * f64, [3, 3], padding=1).view(N, 2, 9, 1, 1, h, w)
    ref = torch.sum(m * up, dim=2).permute(0, 1, 4, 2, 5, 3).reshape(N, 2, 8 * h, 8 * w).numpy()
    out = torch.empty(N, 2, 8 * h, 8 * w, device=DEV)
    _lib.convex_upsample(torch.from_numpy(flow).to(DEV), torch.from_numpy(mask).to(DEV), out)
    o = out.cpu().numpy()
    assert np.abs(o - ref).max() <= 1e-5 * np.abs(ref).max()


def test_voxel_grid_vs_reference_golden():
    """corr_voxel_grid vs the reference VoxelGrid.convert (utils/dsec_utils.py:26-64): raw grid
    bit-identical, normalised grid within 1e-6 of max|v|."""
    from eraft_amd import VoxelGrid
    g = load("g_voxel")
    for t in "ab":
        M, C, H, W = (int(v) for v in g[f"meta_{t}"])
        ev = {k: torch.from_numpy(g[f"ev_{t}"][i].copy()).to(DEV) for i, k in enumerate("xytp")}
        raw = VoxelGrid((C, H, W), normalize=False).convert(ev).cpu().numpy()
        assert bit_equal(raw, g[f"raw_{t}"]), t
        nrm = VoxelGrid((C, H, W), normalize=True).convert(ev).cpu().numpy()
        ref = g[f"norm_{t}"]
        assert np.abs(nrm - ref).max() <= 1e-6 * np.abs(ref).max(), t


def test_voxel_grid_tbilinear_vs_reference_golden():
    """corr_voxel_grid_tbilinear vs the reference EventSequenceToVoxelGrid_Pytorch
    (utils/transformers.py:18-126): raw grid bit-identical (incl. equal stamps -> deltaT = 1),
    normalised grid within 1e-6 of max|v|; through the drop-in class."""
    import types
    from eraft_amd import EventSequenceToVoxelGrid
    g = load("g_voxel_mvsec")
    for t in "abc":
        M, C, H, W = (int(v) for v in g[f"meta_{t}"])
        seq = types.SimpleNamespace(features=g[f"ev_{t}"], image_width=W, image_height=H)
        raw = EventSequenceToVoxelGrid(C, normalize=False)(seq).cpu().numpy()
        assert bit_equal(raw, g[f"raw_{t}"]), t
        nrm = EventSequenceToVoxelGrid(C, normalize=True)(seq).cpu().numpy()
        ref = g[f"norm_{t}"]
        assert np.abs(nrm - ref).max() <= 1e-6 * np.abs(ref).max(), t


def test_voxel_grid_tbilinear_mvsec_size_vs_oracle():
    """An MVSEC window (5 x 260 x 346, 200k events, unsorted tail, out-of-range bins, a hot
    pixel): raw grid bit-identical to the oracle, repeat runs identical, empty input -> zeros."""
    from eraft_amd import _lib
    M, C, H, W = 200000, 5, 260, 346
    u = prng.uniform(71, (4, M)).astype(np.float64)
    t = np.sort(u[2] * 50000.0)
    t[-100:] = t[-100:][::-1]            # a few out-of-order stamps (negative / late bins)
    t[:50] = t[0] - 10.0 * np.arange(50)
    ev = np.stack([t, np.floor(u[0] * W), np.floor(u[1] * H), (u[3] > 0.5).astype(np.float64)], 1)
    ev[::40, 1:3] = (7.0, 9.0)           # hot pixel
    ev = np.ascontiguousarray(ev)
    ref = oracle.voxel_grid_tbilinear(ev, C, H, W, False)
    te = torch.from_numpy(ev).to(DEV)
    outs = []
    for _ in range(2):
        o = torch.empty((C, H, W), device=DEV)
        _lib.voxel_grid_tbilinear(te, o, False)
        outs.append(o.cpu().numpy())
    assert bit_equal(outs[0], ref) and bit_equal(outs[1], ref)
    o = torch.full((C, H, W), 7.0, device=DEV)
    _lib.voxel_grid_tbilinear(torch.empty((0, 4), dtype=torch.float64, device=DEV), o, True)
    assert not o.cpu().numpy().any()


def test_voxel_grid_dsec_size_vs_oracle():
    """A DSEC-sized window (15 x 480 x 640, 300k events with hot pixels): raw grid
    bit-identical to the oracle, repeat runs identical."""
    from eraft_amd import VoxelGrid
    M, C, H, W = 300000, 15, 480, 640
    u = prng.uniform(61, (4, M))
    x = (u[0] * W).astype(np.float32)
    y = (u[1] * H).astype(np.float32)
    x[::50], y[::50] = 100.25, 200.5  # one hot pixel: a long bucket
    t = np.sort(u[2]).astype(np.float32)
    t = (t - t[0]) / (t[-1] - t[0])
    p = (u[3] > 0.5).astype(np.float32)
    ev_np = np.stack([x, y, t, p])
    ev = {k: torch.from_numpy(ev_np[i].copy()).to(DEV) for i, k in enumerate("xytp")}
    vg = VoxelGrid((C, H, W), normalize=False)
    a = vg.convert(ev).cpu().numpy()
    assert bit_equal(a, oracle.voxel_grid(ev_np, C, H, W, False))
    assert bit_equal(vg.convert(ev).cpu().numpy(), a)


@pytest.mark.parametrize("B,H,W,L", [(1, 60, 80, 4), (2, 17, 23, 3)])
def test_lookup_conv_vs_torch_reference(B, H, W, L):
    """Fused lookup + convc1 + ReLU (corr_lookup_conv) vs the unfused reference composition
    relu(conv2d(lookup, W, b)) evaluated in float64 from the (bit-exact) HIP lookup output:
    |diff| <= 1e-5 of max|out|; and the same without ReLU."""
    import torch.nn.functional as F
    D, r = 32, 4
    K = (2 * r + 1) ** 2
    f1, f2 = prng.gauss(81, (B, D, H, W)), prng.gauss(82, (B, D, H, W))
    cb = _cb()(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    c = torch.from_numpy(prng.lookup_coords(83, B, H, W, 3.0)).to(DEV)
    w = torch.from_numpy(prng.gauss(84, (256, L * K, 1, 1), 0.05)).to(DEV)
    bias = torch.from_numpy(prng.gauss(85, (256,), 0.1)).to(DEV)
    corr = cb(c).cpu().double()
    pre = F.conv2d(corr, w.cpu().double(), bias.cpu().double())
    for relu in (True, False):
        ref = (torch.relu(pre) if relu else pre).numpy()
        out = cb.lookup_conv(c, w, bias, relu=relu).cpu().numpy()
        assert np.abs(out - ref).max() <= 1e-5 * np.abs(ref).max(), relu


def test_lookup_conv_autograd_matches_unfused():
    """Training through the fused lookup + convc1 (corr._LookupConvFn): gradients w.r.t. both
    fmaps, the weight and the bias agree with the unfused autograd path (HIP lookup + conv2d +
    relu) within 1e-4 norm-relative, over 3 summed GRU-style lookups."""
    import torch.nn.functional as F
    B, D, H, W, L, r = 2, 32, 16, 20, 4, 4
    K = (2 * r + 1) ** 2
    f1, f2 = prng.gauss(91, (B, D, H, W)), prng.gauss(92, (B, D, H, W))
    w0 = prng.gauss(93, (256, L * K, 1, 1), 0.05)
    b0 = prng.gauss(94, (256,), 0.1)
    coords = [torch.from_numpy(prng.lookup_coords(95 + t, B, H, W, 3.0)).to(DEV) for t in range(3)]
    gouts = [torch.from_numpy(prng.gauss(99 + t, (B, 256, H, W))).to(DEV) for t in range(3)]
    grads = []
    for fused in (True, False):
        t1 = torch.from_numpy(f1).to(DEV).requires_grad_(True)
        t2 = torch.from_numpy(f2).to(DEV).requires_grad_(True)
        w = torch.from_numpy(w0).to(DEV).requires_grad_(True)
        b = torch.from_numpy(b0).to(DEV).requires_grad_(True)
        cb = _cb()(t1, t2, num_levels=L, radius=r)
        loss = 0
        for c, g in zip(coords, gouts):
            out = cb.lookup_conv(c, w, b) if fused else F.relu(F.conv2d(cb(c), w, b))
            loss = loss + (out * g).sum()
        loss.backward()
        grads.append([t.grad.detach().cpu().numpy() for t in (t1, t2, w, b)])
    for name, a, ref in zip(("dfmap1", "dfmap2", "dweight", "dbias"), *grads):
        assert norm_rel(a, ref) <= REL_TOL, (name, norm_rel(a, ref))


@pytest.mark.parametrize("B,H,W,L,relu", [(2, 17, 23, 3, True), (1, 16, 20, 4, False), (8, 36, 48, 4, True),
                                          (1, 8, 12, 3, True)])  # 3 blocks < 8 query ranges: empty ranges
def test_lookup_conv_bwd_vs_fp64(B, H, W, L, relu):
    """corr_lookup_conv_bwd (lookup recomputed on chip, bf16x6 products) vs the float64
    composition from the bit-exact HIP lookup: g' = where(out <= 0, 0, g); d bias = sum g';
    dW = g' lk^T; d lk = W^T g'.  Each element within 2^-20 of its sum of |products| (the
    bf16x6 contract is ~2^-23 per product plus fp32 accumulation); partial 32-query blocks
    (17 x 23), 3 levels, no ReLU, config 4's shape (64 query ranges); bit-identical on a rerun
    and with any subset of the outputs requested."""
    import torch.nn.functional as F
    from eraft_amd import _lib
    from eraft_amd.corr import _weight_pack
    D, r = 32, 4
    K = (2 * r + 1) ** 2
    C = L * K
    f1, f2 = prng.gauss(131, (B, D, H, W)), prng.gauss(132, (B, D, H, W))
    cb = _cb()(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    c = torch.from_numpy(prng.lookup_coords(133, B, H, W, 3.0)).to(DEV)
    w = torch.from_numpy(prng.gauss(134, (256, C, 1, 1), 0.05)).to(DEV)
    bias = torch.from_numpy(prng.gauss(135, (256,), 0.1)).to(DEV)
    g = torch.from_numpy(prng.gauss(136, (B, 256, H, W))).to(DEV)
    out = cb.lookup_conv(c, w, bias, relu=relu)
    lk = cb(c).double().cpu().reshape(B, C, H * W)
    gd = g.double().cpu()
    if relu:
        gd = torch.where(out.cpu() <= 0, torch.zeros((), dtype=torch.float64), gd)
    gd = gd.reshape(B, 256, H * W)
    wd = w.double().cpu().reshape(256, C)
    ref_b = gd.sum(dim=(0, 2))
    ref_w = torch.einsum("bon,bcn->oc", gd, lk)
    mag_w = torch.einsum("bon,bcn->oc", gd.abs(), lk.abs())
    ref_l = torch.einsum("oc,bon->bcn", wd, gd)
    mag_l = torch.einsum("oc,bon->bcn", wd.abs(), gd.abs())

    def run(want_w=True, want_b=True, want_l=True):
        dW = torch.empty((256, C), device=DEV) if want_w else None
        db = torch.empty((256,), device=DEV) if want_b else None
        dl = torch.empty((B, C, H, W), device=DEV) if want_l else None
        _lib.lookup_conv_bwd(cb._state.levels, c, r, _weight_pack(w), out, relu, g, dW, db, dl)
        return [None if t is None else t.cpu() for t in (dW, db, dl)]

    dW, db, dl = run()
    tol = 2.0 ** -20
    assert ((dW.double() - ref_w).abs() <= tol * mag_w + 1e-30).all()
    assert ((db.double() - ref_b).abs() <= tol * gd.abs().sum(dim=(0, 2)) + 1e-30).all()
    assert ((dl.double().reshape(B, C, H * W) - ref_l).abs() <= tol * mag_l + 1e-30).all()
    again = run()
    assert all(torch.equal(a, b) for a, b in zip((dW, db, dl), again))
    only_w, _, _ = run(True, False, False)
    _, _, only_l = run(False, False, True)
    assert torch.equal(only_w, dW) and torch.equal(only_l, dl)


def test_lookup_conv_weight_pack_not_aliased():
    """The packed convc1 split is cached per weight tensor: a second weight that reuses the
    first one's allocation (same data_ptr, same _version) must not see the first one's pack.
    (16 x 16: every level at least 2 x 2, so the reference composition is finite.)"""
    B, D, H, W, L, r = 1, 16, 16, 16, 4, 4
    K = (2 * r + 1) ** 2
    f1, f2 = prng.gauss(111, (B, D, H, W)), prng.gauss(112, (B, D, H, W))
    cb = _cb()(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    c = torch.from_numpy(prng.lookup_coords(113, B, H, W, 3.0)).to(DEV)
    bias = torch.zeros(256, device=DEV)
    outs = []
    for seed in (114, 115):
        w = torch.from_numpy(prng.gauss(seed, (256, L * K, 1, 1), 0.05)).to(DEV)
        outs.append((w.data_ptr(), cb.lookup_conv(c, w, bias).cpu().numpy(),
                     torch.relu(torch.nn.functional.conv2d(cb(c), w, bias)).cpu().numpy()))
        del w
    for _, out, ref in outs:
        assert np.abs(out - ref).max() <= 1e-5 * np.abs(ref).max()


def test_lookup_conv_nan_level_propagates():
    """A degenerate 1 x 2 level makes the reference lookup NaN (utils.py:11-12), and
    relu(conv2d(.)) of it is NaN everywhere: the fused kernel must give NaN at the same places
    (its ReLU keeps a NaN, as torch.relu does)."""
    B, D, H, W, L, r = 1, 16, 12, 16, 4, 4
    K = (2 * r + 1) ** 2
    f1, f2 = prng.gauss(116, (B, D, H, W)), prng.gauss(117, (B, D, H, W))
    cb = _cb()(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
    c = torch.from_numpy(prng.lookup_coords(118, B, H, W, 3.0)).to(DEV)
    w = torch.from_numpy(prng.gauss(119, (256, L * K, 1, 1), 0.05)).to(DEV)
    bias = torch.zeros(256, device=DEV)
    ref = torch.relu(torch.nn.functional.conv2d(cb(c), w, bias)).cpu().numpy()
    out = cb.lookup_conv(c, w, bias).cpu().numpy()
    assert np.array_equal(np.isnan(out), np.isnan(ref)) and np.isnan(ref).any()
    # backward: ReLU's threshold_backward passes the gradient where the output is NaN, so the
    # fused path's bias gradient (sum of g) matches the unfused autograd's NaN pattern and values
    g = torch.from_numpy(prng.gauss(120, (B, 256, H, W))).to(DEV)
    grads = []
    for fused in (True, False):
        wv = w.clone().requires_grad_(True)
        bv = bias.clone().requires_grad_(True)
        o = cb.lookup_conv(c, wv, bv) if fused else torch.relu(torch.nn.functional.conv2d(cb(c), wv, bv))
        (o * g).sum().backward()
        grads.append(bv.grad.cpu().numpy())
    assert np.array_equal(np.isnan(grads[0]), np.isnan(grads[1]))
    fin = np.isfinite(grads[1])
    assert np.abs(grads[0][fin] - grads[1][fin]).max(initial=0.0) <= 1e-5 * max(1.0, np.abs(grads[1][fin]).max(initial=0.0))


@pytest.mark.parametrize("N,h,w", [(1, 60, 80), (2, 9, 70)])
def test_convex_upsample_backward_vs_autograd(N, h, w):
    """corr_convex_upsample_bwd (ERAFT.upsample_flow's HIP backward) vs autograd of the
    reference composition (eraft.py:75-86) in float64: dflow and dmask within 1e-4 of max."""
    from eraft_amd.model import ERAFT
    flow = prng.gauss(121, (N, 2, h, w), 3.0)
    mask = prng.gauss(122, (N, 576, h, w), 2.0)
    g = prng.gauss(123, (N, 2, 8 * h, 8 * w))
    tf = torch.from_numpy(flow).to(DEV).requires_grad_(True)
    tm = torch.from_numpy(mask).to(DEV).requires_grad_(True)
    ERAFT.upsample_flow(tf, tm).backward(torch.from_numpy(g).to(DEV))
    rf = torch.from_numpy(flow).double().requires_grad_(True)
    rm = torch.from_numpy(mask).double().requires_grad_(True)
    ERAFT.upsample_flow(rf, rm).backward(torch.from_numpy(g).double())  # CPU: the torch composition
    for a, ref in ((tf.grad, rf.grad), (tm.grad, rm.grad)):
        a, ref = a.cpu().double().numpy(), ref.numpy()
        assert np.abs(a - ref).max() <= 1e-4 * np.abs(ref).max()
