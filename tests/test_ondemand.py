"""OnDemandCorrBlock / corr_ondemand_*: CorrBlock's lookups computed straight from the feature
maps (no all-pairs volume).

References: the fp64 op chain of oracle/torch_ops.py (cpu_build + cpu_lookup on float64 inputs)
and CorrBlock on the GPU.  "Within tolerance" = norm-relative <= REL_TOL (tests/_util.py) with
identical finite patterns.  The on-demand dot products are fp32 fmaf chains summed in another
order than the build's, so parity is tolerance-level, not bitwise; everything about the taps
(zeros outside the map, NaN for one-cell levels and non-finite coordinates) is exact.
"""
import functools

import numpy as np
import pytest
import torch

import prng
from _util import REL_TOL, bit_equal, norm_rel

DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def _level_cells(H, W, L):
    return sum((H >> l) * (W >> l) for l in range(L))


def test_workspace_size_and_bad_sizes(lib):
    """The workspace holds fmap1 and every pooled level of fmap2, D padded to a multiple of 4;
    sizes the calls would reject give 0."""
    for B, D, H, W, L in ((1, 256, 60, 80, 4), (2, 64, 17, 22, 4), (1, 3, 9, 11, 3), (16, 256, 160, 240, 4),
                          (1, 256, 270, 480, 4), (1, 5, 1, 1, 1)):
        n = lib.corr_ondemand_workspace(B, D, H, W, L)
        cells = H * W + _level_cells(H, W, L)
        assert n >= 4 * B * D * cells
        assert n == 4 * B * ((D + 3) // 4 * 4) * cells  # the documented layout, nothing else
    # 160x240, D = 256, 4 levels: 92 MB where the pyramid takes 7.9 GB
    assert lib.corr_ondemand_workspace(1, 256, 160, 240, 4) < 100e6
    for bad in ((0, 256, 60, 80, 4), (1, 0, 60, 80, 4), (1, 256, 0, 80, 4), (1, 256, 60, 0, 4), (-1, 256, 60, 80, 4),
                (1, 256, 60, 80, 0), (1, 256, 60, 80, 9), (1, 256, 4, 80, 4), (1, 256, 60, 7, 4),
                (1 << 20, 1 << 20, 32, 32, 1)):
        assert lib.corr_ondemand_workspace(*bad) == 0, bad


_WS = 1 << 40  # "large enough" workspace size for validation-only calls (no HIP call is reached)


@pytest.mark.parametrize("args,msg", [
    ((None, 16, 1, 256, 60, 80, 4, 256, _WS, None), "fmap1 is NULL"),
    ((16, None, 1, 256, 60, 80, 4, 256, _WS, None), "fmap2 is NULL"),
    ((6, 16, 1, 256, 60, 80, 4, 256, _WS, None), "fmap1 is not 4-byte aligned"),
    ((16, 16, 0, 256, 60, 80, 4, 256, _WS, None), "B, H, W must be >= 1"),
    ((16, 16, 1, 256, 0, 80, 4, 256, _WS, None), "B, H, W must be >= 1"),
    ((16, 16, 1, 256, 60, 0, 4, 256, _WS, None), "B, H, W must be >= 1"),
    ((16, 16, 1, 0, 60, 80, 4, 256, _WS, None), "D must be >= 1"),
    ((16, 16, 1, 256, 60, 80, 0, 256, _WS, None), "levels must be in [1, 8]"),
    ((16, 16, 1, 256, 60, 80, 9, 256, _WS, None), "levels must be in [1, 8]"),
    ((16, 16, 1, 256, 4, 80, 4, 256, _WS, None), "too small for 4 pyramid levels"),
    ((16, 16, 1, 256, 60, 80, 4, None, _WS, None), "workspace is NULL"),
    ((16, 16, 1, 256, 60, 80, 4, 264, _WS, None), "workspace is not 16-byte aligned"),
    ((16, 16, 1, 256, 60, 80, 4, 256, 4 * 256 * 4800, None), "workspace of"),
])
def test_prepare_rejects_bad_arguments(lib, args, msg):
    rc = lib.corr_ondemand_prepare(*args)
    assert rc == -1  # CORR_EINVAL
    assert "corr_ondemand_prepare" in lib.corr_last_error().decode()
    assert msg in lib.corr_last_error().decode()


@pytest.mark.parametrize("args,msg", [
    ((None, 16, 1, 256, 60, 80, 4, 4, 0, 16, None), "workspace is NULL"),
    ((264, 16, 1, 256, 60, 80, 4, 4, 0, 16, None), "workspace is not 16-byte aligned"),
    ((256, None, 1, 256, 60, 80, 4, 4, 0, 16, None), "coords is NULL"),
    ((256, 18, 1, 256, 60, 80, 4, 4, 0, 16, None), "coords is not 4-byte aligned"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 0, None, None), "out is NULL"),
    ((256, 16, 0, 256, 60, 80, 4, 4, 0, 16, None), "B, H, W must be >= 1"),
    ((256, 16, 1, 0, 60, 80, 4, 4, 0, 16, None), "D must be >= 1"),
    ((256, 16, 1, 256, 60, 80, 0, 4, 0, 16, None), "levels must be in [1, 8]"),
    ((256, 16, 1, 256, 60, 80, 9, 4, 0, 16, None), "levels must be in [1, 8]"),
    ((256, 16, 1, 256, 60, 7, 4, 4, 0, 16, None), "too small for 4 pyramid levels"),
    ((256, 16, 1, 256, 60, 80, 4, 8, 0, 16, None), "radius must be in [0, 7]"),
    ((256, 16, 1, 256, 60, 80, 4, -1, 0, 16, None), "radius must be in [0, 7]"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 2, 16, None), "unknown flags"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 1 | 4, 16, None), "unknown flags"),
])
def test_lookup_rejects_bad_arguments(lib, args, msg):
    rc = lib.corr_ondemand_lookup(*args)
    assert rc == -1  # CORR_EINVAL
    assert "corr_ondemand_lookup" in lib.corr_last_error().decode()
    assert msg in lib.corr_last_error().decode()


def test_version_is_unchanged_and_symbols_are_exported(lib):
    from eraft_amd import _lib
    assert lib.corr_version() == 202
    for name in ("corr_ondemand_workspace", "corr_ondemand_prepare", "corr_ondemand_lookup"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert _lib.ONDEMAND_GENERAL == 1


def test_refuses_cpu_tensors():
    from eraft_amd import OnDemandCorrBlock
    f = torch.zeros(1, 8, 16, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        OnDemandCorrBlock(f, f)


def test_block_has_no_pyramid_and_no_fused_conv():
    from eraft_amd import OnDemandCorrBlock
    assert not hasattr(OnDemandCorrBlock, "corr_pyramid") and not hasattr(OnDemandCorrBlock, "lookup_conv")


def test_model_switch_default_off_and_env_override(monkeypatch):
    from eraft_amd.model import ERAFT
    monkeypatch.delenv("ERAFT_AMD_ONDEMAND", raising=False)
    assert ERAFT({"subtype": "standard"}, n_first_channels=3).alternate_corr is False
    assert ERAFT({"subtype": "standard", "alternate_corr": True}, n_first_channels=3).alternate_corr is True
    monkeypatch.setenv("ERAFT_AMD_ONDEMAND", "1")
    assert ERAFT({"subtype": "standard"}, n_first_channels=3).alternate_corr is True
    monkeypatch.setenv("ERAFT_AMD_ONDEMAND", "0")
    assert ERAFT({"subtype": "standard", "alternate_corr": True}, n_first_channels=3).alternate_corr is False


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------
def _fmaps(seed, B, D, H, W):
    return prng.gauss(seed, (B, D, H, W)), prng.gauss(seed + 1, (B, D, H, W))


def _coherent(seed, B, H, W):
    """grid + constant flow (2.3, -1.6) + sigma 0.05: what the GRU produces."""
    c = prng.lookup_coords(seed, B, H, W, 0.05)
    c[:, 0] += np.float32(2.3)
    c[:, 1] -= np.float32(1.6)
    return c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(f1, f2, coords, levels, radius) of a named case; built once."""
    if name == "odd":
        B, D, H, W, L, r = 2, 64, 17, 22, 4, 4
        return (*_fmaps(11, B, D, H, W), prng.lookup_coords(13, B, H, W, 4.0), L, r)
    if name == "coherent":
        B, D, H, W, L, r = 1, 256, 24, 32, 4, 4
        return (*_fmaps(21, B, D, H, W), _coherent(23, B, H, W), L, r)
    if name == "mixed":
        B, D, H, W, L, r = 1, 64, 24, 32, 4, 4
        c = _coherent(33, B, H, W)
        c[..., W // 2:] = prng.lookup_coords(34, B, H, W, 6.0)[..., W // 2:]
        return (*_fmaps(31, B, D, H, W), c, L, r)
    if name == "r0":
        return (*_fmaps(41, 1, 8, 10, 13), prng.lookup_coords(43, 1, 10, 13, 2.0), 1, 0)
    if name == "r3":
        return (*_fmaps(51, 2, 32, 9, 11), prng.lookup_coords(53, 2, 9, 11, 3.0), 3, 3)
    if name == "r7":
        return (*_fmaps(61, 1, 16, 16, 16), prng.lookup_coords(63, 1, 16, 16, 4.0), 2, 7)
    if name == "d3":
        return (*_fmaps(71, 2, 3, 12, 15), prng.lookup_coords(73, 2, 12, 15, 3.0), 2, 2)
    if name == "d300":  # more than one 256-feature chunk, D % 4 == 0 but D % 32 != 0
        return (*_fmaps(81, 1, 300, 9, 12), prng.lookup_coords(83, 1, 9, 12, 3.0), 2, 4)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _ref64(name):
    """The fp64 op chain's lookup (numpy)."""
    from oracle.torch_ops import cpu_build, cpu_lookup
    f1, f2, coords, L, r = _case(name)
    levels = cpu_build(torch.from_numpy(f1).double(), torch.from_numpy(f2).double(), L)
    return cpu_lookup(levels, torch.from_numpy(coords).double(), r).numpy()


@functools.lru_cache(maxsize=None)
def _corrblock(name):
    """CorrBlock's lookup on the GPU (numpy)."""
    from eraft_amd import CorrBlock
    f1, f2, coords, L, r = _case(name)
    with torch.no_grad():
        blk = CorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)
        return blk(torch.from_numpy(coords).to(DEV)).cpu().numpy()


def _ondemand(f1, f2, coords, L, r, flags=0):
    from eraft_amd import OnDemandCorrBlock
    with torch.no_grad():
        blk = OnDemandCorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r,
                                flags=flags)
        out = blk(torch.from_numpy(coords).to(DEV))
    assert out.dtype == torch.float32
    assert tuple(out.shape) == (coords.shape[0], L * (2 * r + 1) ** 2, coords.shape[2], coords.shape[3])
    return out.cpu().numpy()


def _check_case(name):
    from eraft_amd import _lib
    auto = _ondemand(*_case(name))
    gen = _ondemand(*_case(name), flags=_lib.ONDEMAND_GENERAL)
    for what, ref in (("fp64 chain", _ref64(name)), ("CorrBlock", _corrblock(name))):
        ea, eg = norm_rel(auto, ref), norm_rel(gen, ref)
        print(f"{name}: vs {what}: auto {ea:.2e}, general {eg:.2e}")
        assert ea <= REL_TOL and eg <= REL_TOL
    e = norm_rel(auto, gen)
    print(f"{name}: auto vs general {e:.2e}")
    assert e <= REL_TOL


@pytest.mark.gpu
def test_odd_sizes_incoherent_coords():
    """17x22, 4 levels: floor halving drops a row at level 1 and a column at level 2; sigma = 4
    windows cross every border."""
    _check_case("odd")


@pytest.mark.gpu
def test_coherent_flow():
    """grid + (2.3, -1.6) + sigma 0.05 at D = 256: every 8x8 block's neighbourhoods fit a small box."""
    _check_case("coherent")


@pytest.mark.gpu
def test_mixed_coherent_and_incoherent_halves():
    _check_case("mixed")


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["r0", "r3", "r7", "d3", "d300"])
def test_other_shapes(name):
    _check_case(name)


@pytest.mark.gpu
def test_special_coordinates_match_corrblock():
    """special_coords plus NaN, +-inf and 1e30 in a few queries of each batch item: the same NaN
    and zero pattern as CorrBlock, finite values within tolerance."""
    from eraft_amd import CorrBlock, _lib
    B, D, H, W, L, r = 2, 32, 16, 20, 3, 4
    f1, f2 = _fmaps(91, B, D, H, W)
    c = prng.special_coords(B, H, W).reshape(B, 2, -1)
    bad = [np.nan, np.inf, -np.inf, 1e30, -1e30]
    for k, v in enumerate(bad):
        c[:, 0, 40 + k] = v            # x only
        c[:, 1, 60 + k] = v            # y only
        c[:, :, 80 + k] = v            # both
    c[:, 0, 100], c[:, 1, 100] = np.inf, np.nan
    c = c.reshape(B, 2, H, W).astype(np.float32)
    with torch.no_grad():
        ref = CorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)(
            torch.from_numpy(c).to(DEV)).cpu().numpy()
    for flags in (0, _lib.ONDEMAND_GENERAL):
        out = _ondemand(f1, f2, c, L, r, flags)
        assert np.array_equal(np.isnan(out), np.isnan(ref))
        assert np.isnan(ref).any() and (ref == 0).any()
        assert np.array_equal(out == 0, ref == 0)
        e = norm_rel(out, ref)
        print(f"special coords, flags {flags}: {e:.2e}")
        assert e <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("H,W,L,nan_levels", [(8, 8, 4, (3,)), (8, 2, 2, (1,)), (2, 9, 2, (1,))])
def test_one_cell_and_one_wide_levels_are_nan(H, W, L, nan_levels):
    """A level whose H_l or W_l is 1 gives NaN for all its channels, as CorrBlock does; the other
    levels are unaffected."""
    from eraft_amd import CorrBlock
    B, D, r = 1, 16, 4
    K = (2 * r + 1) ** 2
    f1, f2 = _fmaps(101, B, D, H, W)
    c = prng.lookup_coords(103, B, H, W, 1.0)
    out = _ondemand(f1, f2, c, L, r)
    with torch.no_grad():
        ref = CorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=r)(
            torch.from_numpy(c).to(DEV)).cpu().numpy()
    for l in range(L):
        ch = out[:, l * K:(l + 1) * K]
        if l in nan_levels:
            assert np.isnan(ch).all() and np.isnan(ref[:, l * K:(l + 1) * K]).all()
        else:
            assert np.isfinite(ch).all()
    assert norm_rel(out, ref) <= REL_TOL


@pytest.mark.gpu
def test_non_contiguous_coords():
    from eraft_amd import OnDemandCorrBlock
    f1, f2, coords, L, r = _case("r3")
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    cc = torch.from_numpy(coords).to(DEV)
    nc = cc.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # [B, 2, H, W] view of [B, H, W, 2]
    assert not nc.is_contiguous()
    with torch.no_grad():
        blk = OnDemandCorrBlock(t1, t2, num_levels=L, radius=r)
        assert bit_equal(blk(nc).cpu().numpy(), blk(cc).cpu().numpy())
        with pytest.raises(ValueError, match="coords must be"):
            blk(cc[:, :1])
        with pytest.raises(ValueError, match="do not match"):
            blk(cc[:, :, :-1])


@pytest.mark.gpu
def test_deterministic_and_graph_capturable():
    """Two eager runs are bit-equal; prepare + two lookups captured on one stream and replayed
    are bit-equal to eager."""
    from eraft_amd import OnDemandCorrBlock
    f1, f2, coords, L, r = _case("odd")
    t1, t2 = torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV)
    c1 = torch.from_numpy(coords).to(DEV)
    c2 = c1 + 0.37
    with torch.no_grad():
        e1, e2 = (OnDemandCorrBlock(t1, t2, L, r)(c) for c in (c1, c2))
        again = OnDemandCorrBlock(t1, t2, L, r)(c1)
        assert bit_equal(e1.cpu().numpy(), again.cpu().numpy())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            blk = OnDemandCorrBlock(t1, t2, L, r)
            g1, g2 = blk(c1), blk(c2)
        for _ in range(2):
            g1.zero_(), g2.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert bit_equal(g1.cpu().numpy(), e1.cpu().numpy())
            assert bit_equal(g2.cpu().numpy(), e2.cpu().numpy())


@pytest.mark.gpu
def test_memory_is_workspace_plus_output():
    """1x64x60x80: constructing the block and one lookup allocate the workspace (~2.9 MB) and the
    output (~6.2 MB) — under 16 MB, where CorrBlock's pyramid alone is ~123 MB."""
    from eraft_amd import OnDemandCorrBlock
    B, D, H, W = 1, 64, 60, 80
    t1 = torch.from_numpy(prng.gauss(111, (B, D, H, W))).to(DEV)
    t2 = torch.from_numpy(prng.gauss(112, (B, D, H, W))).to(DEV)
    c = torch.from_numpy(prng.lookup_coords(113, B, H, W, 2.0)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.no_grad():
        blk = OnDemandCorrBlock(t1, t2, num_levels=4, radius=4)
        out = blk(c)
    torch.cuda.synchronize()
    inc = torch.cuda.max_memory_allocated() - base
    print(f"peak allocation increase {inc / 1e6:.2f} MB")
    assert inc < 16e6
    assert tuple(out.shape) == (B, 324, H, W) and bool(torch.isfinite(out).all())


def _model(bins, alternate):
    from eraft_amd.model import ERAFT
    m = ERAFT({"subtype": "standard", "alternate_corr": alternate}, n_first_channels=bins).eval()
    with torch.no_grad():
        for name, t in m.state_dict().items():
            v = prng.param_init(name, tuple(t.shape))
            if v is not None:
                t.copy_(torch.from_numpy(v))
    return m


@pytest.mark.gpu
def test_model_alternate_corr_gives_the_same_flow(monkeypatch):
    """ERAFT at 128x160, 3 iterations, random-init weights: alternate_corr on vs off, final-flow
    EPE <= 0.01 px (the project's end-to-end bound)."""
    monkeypatch.delenv("ERAFT_AMD_ONDEMAND", raising=False)
    bins, H, W = 5, 128, 160
    im1 = torch.from_numpy(prng.voxel_grid(121, (1, bins, H, W))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(123, (1, bins, H, W))).to(DEV)
    flows = []
    for alt in (False, True):
        m = _model(bins, alt).to(DEV)
        assert m.alternate_corr is alt
        with torch.no_grad():
            low, ups = m(im1, im2, iters=3)
        flows.append((low.cpu().numpy().astype(np.float64), ups[-1].cpu().numpy().astype(np.float64)))
    for k, what in ((0, "1/8 resolution"), (1, "full resolution")):
        epe = float(np.sqrt(((flows[0][k] - flows[1][k]) ** 2).sum(1)).mean())
        print(f"alternate_corr on vs off, {what}: EPE {epe:.2e} px")
        assert np.isfinite(flows[1][k]).all() and epe <= 0.01


@pytest.mark.gpu
def test_grad_contract():
    """Inference only: grad mode on with a map that requires grad raises and names CorrBlock;
    under no_grad, or with detached maps, it works."""
    from eraft_amd import OnDemandCorrBlock
    f1, f2, coords, L, r = _case("r3")
    t1 = torch.from_numpy(f1).to(DEV).requires_grad_(True)
    t2 = torch.from_numpy(f2).to(DEV)
    c = torch.from_numpy(coords).to(DEV)
    with pytest.raises(NotImplementedError, match="CorrBlock"):
        OnDemandCorrBlock(t1, t2, num_levels=L, radius=r)
    with torch.no_grad():
        a = OnDemandCorrBlock(t1, t2, num_levels=L, radius=r)(c)
    b = OnDemandCorrBlock(t1.detach(), t2, num_levels=L, radius=r)(c)
    assert not a.requires_grad and not b.requires_grad
    assert bit_equal(a.cpu().numpy(), b.cpu().numpy())
    assert norm_rel(a.cpu().numpy(), _corrblock("r3")) <= REL_TOL


@pytest.mark.gpu
def test_c_abi_direct_call_matches_the_block():
    """corr_ondemand_prepare / _lookup through _lib with a caller-allocated workspace."""
    from eraft_amd import _lib
    f1, f2, coords, L, r = _case("r3")
    B, D, H, W = f1.shape
    t1, t2, c = (torch.from_numpy(x).to(DEV) for x in (f1, f2, coords))
    ws = _lib.ondemand_workspace(B, D, H, W, L, t1.device)
    assert ws.numel() * 4 == _lib.load().corr_ondemand_workspace(B, D, H, W, L)
    out = torch.full((B, L * (2 * r + 1) ** 2, H, W), float("nan"), device=DEV)
    _lib.ondemand_prepare(t1, t2, L, ws)
    _lib.ondemand_lookup(ws, c, D, L, r, out, _lib.ONDEMAND_GENERAL)
    assert norm_rel(out.cpu().numpy(), _ref64("r3")) <= REL_TOL
    with pytest.raises(ValueError, match="workspace"):
        _lib.ondemand_lookup(ws[:100], c, D, L, r, out)
