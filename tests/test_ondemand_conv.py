"""OnDemandConvCorrBlock / corr_ondemand_lookup_conv: the on-demand lookup fused with convc1.

What enters the convolution is corr_ondemand_lookup's output bit for bit (checked with weights
that select single channels, on both routes); the convolution is the bf16x6 family's (exact
three-piece split, six products), checked against relu(conv2d(.)) in fp64 from the block's own
lookup (bound 1e-5 of the largest output, test_lookup_conv_vs_torch_reference's) and against the
fp64 chain of oracle/torch_ops.py (norm-relative <= REL_TOL).  All cases use r = 4.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
from _util import REL_TOL, bit_equal, norm_rel

DEV = "cuda:0"
OK, EINVAL, EUNSUPPORTED = 0, -1, -2
R, K = 4, 81


# ---------------------------------------------------------------------------------------------
# without a GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def test_symbol_is_exported_and_version_is_unchanged(lib):
    from eraft_amd import _lib
    assert "corr_ondemand_lookup_conv" in _lib.EXPORTS and hasattr(lib, "corr_ondemand_lookup_conv")
    assert lib.corr_version() == 202


# (workspace, coords, B, D, H, W, levels, radius, flags, packed_weight, bias, relu, out, stream)
@pytest.mark.parametrize("args,code,msg", [
    ((None, 16, 1, 256, 60, 80, 4, 4, 0, 256, 16, 1, 16, None), EINVAL, "workspace is NULL"),
    ((264, 16, 1, 256, 60, 80, 4, 4, 0, 256, 16, 1, 16, None), EINVAL, "workspace is not 16-byte aligned"),
    ((256, None, 1, 256, 60, 80, 4, 4, 0, 256, 16, 1, 16, None), EINVAL, "coords is NULL"),
    ((256, 18, 1, 256, 60, 80, 4, 4, 0, 256, 16, 1, 16, None), EINVAL, "coords is not 4-byte aligned"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 0, None, 16, 1, 16, None), EINVAL, "packed_weight is NULL"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 0, 258, 16, 1, 16, None), EINVAL, "packed_weight is not 4-byte aligned"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 0, 256, None, 1, 16, None), EINVAL, "bias is NULL"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 0, 256, 18, 1, 16, None), EINVAL, "bias is not 4-byte aligned"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 0, 256, 16, 1, None, None), EINVAL, "out is NULL"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 0, 256, 16, 1, 18, None), EINVAL, "out is not 4-byte aligned"),
    ((256, 16, 0, 256, 60, 80, 4, 4, 0, 256, 16, 1, 16, None), EINVAL, "B, H, W must be >= 1"),
    ((256, 16, 1, 0, 60, 80, 4, 4, 0, 256, 16, 1, 16, None), EINVAL, "D must be >= 1"),
    ((256, 16, 1, 256, 60, 80, 9, 4, 0, 256, 16, 1, 16, None), EINVAL, "levels must be in [1, 8]"),
    ((256, 16, 1, 256, 60, 7, 4, 4, 0, 256, 16, 1, 16, None), EINVAL, "too small for 4 pyramid levels"),
    ((256, 16, 1, 256, 60, 80, 4, 8, 0, 256, 16, 1, 16, None), EINVAL, "radius must be in [0, 7]"),
    ((256, 16, 1, 256, 60, 80, 4, 4, 2, 256, 16, 1, 16, None), EINVAL, "unknown flags"),
    ((256, 16, 1, 256, 60, 80, 4, 3, 0, 256, 16, 1, 16, None), EUNSUPPORTED,
     "built for radius 4 and <= 4 levels (got 3, 4)"),
    ((256, 16, 1, 256, 60, 80, 5, 4, 0, 256, 16, 1, 16, None), EUNSUPPORTED,
     "built for radius 4 and <= 4 levels (got 4, 5)"),
])
def test_rejects_bad_arguments(lib, args, code, msg):
    """corr_ondemand_lookup's checks, then corr_lookup_conv's, with their wording (no HIP call is
    reached)."""
    assert lib.corr_ondemand_lookup_conv(*args) == code
    err = lib.corr_last_error().decode()
    assert "corr_ondemand_lookup_conv" in err and msg in err


def test_binding_checks_the_workspace_and_output_sizes(lib):
    """_lib.ondemand_lookup_conv refuses a short workspace and a wrong `out` from the shapes alone,
    as _lib.ondemand_lookup does, before anything touches a device."""
    from eraft_amd import _lib
    B, D, H, W, L = 1, 8, 16, 16, 4
    need = lib.corr_ondemand_workspace(B, D, H, W, L) // 4
    coords = torch.zeros(B, 2, H, W)
    packed, bias = torch.zeros(lib.corr_lookup_conv_weights_bytes() // 4), torch.zeros(256)
    with pytest.raises(ValueError, match="workspace is smaller than corr_ondemand_workspace"):
        _lib.ondemand_lookup_conv(torch.zeros(need - 1), coords, D, L, R, packed, bias, torch.zeros(B, 256, H, W))
    for bad in (torch.zeros(B, 255, H, W), torch.zeros(B, L * K, H, W)):
        with pytest.raises(ValueError, match=f"out has {bad.numel()} floats"):
            _lib.ondemand_lookup_conv(torch.zeros(need), coords, D, L, R, packed, bias, bad)
    with pytest.raises(RuntimeError, match="MI355X"):  # right sizes: the device check is next
        _lib.ondemand_lookup_conv(torch.zeros(need), coords, D, L, R, packed, bias, torch.zeros(B, 256, H, W))


def test_only_the_subclass_has_lookup_conv():
    import eraft_amd
    from eraft_amd import OnDemandConvCorrBlock, OnDemandCorrBlock
    assert issubclass(OnDemandConvCorrBlock, OnDemandCorrBlock)
    assert hasattr(OnDemandConvCorrBlock, "lookup_conv") and not hasattr(OnDemandCorrBlock, "lookup_conv")
    assert "OnDemandConvCorrBlock" in eraft_amd.__all__


def test_model_switch_is_off_by_default():
    """ERAFT_AMD_ONDEMAND_FUSE_CONV is read once, at import; unset (or anything but "1") is off."""
    import os
    from eraft_amd.model import ERAFT
    assert ERAFT.fuse_ondemand_conv is (os.environ.get("ERAFT_AMD_ONDEMAND_FUSE_CONV", "0") == "1")
    assert "ERAFT_AMD_ONDEMAND_FUSE_CONV" in os.environ or ERAFT.fuse_ondemand_conv is False


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------
def _fmaps(seed, B, D, H, W):
    return prng.gauss(seed, (B, D, H, W)), prng.gauss(seed + 1, (B, D, H, W))


def _coherent(seed, B, H, W):
    """grid + constant flow (2.3, -1.6) + sigma 0.05: what the GRU produces (test_ondemand.py's)."""
    c = prng.lookup_coords(seed, B, H, W, 0.05)
    c[:, 0] += np.float32(2.3)
    c[:, 1] -= np.float32(1.6)
    return c.astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(f1, f2, coords, levels) of a named case; built once, read-only."""
    if name == "sel_coherent":  # every block tiled at all four levels
        B, D, H, W, L = 1, 64, 24, 32, 4
        return (*_fmaps(211, B, D, H, W), _coherent(213, B, H, W), L)
    if name == "sel_odd":  # partial blocks, B = 2, the fallback inside the launch
        B, D, H, W, L = 2, 64, 17, 22, 4
        return (*_fmaps(221, B, D, H, W), prng.lookup_coords(223, B, H, W, 4.0), L)
    if name == "coherent":
        B, D, H, W, L = 1, 256, 24, 32, 4
        return (*_fmaps(231, B, D, H, W), _coherent(233, B, H, W), L)
    if name == "mixed":  # left half coherent, right half sigma = 6: both routes in one launch
        B, D, H, W, L = 1, 64, 24, 32, 4
        c = _coherent(243, B, H, W)
        c[..., W // 2:] = prng.lookup_coords(244, B, H, W, 6.0)[..., W // 2:]
        return (*_fmaps(241, B, D, H, W), c, L)
    if name == "l3":  # K = 243: the pack's zero region
        B, D, H, W, L = 2, 32, 17, 23, 3
        return (*_fmaps(251, B, D, H, W), prng.lookup_coords(253, B, H, W, 3.0), L)
    if name == "d300":  # more than one 256-feature chunk
        B, D, H, W, L = 1, 300, 9, 12, 2
        return (*_fmaps(261, B, D, H, W), prng.lookup_coords(263, B, H, W, 3.0), L)
    if name == "d3":  # Dp padding
        B, D, H, W, L = 2, 3, 16, 15, 2
        return (*_fmaps(271, B, D, H, W), prng.lookup_coords(273, B, H, W, 3.0), L)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def _wb(L):
    """convc1-like weight [256, L*81, 1, 1] and bias [256] on the device (read-only)."""
    w = torch.from_numpy(prng.gauss(284 + L, (256, L * K, 1, 1), 0.05)).to(DEV)
    b = torch.from_numpy(prng.gauss(285 + L, (256,), 0.1)).to(DEV)
    return w, b


def _block(name, flags=0, cls=None):
    from eraft_amd import OnDemandConvCorrBlock
    f1, f2, coords, L = _case(name)
    with torch.no_grad():
        blk = (cls or OnDemandConvCorrBlock)(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV),
                                             num_levels=L, radius=R, flags=flags)
    return blk, torch.from_numpy(coords).to(DEV)


def _select(first, L):
    """W with a single 1.0 per output row: output o = lookup channel first + o."""
    w = torch.zeros(256, L * K, 1, 1)
    w[torch.arange(256), first + torch.arange(256)] = 1.0
    return w.to(DEV)


@pytest.mark.gpu
@pytest.mark.parametrize("general", [False, True], ids=["auto", "general"])
@pytest.mark.parametrize("name", ["sel_coherent", "sel_odd"])
def test_selection_weights_return_the_lookup_exactly(name, general):
    """A weight that selects channel c (one 1.0 per row), zero bias, no ReLU: the three pieces of
    a float sum to it exactly and every other product is an exact zero, so the output must EQUAL
    (as values: -0 = +0) the block's own lookup — channels 0-255 in one call, 68-323 in a second —
    with the same flags.  What enters the product is therefore corr_ondemand_lookup's output."""
    from eraft_amd import _lib
    blk, c = _block(name, _lib.ONDEMAND_GENERAL if general else 0)
    L = blk.num_levels
    zero = torch.zeros(256, device=DEV)
    with torch.no_grad():
        look = blk(c).cpu().numpy()
        assert np.isfinite(look).all()  # a NaN would reach all 256 outputs of its query (NaN * 0)
        for first in (0, L * K - 256):
            out = blk.lookup_conv(c, _select(first, L), zero, relu=False).cpu().numpy()
            assert out.shape == (look.shape[0], 256) + look.shape[2:]
            assert np.array_equal(out, look[:, first:first + 256]), (name, general, first)


def _ref64_from(look, w, b):
    """conv2d in fp64 on the CPU from a lookup output (before ReLU)."""
    return F.conv2d(look.cpu().double(), w.cpu().double(), b.cpu().double())


@functools.lru_cache(maxsize=None)
def _oracle64(name):
    """The fp64 chain of oracle/torch_ops.py: cpu_build, cpu_lookup, then the fp64 convolution."""
    from oracle.torch_ops import cpu_build, cpu_lookup
    f1, f2, coords, L = _case(name)
    levels = cpu_build(torch.from_numpy(f1).double(), torch.from_numpy(f2).double(), L)
    look = cpu_lookup(levels, torch.from_numpy(coords).double(), R)
    w, b = _wb(L)
    return _ref64_from(look, w, b)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["coherent", "mixed", "l3", "d300", "d3"])
def test_accuracy(name):
    """Against relu(conv2d(.)) in fp64 from the block's own lookup: |diff| <= 1e-5 max|ref|, with
    and without ReLU (test_lookup_conv_vs_torch_reference's bound: the bf16x6 product is no
    narrower than fp32).  Against the fp64 chain: norm-relative <= REL_TOL.  Auto against
    ONDEMAND_GENERAL <= REL_TOL.  The unfused fp32 composition's errors are printed beside."""
    from eraft_amd import _lib
    L = _case(name)[3]
    w, b = _wb(L)
    outs = {}
    for flags in (0, _lib.ONDEMAND_GENERAL):
        blk, c = _block(name, flags)
        with torch.no_grad():
            look = blk(c)
            pre = _ref64_from(look, w, b)
            unfused = F.conv2d(look, w, b)
            for relu in (True, False):
                ref = (torch.relu(pre) if relu else pre).numpy()
                out = blk.lookup_conv(c, w, b, relu=relu).cpu().numpy()
                un = (torch.relu(unfused) if relu else unfused).cpu().numpy()
                e = np.abs(out - ref).max() / np.abs(ref).max()
                eu = np.abs(un - ref).max() / np.abs(ref).max()
                print(f"{name} flags {flags} relu {relu}: vs fp64 of own lookup: fused {e:.2e}, unfused fp32 {eu:.2e}")
                assert e <= 1e-5, (flags, relu)
                outs[flags, relu] = out
            orc = _oracle64(name)
            for relu in (True, False):
                ref = (torch.relu(orc) if relu else orc).numpy()
                e = norm_rel(outs[flags, relu], ref)
                un = (torch.relu(unfused) if relu else unfused).cpu().numpy()
                print(f"{name} flags {flags} relu {relu}: vs fp64 chain: fused {e:.2e}, unfused fp32 "
                      f"{norm_rel(un, ref):.2e}")
                assert e <= REL_TOL, (flags, relu)
    for relu in (True, False):
        e = norm_rel(outs[0, relu], outs[_lib.ONDEMAND_GENERAL, relu])
        print(f"{name} relu {relu}: auto vs general {e:.2e}")
        assert e <= REL_TOL


def _fused_matches_own_lookup(f1, f2, c, L, flags):
    """Non-finite pattern and finite values of lookup_conv against the fp64 composition from the
    block's own lookup (norm_rel asserts the pattern)."""
    from eraft_amd import OnDemandConvCorrBlock
    w, b = _wb(L)
    with torch.no_grad():
        blk = OnDemandConvCorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L,
                                    radius=R, flags=flags)
        ct = torch.from_numpy(c).to(DEV)
        look = blk(ct)
        pre = _ref64_from(look, w, b)
        errs = []
        for relu in (True, False):
            ref = (torch.relu(pre) if relu else pre).numpy()
            out = blk.lookup_conv(ct, w, b, relu=relu).cpu().numpy()
            errs.append(norm_rel(out, ref))
    return look.cpu().numpy(), errs


@pytest.mark.gpu
def test_special_coordinates():
    """test_special_coordinates_match_corrblock's coordinates (far, NaN, +-inf, borders, near
    2^20): a query whose lookup holds a NaN is NaN in all 256 outputs, as the fp64 composition
    is; every other value is within 1e-5 of the largest."""
    from eraft_amd import _lib
    B, D, H, W, L = 2, 32, 16, 20, 3
    f1, f2 = _fmaps(291, B, D, H, W)
    c = prng.special_coords(B, H, W).reshape(B, 2, -1)
    for k, v in enumerate([np.nan, np.inf, -np.inf, 1e30, -1e30]):
        c[:, 0, 40 + k] = v            # x only
        c[:, 1, 60 + k] = v            # y only
        c[:, :, 80 + k] = v            # both
    c[:, 0, 100], c[:, 1, 100] = np.inf, np.nan
    c = c.reshape(B, 2, H, W).astype(np.float32)
    for flags in (0, _lib.ONDEMAND_GENERAL):
        look, errs = _fused_matches_own_lookup(f1, f2, c, L, flags)
        assert np.isnan(look).any() and np.isfinite(look).any()
        print(f"special coordinates, flags {flags}: relu / no relu {errs[0]:.2e} / {errs[1]:.2e}")
        assert max(errs) <= 1e-5


@pytest.mark.gpu
def test_one_cell_last_level():
    """8x8 with 4 levels: level 3 is one cell, its 81 channels are NaN (as CorrBlock's), so every
    output is NaN — in the fused launch and in the composition alike."""
    B, D, H, W, L = 1, 16, 8, 8, 4
    f1, f2 = _fmaps(301, B, D, H, W)
    look, errs = _fused_matches_own_lookup(f1, f2, prng.lookup_coords(303, B, H, W, 1.0), L, 0)
    assert np.isnan(look[:, 3 * K:]).all() and np.isfinite(look[:, :3 * K]).all()
    assert max(errs) == 0.0  # nothing finite is left to differ


@pytest.mark.gpu
def test_deterministic_and_graph_capturable():
    """Two eager runs are bit-equal; a captured launch replayed is bit-equal to eager."""
    blk, c = _block("sel_odd")
    w, b = _wb(blk.num_levels)
    with torch.no_grad():
        e1 = blk.lookup_conv(c, w, b)
        e2 = blk.lookup_conv(c, w, b)
        assert bit_equal(e1.cpu().numpy(), e2.cpu().numpy())
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            g = blk.lookup_conv(c, w, b)
        for _ in range(2):
            g.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert bit_equal(g.cpu().numpy(), e1.cpu().numpy())


@pytest.mark.gpu
def test_non_contiguous_coords_and_shape_checks():
    blk, cc = _block("l3")
    w, b = _wb(blk.num_levels)
    nc = cc.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)  # [B, 2, H, W] view of [B, H, W, 2]
    assert not nc.is_contiguous()
    with torch.no_grad():
        assert bit_equal(blk.lookup_conv(nc, w, b).cpu().numpy(), blk.lookup_conv(cc, w, b).cpu().numpy())
        with pytest.raises(ValueError, match="coords must be"):
            blk.lookup_conv(cc[:, :1], w, b)
        with pytest.raises(ValueError, match="lookup_conv needs weight"):
            blk.lookup_conv(cc, _wb(4)[0], b)
        with pytest.raises(ValueError, match="lookup_conv needs weight"):
            blk.lookup_conv(cc, w, b[:255])


@pytest.mark.gpu
def test_peak_allocation_is_the_output():
    """1x64x24x32: lookup_conv allocates its [B, 256, H, W] output (786 KB) and nothing else —
    the 324-channel lookup would be another 995 KB."""
    blk, c = _block("sel_coherent")
    w, b = _wb(4)
    with torch.no_grad():
        blk.lookup_conv(c, w, b)  # the pack is made once per weight
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = blk.lookup_conv(c, w, b)
        torch.cuda.synchronize()
    inc = torch.cuda.max_memory_allocated() - base
    n = c.shape[0] * c.shape[2] * c.shape[3]
    print(f"peak allocation increase {inc} B, output {out.numel() * 4} B, a lookup would be {324 * n * 4} B")
    assert out.numel() * 4 <= inc <= out.numel() * 4 + 4096  # the allocator's rounding, no more


@pytest.mark.gpu
def test_autograd_is_the_unfused_composition():
    """A weight that requires grad under grad mode: result and gradients are bit-equal to
    F.relu(F.conv2d(block(coords), W, b)); so is a train=True block's (gradients to the maps)."""
    from eraft_amd import OnDemandConvCorrBlock
    f1, f2, coords, L = _case("l3")
    c = torch.from_numpy(coords).to(DEV)
    w0, b0 = _wb(L)
    g = torch.from_numpy(prng.gauss(311, (coords.shape[0], 256) + coords.shape[2:])).to(DEV)
    for train in (False, True):
        res = []
        for fused in (True, False):
            t1 = torch.from_numpy(f1).to(DEV).requires_grad_(train)
            t2 = torch.from_numpy(f2).to(DEV).requires_grad_(train)
            w, b = w0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
            blk = OnDemandConvCorrBlock(t1, t2, num_levels=L, radius=R, train=train)
            out = blk.lookup_conv(c, w, b) if fused else F.relu(F.conv2d(blk(c), w, b))
            assert out.requires_grad
            (out * g).sum().backward()
            res.append([out.detach()] + [t.grad for t in ((t1, t2, w, b) if train else (w, b))])
        for a, r in zip(*res):
            assert bit_equal(a.cpu().numpy(), r.cpu().numpy()), train


@pytest.mark.gpu
def test_pack_is_shared_with_corrblock(monkeypatch):
    """One CorrBlock.lookup_conv call and one OnDemandConvCorrBlock.lookup_conv call with the same
    weight make one pack (corr._weight_pack's cache serves both)."""
    from eraft_amd import CorrBlock, _lib
    f1, f2, coords, L = _case("l3")
    blk, c = _block("l3")
    w = _wb(L)[0].clone()  # a weight no other test has packed
    b = _wb(L)[1]
    calls, real = [], _lib.lookup_conv_weights
    monkeypatch.setattr(_lib, "lookup_conv_weights", lambda weight: (calls.append(1), real(weight))[1])
    with torch.no_grad():
        cb = CorrBlock(torch.from_numpy(f1).to(DEV), torch.from_numpy(f2).to(DEV), num_levels=L, radius=R)
        a = cb.lookup_conv(c, w, b)
        o = blk.lookup_conv(c, w, b)
    assert len(calls) == 1
    assert norm_rel(o.cpu().numpy(), a.cpu().numpy()) <= REL_TOL


def _model(bins, alternate):
    from eraft_amd.model import ERAFT
    m = ERAFT({"subtype": "standard", "alternate_corr": alternate}, n_first_channels=bins).eval()
    with torch.no_grad():
        for name, t in m.state_dict().items():
            v = prng.param_init(name, tuple(t.shape))
            if v is not None:
                t.copy_(torch.from_numpy(v))
    return m


def _epe(a, b):
    a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    return float(np.sqrt(((a - b) ** 2).sum(1)).mean())


@pytest.mark.gpu
def test_model_with_the_switch(monkeypatch):
    """ERAFT at 128x160, 3 iterations, random-init weights: alternate_corr with fuse_ondemand_conv
    against alternate_corr alone and against alternate_corr off, EPE <= 0.01 px at both
    resolutions; then with all four inference switches as well and torch.nn.functional.conv2d
    made to raise, the on-demand forward completes: no torch convolution is left."""
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    from eraft_amd.ondemand import OnDemandConvCorrBlock
    monkeypatch.delenv("ERAFT_AMD_ONDEMAND", raising=False)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", True)
    bins, H, W = 5, 128, 160
    im1 = torch.from_numpy(prng.voxel_grid(121, (1, bins, H, W))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(123, (1, bins, H, W))).to(DEV)
    used = []
    real = OnDemandConvCorrBlock.lookup_conv
    monkeypatch.setattr(OnDemandConvCorrBlock, "lookup_conv", lambda self, *a, **k: (used.append(1), real(self, *a, **k))[1])
    flows = {}
    for key, alt, fuse in (("off", False, False), ("alt", True, False), ("fused", True, True)):
        monkeypatch.setattr(ERAFT, "fuse_ondemand_conv", fuse)
        m = _model(bins, alt).to(DEV)
        with torch.no_grad():
            low, ups = m(im1, im2, iters=3)
        assert len(used) == (3 if fuse else 0)
        flows[key] = (low, ups[-1])
    assert all(bool(torch.isfinite(t).all()) for t in flows["fused"])
    for other in ("alt", "off"):
        for k, what in ((0, "1/8 resolution"), (1, "full resolution")):
            epe = _epe(flows["fused"][k], flows[other][k])
            print(f"fuse_ondemand_conv against alternate_corr {other}, {what}: EPE {epe:.2e} px")
            assert epe <= 0.01
    # every switch on: the forward runs without a torch convolution
    for cls in (BasicEncoder, BasicUpdateBlock, SepConvGRU):
        monkeypatch.setattr(cls, "fused", True)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", True)
    m = _model(bins, True).to(DEV)
    with torch.no_grad():
        m(im1, im2, iters=3)  # the packs

        def refuse(*a, **k):
            raise AssertionError("torch.nn.functional.conv2d was called")

        monkeypatch.setattr(F, "conv2d", refuse)
        low, ups = m(im1, im2, iters=3)
    assert len(ups) == 3 and bool(torch.isfinite(low).all())
    for k, t in ((0, low), (1, ups[-1])):
        epe = _epe(t, flows["alt"][k])
        print(f"all switches on against alternate_corr alone, output {k}: EPE {epe:.2e} px")
        assert epe <= 0.01
