"""The mask head fused with the convex upsampling (corr_mask_upsample_*, csrc/corr_mask_upsample.hip;
eraft_amd/upsample.py; ERAFT.fuse_mask_upsample).

The yardstick of every parity test is the reference composition in fp64 on the CPU: the 1x1
convolution in fp64, times 0.25, then the torch branch of ERAFT.upsample_flow (the reference's
eraft.py:75-86) in fp64; the bound is REL_TOL, norm-relative.  Inputs come from prng.

CPU: the exports, the size function, the argument validation (all before any HIP call), the
Python layer's refusals, that the switch is inert on CPU tensors, and defer_mask.  GPU: parity at
the smallest shapes that reach every neighbour outside the map, a partial 16-pixel column block,
a row change inside a workgroup and a second batch item; tap / sub-pixel orientation bit for bit;
the output buffer's bounds; determinism and graph replay; re-packing; the module and the end-to-end
golden.

Measured on an MI355X (norm_rel against fp64; the torch fp32 chain beside it): see DESIGN.md §17.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
from _util import REL_TOL, bit_equal, load, norm_rel

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAMES = ("corr_mask_upsample_weights_bytes", "corr_mask_upsample_pack_weights", "corr_mask_upsample_forward")
DEV = "cuda:0"
SCALE = 0.25  # the reference's factor on the mask (update.py:106)


# ----------------------------------------------------------------------------------------------
# shared data (read-only by convention)
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _head(lscale):
    """mask[2]'s weight [576, 256] and bias [576], sized so that the logits 0.25 (W h + b) of a
    relu(gauss) hidden (mean square 1/2 per channel) have a standard deviation near `lscale`."""
    sigma = lscale / (SCALE * np.sqrt(256 * 0.5))
    return prng.gauss(901, (576, 256), sigma), prng.gauss(902, (576,), 0.1 * lscale / SCALE)


@functools.lru_cache(maxsize=None)
def _inputs(B, H, W):
    """hidden = relu(gauss) [B, 256, H, W] (as relu(mask[0](net))) and a flow [B, 2, H, W]."""
    hidden = np.maximum(prng.gauss(911, (B, 256, H, W)), 0.0).astype(np.float32)
    return hidden, prng.gauss(912, (B, 2, H, W), 3.0)


def _upsample64(flow, mask):
    """The torch branch of ERAFT.upsample_flow on fp64 CPU tensors."""
    from eraft_amd.model import ERAFT
    assert not flow.is_cuda and flow.dtype == torch.float64
    return ERAFT.upsample_flow(flow, mask)


@functools.lru_cache(maxsize=None)
def _ref64(B, H, W, lscale):
    w, b = _head(lscale)
    hidden, flow = _inputs(B, H, W)
    mask = SCALE * F.conv2d(torch.from_numpy(hidden).double(), torch.from_numpy(w).double().view(576, 256, 1, 1),
                            torch.from_numpy(b).double())
    return _upsample64(torch.from_numpy(flow).double(), mask).numpy()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fused(hidden, flow, w, b, embed=False, out=None, scale=SCALE):
    """mask_upsample_forward of numpy inputs; `embed`: hidden sits at channels 256 .. 511 of a
    buffer whose other channels hold 1e30."""
    from eraft_amd import _lib
    hg, off = _gpu(hidden), 0
    if embed:
        buf = torch.full((hidden.shape[0], 512) + hidden.shape[2:], 1e30, dtype=torch.float32, device=DEV)
        buf[:, 256:] = hg
        hg, off = buf, 256
    packed = _lib.mask_upsample_pack_weights(_gpu(w))
    return _lib.mask_upsample_forward(hg, off, _gpu(flow), packed, _gpu(b), scale, out=out)


def _torch_chain(hidden, flow, w, b):
    """What the kernel replaces, in fp32 on the GPU: 0.25 * mask[2](hidden), corr_convex_upsample."""
    from eraft_amd.model import ERAFT
    mask = SCALE * F.conv2d(_gpu(hidden), _gpu(w).view(576, 256, 1, 1), _gpu(b))
    return ERAFT.upsample_flow(_gpu(flow), mask)


# ----------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def test_exports_and_version(lib):
    from eraft_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.corr_version() == 202


def test_weights_bytes(lib):
    assert lib.corr_mask_upsample_weights_bytes() >= 576 * 256 * 6


# corr_mask_upsample_forward(hidden, hidden_channels, hidden_offset, flow, packed, bias, mask_scale, B, H, W, out, stream)
# (fake pointers, far enough apart that no buffer of these sizes overlaps another)
_GOOD = dict(hidden=0x10000000, hidden_channels=512, hidden_offset=256, flow=0x20000000, packed=0x30000000,
             bias=0x40000000, mask_scale=0.25, B=2, H=6, W=7, out=0x50000000, stream=None)
_PX = 2 * 6 * 7  # pixels of _GOOD


@pytest.mark.parametrize("change,code,msg", [
    (dict(hidden=None), EINVAL, "hidden is NULL"),
    (dict(flow=None), EINVAL, "flow is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(bias=None), EINVAL, "bias is NULL"),
    (dict(out=None), EINVAL, "out is NULL"),
    (dict(B=0), EINVAL, "B, H, W"),
    (dict(H=0), EINVAL, "B, H, W"),
    (dict(W=-3), EINVAL, "B, H, W"),
    (dict(hidden_offset=-1), EINVAL, "hidden_offset"),
    (dict(hidden_offset=257), EINVAL, "hidden_offset"),
    (dict(hidden_channels=255, hidden_offset=0), EINVAL, "hidden_offset"),
    (dict(packed=0x30000004), EINVAL, "packed is not 16-byte aligned"),
    (dict(mask_scale=float("inf")), EINVAL, "mask_scale"),
    (dict(mask_scale=float("-inf")), EINVAL, "mask_scale"),
    (dict(mask_scale=float("nan")), EINVAL, "mask_scale"),
    (dict(out=0x10000000), EINVAL, "overlap"),
    (dict(out=0x10000000 + 4 * (512 * _PX - 1)), EINVAL, "overlap"),   # the last float of hidden
    (dict(out=0x20000000 + 4 * (2 * _PX - 1)), EINVAL, "overlap"),     # the last float of flow
    (dict(out=0x20000000 - 4 * (128 * _PX - 1)), EINVAL, "overlap"),   # out's last float is flow's first
])
def test_forward_validation(lib, change, code, msg):
    """Every refusal comes before any HIP call (the pointers are never dereferenced)."""
    a = dict(_GOOD, **change)
    assert lib.corr_mask_upsample_forward(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


def test_forward_validation_accepts_what_it_should(lib):
    """A standalone hidden (offset 0 of 256), the last window of a wider buffer and buffers that
    touch without sharing a byte are fine: the refusals below come from the last check (the
    misaligned pack), not from these."""
    for change in (dict(hidden_channels=256, hidden_offset=0),
                   dict(hidden_channels=1024, hidden_offset=768),
                   dict(out=0x10000000 + 4 * 512 * _PX),      # out starts where hidden ends
                   dict(out=0x20000000 - 4 * 128 * _PX),      # out ends where flow starts
                   dict(mask_scale=-3.0), dict(mask_scale=0.0)):
        a = dict(_GOOD, packed=0x30000008, **change)
        assert lib.corr_mask_upsample_forward(*a.values()) == EINVAL, change
        assert "aligned" in lib.corr_last_error().decode(), change


def test_pack_validation(lib):
    assert lib.corr_mask_upsample_pack_weights(None, 16, None) == EINVAL
    assert "w is NULL" in lib.corr_last_error().decode()
    assert lib.corr_mask_upsample_pack_weights(16, None, None) == EINVAL
    assert "packed is NULL" in lib.corr_last_error().decode()
    assert lib.corr_mask_upsample_pack_weights(16, 20, None) == EINVAL
    assert "aligned" in lib.corr_last_error().decode()


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from eraft_amd import _lib
    from eraft_amd.upsample import mask_upsample
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.mask_upsample_pack_weights(torch.zeros(576, 256, 1, 1))
    with pytest.raises(ValueError, match="576, 256"):
        _lib.mask_upsample_pack_weights(torch.zeros(576, 128, 1, 1))
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.mask_upsample_forward(torch.zeros(1, 256, 4, 4), 0, torch.zeros(1, 2, 4, 4), torch.zeros(16),
                                   torch.zeros(576), 0.25)
    with pytest.raises(RuntimeError, match="MI355X"):
        mask_upsample(torch.nn.Conv2d(256, 576, 1), torch.zeros(1, 256, 4, 4), 0, torch.zeros(1, 2, 4, 4))


def test_switch_follows_the_environment_and_defaults_to_off():
    import os
    from eraft_amd.model import ERAFT
    assert ERAFT.fuse_mask_upsample is (os.environ.get("ERAFT_AMD_FUSE_UPSAMPLE", "0") == "1")


def test_block_switches_are_inert_on_cpu_and_defer_mask_returns_the_hidden(monkeypatch):
    from eraft_amd.model import BasicUpdateBlock
    from test_conv import _block, _block_inputs, _run
    m = _block()
    arrs = _block_inputs(3, 1, 6, 7)
    a = _run(m, arrs, dev="cpu")
    monkeypatch.setattr(BasicUpdateBlock, "fused", True, raising=False)
    b = _run(m, arrs, dev="cpu")
    for u, v in zip(a, b):
        assert bit_equal(u, v)
    ts = tuple(torch.from_numpy(x) for x in arrs)
    with torch.no_grad():
        net, hidden, delta = m(*ts, False, defer_mask=True)
        want = torch.relu(m.mask[0](net))
        assert bit_equal(hidden.numpy(), want.numpy())
        assert bit_equal(net.numpy(), a[0]) and bit_equal(delta.numpy(), a[2])
        assert bit_equal((0.25 * m.mask[2](hidden)).numpy(), a[1])


def test_model_switch_is_inert_on_cpu(monkeypatch):
    """A CPU ERAFT forward (the oracle's torch CorrBlock in place of the HIP one, as bench.py's CPU
    baseline runs it) with the switch forced on is bit-equal to the switch off."""
    import eraft_amd.model as M
    from oracle import torch_ops
    from test_e2e import _model

    class CpuCorrBlock:
        def __init__(self, f1, f2, num_levels=4, radius=4):
            self.levels, self.radius = torch_ops.cpu_build(f1, f2, num_levels), radius

        def __call__(self, coords):
            return torch_ops.cpu_lookup(self.levels, coords, self.radius)

    monkeypatch.setattr(M, "CorrBlock", CpuCorrBlock)
    model = _model(3)
    im1 = torch.from_numpy(prng.voxel_grid(21, (1, 3, 128, 160)))
    im2 = torch.from_numpy(prng.voxel_grid(23, (1, 3, 128, 160)))
    outs = []
    for on in (False, True):
        monkeypatch.setattr(M.ERAFT, "fuse_mask_upsample", on, raising=False)
        with torch.no_grad():
            low, ups = model(im1, im2, iters=2)
        outs.append([low.numpy()] + [u.numpy() for u in ups])
    for u, v in zip(*outs):
        assert np.isfinite(u).all() and bit_equal(u, v)


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1),    # every neighbour is outside the map
          (1, 1, 17),   # a partial second column block of one pixel
          (1, 3, 16),   # whole blocks: a workgroup's blocks lie in different rows
          (1, 5, 35),   # three blocks a row, the last partial; a workgroup wraps to the next row
          (2, 7, 9),    # partial blocks only, B > 1: a workgroup's blocks lie in different batch items
          (1, 8, 32)]   # whole blocks, an even number a row


@pytest.mark.gpu
@pytest.mark.parametrize("embed", [False, True])
@pytest.mark.parametrize("lscale", [1, 30])
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_parity(shape, lscale, embed):
    B, H, W = shape
    w, b = _head(lscale)
    hidden, flow = _inputs(B, H, W)
    ref = _ref64(B, H, W, lscale)
    got = _fused(hidden, flow, w, b, embed).cpu().numpy()
    e_torch = norm_rel(_torch_chain(hidden, flow, w, b).cpu().numpy(), ref)
    assert got.shape == (B, 2, 8 * H, 8 * W) and np.isfinite(got).all()
    e = norm_rel(got, ref)
    print(f"mask_upsample B={B} {H}x{W} logits ~{lscale} offset={256 * int(embed)}: fused {e:.2e}, "
          f"torch fp32 chain {e_torch:.2e}")
    assert e <= REL_TOL


def _winner(s):
    """The tap that wins sub-pixel s = 8i + j in the orientation test: all nine taps occur, and
    neighbours in i and in j get different taps."""
    return (5 * s + s // 8) % 9


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 5, 35)])
def test_tap_and_subpixel_orientation_bit_exact(shape):
    """Zero weights and a bias of 4000 on one tap per sub-pixel: the losing taps' exponentials
    are exactly 0, so every output is 8 * one flow neighbour (or 0 outside the map), bit for bit."""
    B, H, W = shape
    assert sorted({_winner(s) for s in range(64)}) == list(range(9))
    bias = np.zeros(576, np.float32)
    for s in range(64):
        bias[64 * _winner(s) + s] = 4000.0
    hidden, flow = _inputs(B, H, W)
    got = _fused(hidden, flow, np.zeros((576, 256), np.float32), bias).cpu().numpy()
    padded = np.zeros((B, 2, H + 2, W + 2), np.float32)
    padded[:, :, 1:-1, 1:-1] = np.float32(8.0) * flow
    want = np.empty((B, 2, 8 * H, 8 * W), np.float32)
    for s in range(64):
        k, i, j = _winner(s), s // 8, s % 8
        dy, dx = k // 3 - 1, k % 3 - 1
        want[:, :, i::8, j::8] = padded[:, :, 1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    assert bit_equal(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lead", [((2, 7, 9), 64), ((2, 7, 9), 3), ((1, 5, 35), 64)])
def test_buffer_discipline(shape, lead):
    """`out` inside a larger sentinel-filled buffer (16-byte aligned, and not): every output float
    is written and nothing outside the output is touched."""
    B, H, W = shape
    w, b = _head(1)
    hidden, flow = _inputs(B, H, W)
    n, sentinel = B * 2 * 64 * H * W, 0x4B3C2D1E
    big = torch.full((lead + n + 64,), sentinel, dtype=torch.int32, device=DEV).view(torch.float32)
    out = big[lead:lead + n].view(B, 2, 8 * H, 8 * W)
    assert out.data_ptr() % 16 == (4 * lead) % 16
    res = _fused(hidden, flow, w, b, out=out)
    assert res is out
    bits = big.view(torch.int32).cpu().numpy()
    assert (bits[:lead] == sentinel).all() and (bits[lead + n:] == sentinel).all()
    assert (bits[lead:lead + n] != sentinel).all()
    assert norm_rel(out.cpu().numpy(), _ref64(B, H, W, 1)) <= REL_TOL


@pytest.mark.gpu
def test_deterministic_and_capturable():
    from eraft_amd import _lib
    B, H, W = 2, 7, 9
    w, b = _head(1)
    hidden, flow = _inputs(B, H, W)
    hg, fg, bg = _gpu(hidden), _gpu(flow), _gpu(b)
    packed = _lib.mask_upsample_pack_weights(_gpu(w))  # outside the capture
    a = _lib.mask_upsample_forward(hg, 0, fg, packed, bg, SCALE)
    c = _lib.mask_upsample_forward(hg, 0, fg, packed, bg, SCALE)
    assert bit_equal(a.cpu().numpy(), c.cpu().numpy())
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        d = _lib.mask_upsample_forward(hg, 0, fg, packed, bg, SCALE)
    gph.replay()
    torch.cuda.synchronize()
    assert bit_equal(a.cpu().numpy(), d.cpu().numpy())


def _conv64(conv, hidden, flow):
    mask = SCALE * F.conv2d(torch.from_numpy(hidden).double(), conv.weight.detach().cpu().double(),
                            conv.bias.detach().cpu().double())
    return _upsample64(torch.from_numpy(flow).double(), mask).numpy()


@pytest.mark.gpu
def test_repack_follows_the_weights():
    from eraft_amd.upsample import mask_upsample
    B, H, W = 2, 7, 9
    hidden, flow = _inputs(B, H, W)
    w, b = _head(1)
    conv = torch.nn.Conv2d(256, 576, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(_gpu(w).view(576, 256, 1, 1))
        conv.bias.copy_(_gpu(b))
    hg, fg = _gpu(hidden), _gpu(flow)
    before = mask_upsample(conv, hg, 0, fg).cpu().numpy()
    assert norm_rel(before, _ref64(B, H, W, 1)) <= REL_TOL
    with torch.no_grad():
        conv.weight.copy_(_gpu(prng.gauss(903, (576, 256, 1, 1), float(np.std(w)))))
    after = mask_upsample(conv, hg, 0, fg).cpu().numpy()
    assert norm_rel(after, before) > 100 * REL_TOL
    assert norm_rel(after, _conv64(conv, hidden, flow)) <= REL_TOL
    # packing inside a capture is refused like the other packs
    with torch.no_grad():
        conv.bias.add_(1.0)
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="before a graph capture"):
        with torch.cuda.graph(gph):
            mask_upsample(conv, hg, 0, fg)


@pytest.mark.gpu
@pytest.mark.parametrize("block_fused", [False, True])
def test_block_defer_mask_then_mask_upsample(monkeypatch, block_fused):
    """defer_mask=True followed by mask_upsample against the module's torch path (mask, then
    corr_convex_upsample).  On the kernel path the hidden is a view of the stacked heads' buffer
    and is handed on as (buffer, 256) without a copy."""
    from eraft_amd.model import ERAFT, BasicUpdateBlock
    from eraft_amd.upsample import channel_window, mask_upsample
    from test_conv import _block, _block_inputs
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m = _block(DEV)
    ts = tuple(torch.from_numpy(a).to(DEV) for a in _block_inputs(71, 2, 7, 9))
    with torch.no_grad():
        monkeypatch.setattr(BasicUpdateBlock, "fused", False)
        net_t, mask_t, delta_t = m(*ts)
        flow = ts[3] + delta_t
        plain = ERAFT.upsample_flow(flow, mask_t).cpu().numpy()
        monkeypatch.setattr(BasicUpdateBlock, "fused", block_fused)
        net, hidden, delta = m(*ts, False, defer_mask=True)
        buf, off = channel_window(hidden)
        if block_fused:
            assert off == 256 and buf.shape[1] == 512 and buf.data_ptr() + 4 * 256 * 7 * 9 == hidden.data_ptr()
        else:
            assert off == 0 and buf is hidden
        up = mask_upsample(m.mask[2], buf, off, flow).cpu().numpy()
    assert norm_rel(net.cpu().numpy(), net_t.cpu().numpy()) <= REL_TOL
    assert norm_rel(delta.cpu().numpy(), delta_t.cpu().numpy()) <= REL_TOL
    e = norm_rel(up, plain)
    print(f"update block (3x3 kernels: {block_fused}) + mask_upsample against the torch path: {e:.2e}")
    assert e <= REL_TOL
    assert not bit_equal(up, plain)  # the kernel did run


def _small_model_and_images():
    from test_e2e import _model
    model = _model(3).to(DEV)
    im1 = torch.from_numpy(prng.voxel_grid(21, (2, 3, 128, 160))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(23, (2, 3, 128, 160))).to(DEV)
    return model, im1, im2


@pytest.mark.gpu
@pytest.mark.parametrize("lookup_conv", [False, True])
@pytest.mark.parametrize("others", [False, True])
def test_model_switch(monkeypatch, lookup_conv, others):
    """ERAFT at 128 x 160 (a 16 x 20 map), B = 2, three iterations, with the lookup fused into convc1
    or not and the other three switches on or off.  The predictions do not feed the recurrence, so
    with deterministic convolutions every iteration's mask inputs are the same bits with the switch
    on and off, and each prediction is held to REL_TOL against the switch off."""
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", lookup_conv)
    for cls in (BasicEncoder, BasicUpdateBlock, SepConvGRU):
        monkeypatch.setattr(cls, "fused", others)
    model, im1, im2 = _small_model_and_images()
    outs = []
    for on in (False, True):
        monkeypatch.setattr(ERAFT, "fuse_mask_upsample", on)
        with torch.no_grad():
            low, ups = model(im1, im2, iters=3)
        outs.append((low.cpu().numpy(), [u.cpu().numpy() for u in ups]))
    assert np.isfinite(outs[0][0]).all() and bit_equal(outs[0][0], outs[1][0])
    for k, (p, f) in enumerate(zip(outs[0][1], outs[1][1])):
        e = norm_rel(f, p)
        print(f"ERAFT switch (lookup+convc1 {lookup_conv}, other switches {others}) prediction {k}: {e:.2e}")
        assert f.shape == p.shape == (2, 2, 128, 160)
        assert e <= REL_TOL
        assert not bit_equal(f, p)  # the kernel did run


@pytest.mark.gpu
def test_model_under_autograd_takes_the_torch_path(monkeypatch):
    from eraft_amd.model import ERAFT
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    model, im1, im2 = _small_model_and_images()
    outs = []
    for on in (True, False):
        monkeypatch.setattr(ERAFT, "fuse_mask_upsample", on)
        low, ups = model(im1, im2, iters=2)
        assert all(u.grad_fn is not None for u in ups)
        outs.append([u.detach().cpu().numpy() for u in ups])
    for f, p in zip(*outs):
        assert np.isfinite(p).all() and bit_equal(f, p)


@pytest.mark.gpu
def test_model_capturable(monkeypatch):
    """After one eager forward (the packs) the forward with the switch on captures into a graph,
    and the replay gives the eager bits of the predictions."""
    from eraft_amd.model import ERAFT
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", True)
    model, im1, im2 = _small_model_and_images()
    with torch.no_grad():
        model(im1, im2, iters=2)
        _, eager = model(im1, im2, iters=2)
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            _, ups = model(im1, im2, iters=2)
        gph.replay()
        torch.cuda.synchronize()
    for u, v in zip(eager, ups):
        assert bool(torch.isfinite(u).all()) and bit_equal(u.cpu().numpy(), v.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("others", [False, True])
def test_e2e_with_fused_mask_upsample_matches_reference(monkeypatch, others):
    """The g_e2e_dsec golden, cold and warm start, with the switch on: alone, and with the other
    three switches on."""
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    from test_e2e import EPE_TOL, _epe, _model
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", True)
    for cls in (BasicEncoder, BasicUpdateBlock, SepConvGRU):
        monkeypatch.setattr(cls, "fused", others)
    g = load("g_e2e_dsec")
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W))).to(DEV)
    model = _model(bins).to(DEV)
    finit = torch.from_numpy(g["flow_init"]).to(DEV)
    with torch.no_grad():
        low, ups = model(im1, im2, iters=iters)
        low_w, ups_w = model(im1, im2, iters=iters, flow_init=finit)
    errs = (_epe(low.cpu().numpy(), g["low"]), _epe(ups[-1][..., ::4, ::4].cpu().numpy(), g["up_sub"]),
            _epe(low_w.cpu().numpy(), g["low_warm"]), _epe(ups_w[-1][..., ::4, ::4].cpu().numpy(), g["up_warm_sub"]))
    print(f"e2e fused mask + upsample (other switches {others}): cold low/up {errs[0]:.2e}/{errs[1]:.2e}, "
          f"warm low/up {errs[2]:.2e}/{errs[3]:.2e} px")
    assert all(e <= EPE_TOL for e in errs)
