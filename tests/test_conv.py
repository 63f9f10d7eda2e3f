"""The 3x3 convolution kernel (corr_conv_*, csrc/corr_conv.hip) and the update block built on it
(eraft_amd/update.py, BasicUpdateBlock.fused).

CPU: the exports, the size function and the argument validation (all before any HIP call), that
the module switch is inert on CPU tensors, and that the repository's BasicUpdateBlock agrees with
the reference's own (tests/golden/update_reference.npz, make_golden_update.py).  GPU: parity of
conv_forward with an fp64 CPU F.conv2d of the same formula within REL_TOL (norm-relative), the
output window, the tap order, determinism, graph capture, re-packing, the module switch, the
reference's BasicUpdateBlock and the end-to-end golden.

Measured on an MI355X (norm_rel against fp64; torch's own fp32 GPU result beside it): see
DESIGN.md §15.
"""
import copy
import functools
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
from _util import REL_TOL, bit_equal, load, norm_rel

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAMES = ("corr_conv_weights_bytes", "corr_conv_pack_weights", "corr_conv_forward")
DEV = "cuda:0"


# ----------------------------------------------------------------------------------------------
# shared data (read-only by convention)
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(cin, cout):
    """A list of Conv2d weights [*, cin, 3, 3] stacked to cout rows (two halves for the stacked
    heads' 512, one otherwise) and the bias [cout], from prng.param_init by name."""
    parts = (cout // 2, cout // 2) if cout == 512 else (cout,)
    ws = tuple(prng.param_init(f"conv{k}_{cin}_{n}.weight", (n, cin, 3, 3)) for k, n in enumerate(parts))
    return ws, prng.param_init(f"conv_{cin}_{cout}.bias", (cout,))


@functools.lru_cache(maxsize=None)
def _input(seed, B, C, H, W):
    return prng.gauss(seed, (B, C, H, W))


@functools.lru_cache(maxsize=None)
def _ref64(seed, B, H, W, ca, cb, cout):
    """The convolution before the activation, in fp64 on the CPU."""
    ws, bias = _weights(ca + cb, cout)
    x = torch.from_numpy(_input(seed, B, ca + cb, H, W)).double()
    w = torch.from_numpy(np.concatenate(ws)).double()
    return F.conv2d(x, w, torch.from_numpy(bias).double(), padding=1).numpy()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _fused(x, ca, ws, bias, relu, out=None, out_offset=0):
    """conv_forward of x split at channel ca into the kernel's two input pointers."""
    from eraft_amd import _lib
    xg = _gpu(x)
    a = xg[:, :ca].contiguous()
    b = xg[:, ca:].contiguous() if ca < x.shape[1] else None
    packed = _lib.conv_pack_weights([_gpu(w) for w in ws] if len(ws) > 1 else _gpu(ws[0]))
    cout = sum(w.shape[0] for w in ws)
    return _lib.conv_forward(a, b, packed, _gpu(bias), cout, relu, out=out, out_offset=out_offset)


def _block(dev="cpu"):
    from eraft_amd.model import BasicUpdateBlock
    m = BasicUpdateBlock().eval()
    with torch.no_grad():
        for name, t in m.state_dict().items():
            t.copy_(torch.from_numpy(prng.param_init(name, tuple(t.shape))))
    return m.to(dev)


@functools.lru_cache(maxsize=None)
def _block_inputs(seed, B, H, W, fused=False):
    """net, inp, corr, flow as make_golden_update.py makes them; with `fused` corr stands for
    relu(convc1(lookup)) [B, 256, H, W]."""
    net = np.tanh(prng.gauss(seed, (B, 128, H, W)).astype(np.float64)).astype(np.float32)
    inp = np.maximum(prng.gauss(seed + 1, (B, 128, H, W)), 0.0).astype(np.float32)
    corr = prng.gauss(seed + 2, (B, 324, H, W))
    if fused:
        corr = np.maximum(prng.gauss(seed + 2, (B, 256, H, W)), 0.0).astype(np.float32)
    return net, inp, corr, prng.gauss(seed + 3, (B, 2, H, W))


def _run(m, arrs, fused=False, dev=DEV, dtype=torch.float32):
    with torch.no_grad():
        out = m(*(torch.from_numpy(a).to(device=dev, dtype=dtype) for a in arrs), fused)
    return tuple(t.cpu().numpy() for t in out)


def _block64(m, arrs, fused=False):
    return _run(copy.deepcopy(m).cpu().double(), arrs, fused, "cpu", torch.float64)


# ----------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def test_exports(lib):
    from eraft_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name


def test_sizes(lib):
    for cout, cin in ((192, 256), (126, 256), (512, 128), (1, 32)):
        assert lib.corr_conv_weights_bytes(cout, cin) >= 9 * cin * ((cout + 15) // 16 * 16) * 6, (cout, cin)
    for cout, cin in ((192, 100), (192, 1056), (0, 256), (1025, 256)):
        assert lib.corr_conv_weights_bytes(cout, cin) == 0, (cout, cin)


# corr_conv_forward(in_a, ca, in_b, cb, B, H, W, packed, bias, cout, relu, out, out_channels, out_offset, stream)
# (fake pointers, far enough apart that no buffer of these sizes overlaps another)
_GOOD = dict(in_a=0x10000000, ca=192, in_b=0x20000000, cb=64, B=2, H=6, W=7, packed=0x30000000, bias=0x40000000,
             cout=126, relu=1, out=0x50000000, out_channels=256, out_offset=128, stream=None)


@pytest.mark.parametrize("change,code,msg", [
    (dict(ca=0), EUNSUPPORTED, "ca >= 32"),
    (dict(ca=48), EUNSUPPORTED, "multiples of 32"),
    (dict(cb=16), EUNSUPPORTED, "multiples of 32"),
    (dict(cb=-32), EUNSUPPORTED, "cb >= 0"),
    (dict(ca=1024, cb=32), EUNSUPPORTED, "<= 1024"),
    (dict(cout=0, out_offset=0), EUNSUPPORTED, "1 <= cout"),
    (dict(cout=1025, out_channels=2048), EUNSUPPORTED, "cout <= 1024"),
    (dict(in_a=None), EINVAL, "in_a is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(out=None), EINVAL, "out is NULL"),
    (dict(in_b=None), EINVAL, "in_b is NULL"),
    (dict(relu=2), EINVAL, "relu must be"),
    (dict(relu=-1), EINVAL, "relu must be"),
    (dict(out_offset=-1), EINVAL, "out_offset"),
    (dict(out_offset=131), EINVAL, "out_offset"),
    (dict(packed=0x30000004), EINVAL, "packed is not 16-byte aligned"),
    (dict(B=0), EINVAL, "B, H, W"),
    (dict(H=0), EINVAL, "B, H, W"),
    (dict(W=-3), EINVAL, "B, H, W"),
    (dict(out=0x10000000), EINVAL, "overlap"),
    (dict(out=0x10000000 + 4 * (2 * 192 * 42 - 1)), EINVAL, "overlap"),   # the last float of in_a
    (dict(out=0x20000000 - 4 * (2 * 256 * 42 - 1)), EINVAL, "overlap"),   # out's last float is in_b's first
])
def test_forward_validation(lib, change, code, msg):
    """Every refusal comes before any HIP call (the pointers are never dereferenced)."""
    a = dict(_GOOD, **change)
    assert lib.corr_conv_forward(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


def test_forward_validation_accepts_what_it_should(lib):
    """in_b is ignored when cb = 0, and buffers that touch without sharing a byte are fine: the
    refusals below come from a later check, not from these."""
    a = dict(_GOOD, ca=256, in_b=None, cb=0, packed=0x30000008)
    assert lib.corr_conv_forward(*a.values()) == EINVAL and "aligned" in lib.corr_last_error().decode()
    a = dict(_GOOD, out=0x10000000 + 4 * 2 * 192 * 42, packed=0x30000008)  # out starts where in_a ends
    assert lib.corr_conv_forward(*a.values()) == EINVAL and "aligned" in lib.corr_last_error().decode()


def test_pack_validation(lib):
    assert lib.corr_conv_pack_weights(16, 192, 100, 16, None) == EUNSUPPORTED
    assert lib.corr_conv_pack_weights(16, 0, 256, 16, None) == EUNSUPPORTED
    assert lib.corr_conv_pack_weights(None, 192, 256, 16, None) == EINVAL
    assert "w is NULL" in lib.corr_last_error().decode()
    assert lib.corr_conv_pack_weights(16, 192, 256, None, None) == EINVAL
    assert "packed is NULL" in lib.corr_last_error().decode()
    assert lib.corr_conv_pack_weights(16, 192, 256, 20, None) == EINVAL
    assert "aligned" in lib.corr_last_error().decode()


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from eraft_amd import _lib
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.conv_pack_weights(torch.zeros(64, 128, 3, 3))
    with pytest.raises(ValueError, match="3, 3"):
        _lib.conv_pack_weights(torch.zeros(64, 128, 1, 5))
    with pytest.raises(ValueError, match="equal cin"):
        _lib.conv_pack_weights([torch.zeros(64, 128, 3, 3), torch.zeros(64, 96, 3, 3)])
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.conv_forward(torch.zeros(1, 32, 4, 4), None, torch.zeros(16), None, 1, True)


def test_module_switch_is_inert_on_cpu(monkeypatch):
    from eraft_amd.model import BasicUpdateBlock
    m = _block()
    arrs = _block_inputs(3, 1, 6, 7)
    monkeypatch.setattr(BasicUpdateBlock, "fused", False, raising=False)
    a = _run(m, arrs, dev="cpu")
    monkeypatch.setattr(BasicUpdateBlock, "fused", True, raising=False)
    b = _run(m, arrs, dev="cpu")
    for u, v in zip(a, b):
        assert bit_equal(u, v)


def test_switch_follows_the_environment_and_defaults_to_off():
    import os
    from eraft_amd.model import BasicUpdateBlock
    assert BasicUpdateBlock.fused is (os.environ.get("ERAFT_AMD_FUSE_UPDATE", "0") == "1")


def test_update_block_refuses_cpu_tensors():
    from eraft_amd.update import update_block
    with pytest.raises(RuntimeError, match="MI355X"):
        update_block(_block(), *(torch.from_numpy(a) for a in _block_inputs(3, 1, 6, 7)))


def test_cpu_block_matches_reference_golden():
    """The restated module and the fixture agree before any GPU test leans on either."""
    g = load("update_reference")
    m = _block()
    for k, (seed, B, H, W) in enumerate(g["cases"].tolist()):
        out = _run(m, _block_inputs(seed, B, H, W), dev="cpu")
        for nm, o in zip(("net", "mask", "delta_flow"), out):
            assert norm_rel(o, g[f"{nm}{k}"]) <= REL_TOL, (nm, k)


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1),    # only the centre tap is inside the map
          (1, 3, 4),    # the halo covers the whole map
          (2, 7, 9),    # odd sizes, partial tiles, B > 1
          (1, 5, 35),   # more than two tiles along W
          (1, 13, 5)]   # more than two tiles along H
CHANNELS = [(256, 0, 192),   # convc2
            (128, 0, 64),    # convf2
            (192, 64, 126),  # conv: two pointers split away from 128, padded output rows
            (128, 0, 512),   # the stacked heads, packed from two weights
            (32, 32, 1)]     # the smallest channel counts
CASES = [(s, (192, 64, 126)) for s in SHAPES] + [((2, 7, 9), c) for c in CHANNELS if c != (192, 64, 126)]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape,chan", CASES)
def test_forward_parity(shape, chan, relu):
    (B, H, W), (ca, cb, cout) = shape, chan
    seed = 61
    ws, bias = _weights(ca + cb, cout)
    x = _input(seed, B, ca + cb, H, W)
    ref = _ref64(seed, B, H, W, ca, cb, cout)
    ref = np.maximum(ref, 0.0) if relu else ref
    got = _fused(x, ca, ws, bias, relu).cpu().numpy()
    t = F.conv2d(_gpu(x), _gpu(np.concatenate(ws)), _gpu(bias), padding=1)
    e_torch = norm_rel((F.relu(t) if relu else t).cpu().numpy(), ref)
    e = norm_rel(got, ref)
    print(f"conv B={B} {H}x{W} ca={ca} cb={cb} cout={cout} relu={int(relu)}: fused {e:.2e}, torch fp32 {e_torch:.2e}")
    assert got.shape == (B, cout, H, W) and np.isfinite(got).all()
    assert e <= REL_TOL


@pytest.mark.gpu
def test_output_window():
    """Only channels out_offset .. out_offset + cout - 1 are written: the rest of the buffer,
    the rows the pack pads 126 to 128 with included, keeps its bits."""
    B, H, W, ca, cb, cout, oc, off = 2, 7, 9, 192, 64, 126, 256, 128
    ws, bias = _weights(ca + cb, cout)
    sentinel = 0x4B3C2D1E
    out = torch.full((B, oc, H, W), sentinel, dtype=torch.int32, device=DEV).view(torch.float32)
    res = _fused(_input(61, B, ca + cb, H, W), ca, ws, bias, True, out=out, out_offset=off)
    assert res is out
    bits = out.view(torch.int32).cpu().numpy()
    assert (bits[:, :off] == sentinel).all() and (bits[:, off + cout:] == sentinel).all()
    ref = np.maximum(_ref64(61, B, H, W, ca, cb, cout), 0.0)
    assert norm_rel(out[:, off:off + cout].cpu().numpy(), ref) <= REL_TOL


@pytest.mark.gpu
def test_tap_order():
    B, H, W, ca, cb, cout = 1, 6, 7, 192, 64, 126
    ws, bias = _weights(ca + cb, cout)
    x = _input(63, B, ca + cb, H, W)
    out = _fused(x, ca, ws, bias, False).cpu().numpy()
    assert norm_rel(out, _ref64(63, B, H, W, ca, cb, cout)) <= REL_TOL
    w = ws[0]
    for name, v in (("transposed", w.transpose(0, 1, 3, 2)), ("flipped in ky", w[:, :, ::-1]),
                    ("flipped in kx", w[:, :, :, ::-1])):
        other = _fused(x, ca, (np.ascontiguousarray(v),), bias, False).cpu().numpy()
        assert norm_rel(other, out) > 100 * REL_TOL, name


@pytest.mark.gpu
def test_deterministic_and_capturable():
    from eraft_amd import _lib
    B, H, W, ca, cb, cout = 2, 7, 9, 192, 64, 126
    ws, bias = _weights(ca + cb, cout)
    xg = _gpu(_input(65, B, ca + cb, H, W))
    a_in, b_in, bg = xg[:, :ca].contiguous(), xg[:, ca:].contiguous(), _gpu(bias)
    packed = _lib.conv_pack_weights(_gpu(ws[0]))  # outside the capture
    a = _lib.conv_forward(a_in, b_in, packed, bg, cout, True)
    b = _lib.conv_forward(a_in, b_in, packed, bg, cout, True)
    assert bit_equal(a.cpu().numpy(), b.cpu().numpy())
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        c = _lib.conv_forward(a_in, b_in, packed, bg, cout, True)
    gph.replay()
    torch.cuda.synchronize()
    assert bit_equal(a.cpu().numpy(), c.cpu().numpy())


@pytest.mark.gpu
def test_module_capturable(monkeypatch):
    """The whole block captures once its packs exist, and two replays of the graph are bit-equal.
    The torch convolutions that remain (convc1, convf1, the GRU's, the heads' second ones) are
    asked for MIOpen's deterministic solvers: its default ones at this size are not
    bit-reproducible from run to run.  The eager call is compared within REL_TOL only."""
    from eraft_amd.model import BasicUpdateBlock
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    m = _block(DEV)
    ts = tuple(torch.from_numpy(a).to(DEV) for a in _block_inputs(67, 2, 7, 9))
    with torch.no_grad():
        m(*ts)  # the warm-up: the packs are made here, outside the capture
        a = m(*ts)
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            c = m(*ts)
        gph.replay()
        torch.cuda.synchronize()
        first = [t.cpu().numpy() for t in c]
        gph.replay()
        torch.cuda.synchronize()
    for u, v, w in zip(a, first, c):
        assert bit_equal(v, w.cpu().numpy())
        assert norm_rel(v, u.cpu().numpy()) <= REL_TOL


@pytest.mark.gpu
def test_repack_follows_the_weights(monkeypatch):
    from eraft_amd.model import BasicUpdateBlock
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    arrs = _block_inputs(69, 1, 6, 7)
    m = _block(DEV)
    before = _run(m, arrs)
    with torch.no_grad():
        neww = prng.param_init("another.weight", tuple(m.encoder.convc2.weight.shape))
        m.encoder.convc2.weight.copy_(torch.from_numpy(neww))
    after = _run(m, arrs)
    assert norm_rel(after[0], before[0]) > 100 * REL_TOL
    for o, r in zip(after, _block64(m, arrs)):
        assert norm_rel(o, r) <= REL_TOL
    # a fresh module (new tensors, very likely in the freed storage) never sees the old packs
    del m
    gc.collect()
    m2 = _block(DEV)
    fresh = _run(m2, arrs)
    for o, r, b in zip(fresh, _block64(m2, arrs), before):
        assert norm_rel(o, r) <= REL_TOL
        assert norm_rel(o, b) <= REL_TOL  # the same prng weights as the first module's


@pytest.mark.gpu
@pytest.mark.parametrize("fused_input", [False, True])
def test_module_switch(monkeypatch, fused_input):
    from eraft_amd.model import BasicUpdateBlock
    m = _block(DEV)
    arrs = _block_inputs(71, 2, 7, 9, fused_input)
    monkeypatch.setattr(BasicUpdateBlock, "fused", False)
    plain = _run(m, arrs, fused_input)
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    fused = _run(m, arrs, fused_input)
    for nm, p, f in zip(("net", "mask", "delta_flow"), plain, fused):
        assert not bit_equal(p, f), nm  # the kernels did run
        e = norm_rel(f, p)
        print(f"update block switch ({nm}, lookup fused with convc1: {fused_input}): {e:.2e}")
        assert e <= REL_TOL, nm
    # autograd recording: the torch path, untouched (with MIOpen's deterministic solvers, so that
    # two runs of the same torch code can be compared bit for bit: its default 3x3 solvers at this
    # size differ from run to run by themselves)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    ts = [torch.from_numpy(a).to(DEV) for a in arrs]
    ts[0].requires_grad_(True)
    out_f = m(*ts, fused_input)
    monkeypatch.setattr(BasicUpdateBlock, "fused", False)
    out_p = m(*ts, fused_input)
    for f, p in zip(out_f, out_p):
        assert f.grad_fn is not None
        assert bit_equal(f.detach().cpu().numpy(), p.detach().cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_gru", [False, True])
def test_matches_reference_golden(monkeypatch, fuse_gru):
    from eraft_amd.model import BasicUpdateBlock, SepConvGRU
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(SepConvGRU, "fused", fuse_gru)
    g = load("update_reference")
    m = _block(DEV)
    for k, (seed, B, H, W) in enumerate(g["cases"].tolist()):
        out = _run(m, _block_inputs(seed, B, H, W))
        for nm, o in zip(("net", "mask", "delta_flow"), out):
            e = norm_rel(o, g[f"{nm}{k}"])
            print(f"update golden B={B} {H}x{W} fused GRU={fuse_gru} {nm}: {e:.2e}")
            assert e <= REL_TOL, (nm, k)


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_gru", [False, True])
def test_e2e_with_fused_update_matches_reference(monkeypatch, fuse_gru):
    """The g_e2e_dsec golden, cold and warm start, with the update block on the 3x3 kernels."""
    from eraft_amd.model import BasicUpdateBlock, SepConvGRU
    from test_e2e import EPE_TOL, _epe, _model
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(SepConvGRU, "fused", fuse_gru)
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
    print(f"e2e fused update block (fused GRU={fuse_gru}): cold low/up {errs[0]:.2e}/{errs[1]:.2e}, "
          f"warm low/up {errs[2]:.2e}/{errs[3]:.2e} px")
    assert all(e <= EPE_TOL for e in errs)
