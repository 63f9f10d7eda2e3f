"""The update block's tail on its own kernels (corr_flow_enc_*, corr_flow_head_*, csrc/corr_flow.hip;
eraft_amd/update.py; BasicUpdateBlock.fused): the 7x7 convolution of the flow with the flow's
pass-through into the GRU input, and the flow head's 3x3 to 2 channels with the coordinate update.

The yardstick of every parity test is an fp64 CPU F.conv2d of the same formula; the bound is
REL_TOL, norm-relative (tests/_util.py), and EPE_TOL for whole forwards (tests/test_e2e.py).
Inputs and weights come from prng.

CPU: the exports, the size functions, the argument validation (all before any HIP call), the
Python layer's refusals, and that the switch is inert on CPU tensors.  GPU: parity at the smallest
shapes that reach every edge (a map smaller than the window, partial tiles, several tiles along
each axis, B > 1), the output windows and the pass-through bit for bit, the tap order, the
coordinate update bit for bit, determinism and graph replay, the module (no torch convolution
left), the reference's BasicUpdateBlock, a whole forward with torch's convolution disabled, and
the end-to-end golden.

Measured on an MI355X (norm_rel against fp64; torch's own fp32 GPU result beside it): see
DESIGN.md §19.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
from _util import REL_TOL, bit_equal, load, norm_rel

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAMES = ("corr_flow_enc_weights_bytes", "corr_flow_enc_pack_weights", "corr_flow_enc_forward",
         "corr_flow_head_weights_bytes", "corr_flow_head_pack_weights", "corr_flow_head_forward")
DEV = "cuda:0"
SENTINEL = 0x4B3C2D1E


# ----------------------------------------------------------------------------------------------
# shared data (read-only by convention)
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _enc_weights(cout):
    return prng.param_init(f"flow_enc_{cout}.weight", (cout, 2, 7, 7)), prng.param_init(f"flow_enc_{cout}.bias", (cout,))


@functools.lru_cache(maxsize=None)
def _flow(B, H, W):
    return prng.gauss(811, (B, 2, H, W), 3.0)


@functools.lru_cache(maxsize=None)
def _enc_ref64(B, H, W, cout):
    """The 7x7 convolution before the activation, in fp64 on the CPU."""
    w, b = _enc_weights(cout)
    return F.conv2d(torch.from_numpy(_flow(B, H, W)).double(), torch.from_numpy(w).double(),
                    torch.from_numpy(b).double(), padding=3).numpy()


@functools.lru_cache(maxsize=None)
def _head_weights():
    return prng.param_init("flow_head2.weight", (2, 256, 3, 3)), prng.param_init("flow_head2.bias", (2,))


@functools.lru_cache(maxsize=None)
def _hidden(B, H, W):
    """relu(gauss) [B, 256, H, W], as relu(flow_head.conv1(net))."""
    return np.maximum(prng.gauss(821, (B, 256, H, W)), 0.0).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _coords(B, H, W):
    """(coords_in, coords0): the pixel grid plus a flow of a few pixels, and the grid."""
    c0 = prng.coords_grid(B, H, W)
    return (c0 + prng.gauss(823, (B, 2, H, W), 2.0)).astype(np.float32), c0


@functools.lru_cache(maxsize=None)
def _head_ref64(B, H, W):
    w, b = _head_weights()
    return F.conv2d(torch.from_numpy(_hidden(B, H, W)).double(), torch.from_numpy(w).double(),
                    torch.from_numpy(b).double(), padding=1).numpy()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _enc(flow, w, b, relu, **kw):
    from eraft_amd import _lib
    return _lib.flow_enc_forward(_gpu(flow), _lib.flow_enc_pack_weights(_gpu(w)), _gpu(b), w.shape[0], relu, **kw)


def _embedded(hidden, off):
    """`hidden` at channels off .. off + 255 of a 512-channel buffer whose other half holds 1e6."""
    buf = torch.full((hidden.shape[0], 512) + hidden.shape[2:], 1e6, dtype=torch.float32, device=DEV)
    buf[:, off:off + 256] = _gpu(hidden)
    return buf


def _head(hidden, w, b, off=0, **kw):
    from eraft_amd import _lib
    return _lib.flow_head_forward(_embedded(hidden, off), off, _lib.flow_head_pack_weights(_gpu(w)), _gpu(b), **kw)


def _sentinels(shape):
    return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)


def _bits(t):
    return t.view(torch.int32).cpu().numpy()


# ----------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def test_exports_version_and_sizes(lib):
    from eraft_amd import _lib
    for name in NAMES:
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    assert lib.corr_version() == 202
    # the header: rows padded to a multiple of 64, four K steps of three pieces of 64 lanes x 16 bytes
    for cout in (1, 16, 63, 64, 100, 128, 1024):
        n = lib.corr_flow_enc_weights_bytes(cout)
        assert n == (cout + 63) // 64 * 64 // 16 * 4 * 3 * 64 * 16 and n % 16 == 0, cout
    for cout in (0, -1, 1025, 1 << 30):
        assert lib.corr_flow_enc_weights_bytes(cout) == 0, cout
    n = lib.corr_flow_head_weights_bytes()
    assert n >= 2 * 256 * 9 * 6 and n % 16 == 0


# corr_flow_enc_forward(flow, B, H, W, packed, bias, cout, relu, out, out_channels, out_offset, flow_copy,
#                       copy_channels, copy_offset, stream)
# (fake pointers, far enough apart that no buffer of these sizes overlaps another)
_ENC = dict(flow=0x10000000, B=2, H=6, W=7, packed=0x30000000, bias=0x40000000, cout=128, relu=1, out=0x50000000,
            out_channels=128, out_offset=0, flow_copy=0x60000000, copy_channels=256, copy_offset=254, stream=None)
_PX = 2 * 6 * 7  # pixels of _ENC and _HEAD


@pytest.mark.parametrize("change,code,msg", [
    (dict(flow=None), EINVAL, "flow is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(out=None), EINVAL, "out is NULL"),
    (dict(relu=2), EINVAL, "relu must be"),
    (dict(relu=-1), EINVAL, "relu must be"),
    (dict(out_offset=-1), EINVAL, "out_offset"),
    (dict(out_offset=1), EINVAL, "out_offset"),
    (dict(out_channels=127), EINVAL, "out_offset"),
    (dict(copy_offset=-1), EINVAL, "copy_offset"),
    (dict(copy_offset=255), EINVAL, "copy_offset"),
    (dict(copy_channels=1, copy_offset=0), EINVAL, "copy_offset"),
    (dict(packed=0x30000004), EINVAL, "packed is not 16-byte aligned"),
    (dict(B=0), EINVAL, "B, H, W"),
    (dict(H=0), EINVAL, "B, H, W"),
    (dict(W=-3), EINVAL, "B, H, W"),
    (dict(B=2048, H=1024, W=1024), EINVAL, "too large"),   # B*H*W = 2^31
    (dict(cout=0), EUNSUPPORTED, "1 <= cout <= 1024"),
    (dict(cout=1025, out_channels=2048), EUNSUPPORTED, "1 <= cout <= 1024"),
    (dict(out=0x10000000), EINVAL, "overlap"),
    (dict(out=0x10000000 + 4 * (2 * _PX - 1)), EINVAL, "overlap"),     # the last float of flow
    (dict(out=0x10000000 - 4 * (128 * _PX - 1)), EINVAL, "overlap"),   # out's last float is flow's first
    (dict(flow_copy=0x10000000), EINVAL, "overlap"),
    (dict(flow_copy=0x10000000 - 4 * (256 * _PX - 1)), EINVAL, "overlap"),
    (dict(flow_copy=0x50000000), EINVAL, "overlap"),                     # out's tensor with another channel count
    (dict(flow_copy=0x50000000 + 4), EINVAL, "overlap"),
    (dict(flow_copy=0x50000000, out_channels=256, out_offset=128), EINVAL, "overlap"),  # one tensor, windows meet
    (dict(flow_copy=0x50000000, out_channels=256, out_offset=127), EINVAL, "overlap"),
])
def test_flow_enc_validation(lib, change, code, msg):
    """Every refusal comes before any HIP call (the pointers are never dereferenced)."""
    a = dict(_ENC, **change)
    assert lib.corr_flow_enc_forward(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


def test_flow_enc_validation_accepts_what_it_should(lib):
    """No bias, no pass-through (its sizes then mean nothing), a window inside a wider buffer, one
    tensor written through disjoint windows and buffers that touch without sharing a byte are fine:
    the refusals below come from the last check (the misaligned pack), not from these."""
    for change in (dict(bias=None), dict(relu=0), dict(flow_copy=None, copy_channels=-5, copy_offset=99),
                   dict(out_channels=256, out_offset=128), dict(cout=1, out_channels=1), dict(cout=1024, out_channels=1024),
                   dict(flow_copy=0x50000000, out_channels=256, out_offset=0),
                   dict(flow_copy=0x50000000, out_channels=256, out_offset=126),
                   dict(out=0x10000000 + 4 * 2 * _PX),       # out starts where flow ends
                   dict(out=0x10000000 - 4 * 128 * _PX),     # out ends where flow starts
                   dict(B=1, H=1, W=1), dict(B=1, H=3, W=4)):
        a = dict(_ENC, packed=0x30000008, **change)
        assert lib.corr_flow_enc_forward(*a.values()) == EINVAL, change
        assert "aligned" in lib.corr_last_error().decode(), change


# corr_flow_head_forward(hidden, hidden_channels, hidden_offset, B, H, W, packed, bias, coords_in, coords0, delta,
#                        coords_out, flow_out, stream)
_HEAD = dict(hidden=0x10000000, hidden_channels=512, hidden_offset=0, B=2, H=6, W=7, packed=0x30000000,
             bias=0x40000000, coords_in=0x50000000, coords0=0x51000000, delta=0x52000000, coords_out=0x53000000,
             flow_out=0x54000000, stream=None)


@pytest.mark.parametrize("change,code,msg", [
    (dict(hidden=None), EINVAL, "hidden is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(bias=None), EINVAL, "bias is NULL"),
    (dict(delta=None), EINVAL, "delta is NULL"),
    (dict(coords_in=None), EINVAL, "coords0 needs coords_in"),
    (dict(coords_out=None), EINVAL, "coords_out is NULL"),
    (dict(flow_out=None), EINVAL, "flow_out is NULL"),
    (dict(hidden_offset=-1), EINVAL, "hidden_offset"),
    (dict(hidden_offset=257), EINVAL, "hidden_offset"),
    (dict(hidden_channels=255), EINVAL, "hidden_offset"),
    (dict(packed=0x30000004), EINVAL, "packed is not 16-byte aligned"),
    (dict(B=0), EINVAL, "B, H, W"),
    (dict(H=0), EINVAL, "B, H, W"),
    (dict(W=-3), EINVAL, "B, H, W"),
    (dict(B=2048, H=1024, W=1024), EINVAL, "too large"),
    (dict(delta=0x10000000), EINVAL, "overlap"),
    (dict(delta=0x10000000 + 4 * (512 * _PX - 1)), EINVAL, "overlap"),   # the last float of hidden
    (dict(flow_out=0x10000000 - 4 * (2 * _PX - 1)), EINVAL, "overlap"),  # flow_out's last float is hidden's first
    (dict(coords_out=0x50000000), EINVAL, "overlap"),                    # the in-place update
    (dict(coords_out=0x50000000 + 4 * (2 * _PX - 1)), EINVAL, "overlap"),
    (dict(delta=0x50000000), EINVAL, "overlap"),
    (dict(flow_out=0x51000000), EINVAL, "overlap"),
    (dict(coords_out=0x51000000), EINVAL, "overlap"),
    (dict(coords_out=0x52000000), EINVAL, "overlap"),                    # two outputs in one place
    (dict(flow_out=0x53000000), EINVAL, "overlap"),
])
def test_flow_head_validation(lib, change, code, msg):
    """Every refusal comes before any HIP call (the pointers are never dereferenced)."""
    a = dict(_HEAD, **change)
    assert lib.corr_flow_head_forward(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


def test_flow_head_validation_accepts_what_it_should(lib):
    """Only delta (outputs without their inputs are ignored, wherever they point), coordinates
    without coords0, a standalone hidden, the last window of a wider buffer and buffers that touch
    are fine: the refusals below come from the last check (the misaligned pack)."""
    for change in (dict(coords_in=None, coords0=None, coords_out=0x10000000, flow_out=0x10000000),
                   dict(coords_in=None, coords0=None, coords_out=None, flow_out=None),
                   dict(coords0=None, flow_out=None), dict(coords0=None, flow_out=0x50000000),
                   dict(hidden_channels=256), dict(hidden_channels=1024, hidden_offset=768),
                   dict(hidden_offset=256),
                   dict(delta=0x10000000 + 4 * 512 * _PX),   # delta starts where hidden ends
                   dict(delta=0x10000000 - 4 * 2 * _PX),     # delta ends where hidden starts
                   dict(B=1, H=1, W=1)):
        a = dict(_HEAD, packed=0x30000008, **change)
        assert lib.corr_flow_head_forward(*a.values()) == EINVAL, change
        assert "aligned" in lib.corr_last_error().decode(), change


def test_pack_validation(lib):
    assert lib.corr_flow_enc_pack_weights(None, 128, 16, None) == EINVAL
    assert "w is NULL" in lib.corr_last_error().decode()
    assert lib.corr_flow_enc_pack_weights(16, 128, None, None) == EINVAL
    assert "packed is NULL" in lib.corr_last_error().decode()
    assert lib.corr_flow_enc_pack_weights(16, 128, 20, None) == EINVAL
    assert "aligned" in lib.corr_last_error().decode()
    assert lib.corr_flow_enc_pack_weights(16, 0, 16, None) == EUNSUPPORTED
    assert lib.corr_flow_enc_pack_weights(16, 1025, 16, None) == EUNSUPPORTED
    assert "1 <= cout <= 1024" in lib.corr_last_error().decode()
    assert lib.corr_flow_head_pack_weights(None, 16, None) == EINVAL
    assert "w is NULL" in lib.corr_last_error().decode()
    assert lib.corr_flow_head_pack_weights(16, None, None) == EINVAL
    assert "packed is NULL" in lib.corr_last_error().decode()
    assert lib.corr_flow_head_pack_weights(16, 20, None) == EINVAL
    assert "aligned" in lib.corr_last_error().decode()


def test_python_layer_refuses_cpu_tensors_and_bad_shapes():
    from eraft_amd import _lib
    z = torch.zeros
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.flow_enc_pack_weights(z(128, 2, 7, 7))
    with pytest.raises(ValueError, match="2, 7, 7"):
        _lib.flow_enc_pack_weights(z(128, 3, 7, 7))
    with pytest.raises(ValueError, match="2, 7, 7"):
        _lib.flow_enc_pack_weights(z(128, 2, 3, 3))
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.flow_enc_forward(z(1, 2, 4, 4), z(16), z(128), 128, True)
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.flow_head_pack_weights(z(2, 256, 3, 3))
    with pytest.raises(ValueError, match="2, 256, 3, 3"):
        _lib.flow_head_pack_weights(z(2, 128, 3, 3))
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.flow_head_forward(z(1, 256, 4, 4), 0, z(16), z(2))


def test_switch_keys():
    from eraft_amd import update
    assert all(isinstance(update.USE_KERNEL[k], bool) for k in ("convf1", "flow_head2"))


def test_block_switch_is_inert_on_cpu(monkeypatch):
    """BasicUpdateBlock on CPU tensors with the switch on is bit-equal to the switch off, with and
    without the coordinate update in the call (which on the torch path is coords1 + delta and
    that - coords0, one fp32 operation each)."""
    from eraft_amd.model import BasicUpdateBlock
    from test_conv import _block, _block_inputs, _run
    m = _block()
    arrs = _block_inputs(3, 1, 6, 7)
    c1, c0 = (torch.from_numpy(a) for a in _coords(1, 6, 7))
    outs = []
    for on in (False, True):
        monkeypatch.setattr(BasicUpdateBlock, "fused", on, raising=False)
        plain = _run(m, arrs, dev="cpu")
        with torch.no_grad():
            five = m(*(torch.from_numpy(a) for a in arrs), coords1=c1, coords0=c0)
            four = m(*(torch.from_numpy(a) for a in arrs), coords1=c1)
        assert len(plain) == 3 and len(five) == 5 and four[4] is None
        outs.append(plain + tuple(t.numpy() for t in five) + (four[3].numpy(),))
    for u, v in zip(*outs):
        assert bit_equal(u, v)
    net, mask, delta, n5, m5, d5, co, fo, co4 = outs[1]
    assert bit_equal(n5, net) and bit_equal(m5, mask) and bit_equal(d5, delta)
    assert bit_equal(co, c1.numpy() + delta) and bit_equal(co4, co) and bit_equal(fo, co - c0.numpy())


# ----------------------------------------------------------------------------------------------
# GPU: the two kernels
# ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1),    # only the centre tap is inside the map
          (1, 3, 4),    # the window covers the whole map
          (2, 7, 9),    # odd sizes, partial tiles, B > 1
          (1, 5, 35),   # more than two tiles along W, H < 7
          (1, 13, 5)]   # more than two tiles along H, W < 7
# cout = 128 everywhere; at 2 x 7 x 9 also the smallest supported cout and one that is no multiple of 16
ENC_CASES = [(s, 128) for s in SHAPES] + [((2, 7, 9), 1), ((2, 7, 9), 100)]


@pytest.mark.gpu
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("shape,cout", ENC_CASES)
def test_flow_enc_parity(shape, cout, relu):
    B, H, W = shape
    w, b = _enc_weights(cout)
    flow = _flow(B, H, W)
    ref = _enc_ref64(B, H, W, cout)
    ref = np.maximum(ref, 0.0) if relu else ref
    got = _enc(flow, w, b, relu).cpu().numpy()
    t = F.conv2d(_gpu(flow), _gpu(w), _gpu(b), padding=3)
    e_torch = norm_rel((F.relu(t) if relu else t).cpu().numpy(), ref)
    e = norm_rel(got, ref)
    print(f"flow_enc B={B} {H}x{W} cout={cout} relu={int(relu)}: kernel {e:.2e}, torch fp32 {e_torch:.2e}")
    assert got.shape == (B, cout, H, W) and np.isfinite(got).all()
    assert e <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cout", [((2, 7, 9), 126), ((1, 5, 35), 128)])
def test_flow_enc_output_window_and_pass_through(shape, cout):
    """Only channels out_offset .. out_offset + cout - 1 of out and copy_offset, + 1 of the copy
    target change (the rows the pack pads 126 to 128 with are not stored); the copied flow is the
    input bit for bit."""
    B, H, W = shape
    w, b = _enc_weights(cout)
    flow = _flow(B, H, W)
    oc, off, cc, co = 200, 37, 256, 254
    out, copy = _sentinels((B, oc, H, W)), _sentinels((B, cc, H, W))
    res = _enc(flow, w, b, True, out=out, out_offset=off, flow_copy=copy, copy_offset=co)
    assert res is out
    bits, cbits = _bits(out), _bits(copy)
    assert (bits[:, :off] == SENTINEL).all() and (bits[:, off + cout:] == SENTINEL).all()
    assert (cbits[:, :co] == SENTINEL).all() and (cbits[:, co + 2:] == SENTINEL).all()
    assert bit_equal(copy[:, co:co + 2].cpu().numpy(), flow)
    assert norm_rel(out[:, off:off + cout].cpu().numpy(), np.maximum(_enc_ref64(B, H, W, cout), 0.0)) <= REL_TOL
    # one tensor through disjoint windows, as the header allows; without the copy nothing else is touched
    both = _sentinels((B, cc, H, W))
    _enc(flow, w, b, True, out=both, out_offset=0, flow_copy=both, copy_offset=co)
    bb = _bits(both)
    assert (bb[:, cout:co] == SENTINEL).all()
    assert bit_equal(both[:, co:].cpu().numpy(), flow) and bit_equal(both[:, :cout].cpu().numpy(), out[:, off:off + cout].cpu().numpy())


@pytest.mark.gpu
def test_flow_enc_tap_order():
    B, H, W, cout = 2, 7, 9, 128
    w, b = _enc_weights(cout)
    flow = _flow(B, H, W)
    out = _enc(flow, w, b, False).cpu().numpy()
    assert norm_rel(out, _enc_ref64(B, H, W, cout)) <= REL_TOL
    for name, v in (("transposed", w.transpose(0, 1, 3, 2)), ("flipped in ky", w[:, :, ::-1]),
                    ("flipped in kx", w[:, :, :, ::-1]), ("input channels swapped", w[:, ::-1])):
        other = _enc(flow, np.ascontiguousarray(v), b, False).cpu().numpy()
        assert norm_rel(other, out) > 100 * REL_TOL, name


@pytest.mark.gpu
@pytest.mark.parametrize("off", [0, 256])
@pytest.mark.parametrize("shape", SHAPES)
def test_flow_head_parity_and_coordinate_update(shape, off):
    """delta against fp64; coords_out and flow_out bit for bit from the kernel's own delta.  The
    other half of the 512-channel buffer holds 1e6, so a wrong offset or batch stride cannot pass."""
    B, H, W = shape
    w, b = _head_weights()
    hidden = _hidden(B, H, W)
    cin, c0 = _coords(B, H, W)
    ref = _head_ref64(B, H, W)
    delta, cout, fout = (t.cpu().numpy() for t in _head(hidden, w, b, off, coords_in=_gpu(cin), coords0=_gpu(c0)))
    e_torch = norm_rel(F.conv2d(_gpu(hidden), _gpu(w), _gpu(b), padding=1).cpu().numpy(), ref)
    e = norm_rel(delta, ref)
    print(f"flow_head B={B} {H}x{W} offset={off}: kernel {e:.2e}, torch fp32 {e_torch:.2e}")
    assert delta.shape == (B, 2, H, W) and np.isfinite(delta).all()
    assert e <= REL_TOL
    assert bit_equal(cout, cin + delta)
    assert bit_equal(fout, cout - c0)
    assert bit_equal(cout, (_gpu(cin) + _gpu(delta)).cpu().numpy())  # torch's own fp32 add on the GPU


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 5, 35)])
def test_flow_head_writes_only_what_it_is_asked_for(shape):
    B, H, W = shape
    w, b = _head_weights()
    hidden = _hidden(B, H, W)
    cin, c0 = _coords(B, H, W)
    n = B * 2 * H * W
    # delta inside a larger buffer; without coords_in the other two outputs keep their bits
    big, co, fo = _sentinels((16 + n + 16,)), _sentinels((B, 2, H, W)), _sentinels((B, 2, H, W))
    d = big[16:16 + n].view(B, 2, H, W)
    res = _head(hidden, w, b, 256, delta=d, coords_out=co, flow_out=fo)
    assert res[0] is d and res[1] is None and res[2] is None
    bits = _bits(big)
    assert (bits[:16] == SENTINEL).all() and (bits[16 + n:] == SENTINEL).all() and (bits[16:16 + n] != SENTINEL).all()
    assert (_bits(co) == SENTINEL).all() and (_bits(fo) == SENTINEL).all()
    assert norm_rel(d.cpu().numpy(), _head_ref64(B, H, W)) <= REL_TOL
    # with coords_in and no coords0: coords_out too, flow_out still untouched; the same delta bits
    d2, co2, none = _head(hidden, w, b, 256, coords_in=_gpu(cin), coords_out=co, flow_out=fo)
    assert co2 is co and none is None and (_bits(fo) == SENTINEL).all()
    assert bit_equal(d2.cpu().numpy(), d.cpu().numpy()) and bit_equal(co.cpu().numpy(), cin + d2.cpu().numpy())


@pytest.mark.gpu
def test_flow_head_tap_order():
    B, H, W = 2, 7, 9
    w, b = _head_weights()
    hidden = _hidden(B, H, W)
    out = _head(hidden, w, b)[0].cpu().numpy()
    assert norm_rel(out, _head_ref64(B, H, W)) <= REL_TOL
    for name, v in (("transposed", w.transpose(0, 1, 3, 2)), ("flipped in ky", w[:, :, ::-1]),
                    ("flipped in kx", w[:, :, :, ::-1]), ("output rows swapped", w[::-1])):
        other = _head(hidden, np.ascontiguousarray(v), b)[0].cpu().numpy()
        assert norm_rel(other, out) > 100 * REL_TOL, name


@pytest.mark.gpu
def test_deterministic_and_capturable():
    """Two eager calls are bit-equal, and so are two replays of a graph captured after the packs
    were made."""
    from eraft_amd import _lib
    B, H, W, cout = 2, 7, 9, 128
    we, be = _enc_weights(cout)
    wh, bh = _head_weights()
    fg, hg = _gpu(_flow(B, H, W)), _embedded(_hidden(B, H, W), 0)
    cin, c0 = (_gpu(a) for a in _coords(B, H, W))
    pe, ph, beg, bhg = _lib.flow_enc_pack_weights(_gpu(we)), _lib.flow_head_pack_weights(_gpu(wh)), _gpu(be), _gpu(bh)

    def run():
        x = torch.zeros((B, 256, H, W), dtype=torch.float32, device=DEV)
        f1 = _lib.flow_enc_forward(fg, pe, beg, cout, True, flow_copy=x, copy_offset=254)
        return (f1, x) + _lib.flow_head_forward(hg, 0, ph, bhg, coords_in=cin, coords0=c0)

    a = [t.cpu().numpy() for t in run()]
    for u, v in zip(a, run()):
        assert bit_equal(u, v.cpu().numpy())
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        c = run()
    for _ in range(2):
        gph.replay()
        torch.cuda.synchronize()
        for u, v in zip(a, c):
            assert bit_equal(u, v.cpu().numpy())


@pytest.mark.gpu
def test_packing_inside_a_capture_raises():
    from eraft_amd import update
    from test_conv import _block
    m = _block(DEV)
    torch.cuda.synchronize()
    for pack, conv in ((update._flow_enc_pack, m.encoder.convf1), (update._flow_head_pack, m.flow_head.conv2)):
        gph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="before a graph capture"):
            with torch.cuda.graph(gph):
                pack(conv)
        first = pack(conv)   # outside a capture it packs, and the next call finds the cache
        assert pack(conv)[0] is first[0]
    # another kind of pack of the same convolution's tensors has a cache entry of its own
    from eraft_amd import _lib
    other = update._conv_pack((m.flow_head.conv2,))[0]
    assert other.numel() * 4 >= _lib.load().corr_conv_weights_bytes(2, 256) > first[0].numel() * 4
    assert update._flow_head_pack(m.flow_head.conv2)[0] is first[0]


# ----------------------------------------------------------------------------------------------
# GPU: the module
# ----------------------------------------------------------------------------------------------
def _count_conv2d(monkeypatch):
    calls = []
    real = F.conv2d

    def counted(x, w, *a, **k):
        calls.append(tuple(w.shape))
        return real(x, w, *a, **k)

    monkeypatch.setattr(F, "conv2d", counted)
    return calls


@pytest.mark.gpu
@pytest.mark.parametrize("fused_input", [False, True])
def test_module_leaves_no_torch_convolution(monkeypatch, fused_input):
    """With the block's and the GRU's switches on and the mask deferred, F.conv2d is called for
    convc1 only, and not at all when the lookup already went through convc1."""
    from eraft_amd.model import BasicUpdateBlock, SepConvGRU
    from test_conv import _block, _block64, _block_inputs
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(SepConvGRU, "fused", True)
    m = _block(DEV)
    arrs = _block_inputs(71, 2, 7, 9, fused_input)
    ts = tuple(torch.from_numpy(a).to(DEV) for a in arrs)
    calls = _count_conv2d(monkeypatch)
    with torch.no_grad():
        net, hidden, delta = m(*ts, fused_input, defer_mask=True)
    assert calls == ([] if fused_input else [(256, 324, 1, 1)])
    r_net, _, r_delta = _block64(m, arrs, fused_input)
    assert norm_rel(net.cpu().numpy(), r_net) <= REL_TOL and norm_rel(delta.cpu().numpy(), r_delta) <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("fused_input", [False, True])
def test_module_switch(monkeypatch, fused_input):
    """The block with the switch on against the switch off and against the fp64 module; each of the
    two new keys set False in turn (that piece back on torch); the coordinate update bit for bit;
    a workspace kept across calls; and under autograd recording the torch path, untouched."""
    from eraft_amd import update
    from eraft_amd.model import BasicUpdateBlock
    from test_conv import _block, _block64, _block_inputs, _run
    m = _block(DEV)
    arrs = _block_inputs(71, 2, 7, 9, fused_input)
    ref64 = _block64(m, arrs, fused_input)
    monkeypatch.setattr(BasicUpdateBlock, "fused", False)
    plain = _run(m, arrs, fused_input)
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    ts = tuple(torch.from_numpy(a).to(DEV) for a in arrs)
    c1, c0 = (_gpu(a) for a in _coords(2, 7, 9))
    for off_key in (None, "convf1", "flow_head2"):
        if off_key:
            monkeypatch.setitem(update.USE_KERNEL, off_key, False)
        fused = _run(m, arrs, fused_input)
        for nm, p, f, r in zip(("net", "mask", "delta_flow"), plain, fused, ref64):
            e, e64, p64 = norm_rel(f, p), norm_rel(f, r), norm_rel(p, r)
            print(f"update block tail ({nm}, lookup fused with convc1: {fused_input}, on torch: {off_key}): "
                  f"against the switch off {e:.2e}, against fp64 {e64:.2e} (switch off against fp64 {p64:.2e})")
            assert e <= REL_TOL and e64 <= REL_TOL, nm
        with torch.no_grad():
            ws = update.UpdateWorkspace(ts[1])
            first = m(*ts, fused_input, workspace=ws, coords1=c1, coords0=c0)
            kept = [t.cpu().numpy() for t in first]
            again = m(*ts, fused_input, workspace=ws, coords1=first[3], coords0=c0)
        assert bit_equal(ws.x[:, :128].cpu().numpy(), arrs[1]) and bit_equal(ws.x[:, 254:].cpu().numpy(), arrs[3])
        for k in range(3):
            assert norm_rel(kept[k], fused[k]) <= REL_TOL
            assert norm_rel(again[k].cpu().numpy(), fused[k]) <= REL_TOL
        assert bit_equal(kept[3], c1.cpu().numpy() + kept[2]) and bit_equal(kept[4], kept[3] - c0.cpu().numpy())
        # the second call wrote the other pair of buffers: the first call's results are still there
        assert bit_equal(first[3].cpu().numpy(), kept[3]) and bit_equal(first[4].cpu().numpy(), kept[4])
        assert bit_equal(again[3].cpu().numpy(), kept[3] + again[2].cpu().numpy())
        if off_key:
            monkeypatch.setitem(update.USE_KERNEL, off_key, True)
    assert not bit_equal(plain[2], fused[2])  # the kernels did run
    # autograd recording: the torch path (with MIOpen's deterministic solvers, as test_conv.test_module_switch)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    ts = [torch.from_numpy(a).to(DEV) for a in arrs]
    ts[0].requires_grad_(True)
    out_f = m(*ts, fused_input, coords1=c1, coords0=c0)
    monkeypatch.setattr(BasicUpdateBlock, "fused", False)
    out_p = m(*ts, fused_input, coords1=c1, coords0=c0)
    assert len(out_f) == len(out_p) == 5
    for f, p in zip(out_f, out_p):
        assert f.grad_fn is not None
        assert bit_equal(f.detach().cpu().numpy(), p.detach().cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_gru", [False, True])
def test_matches_reference_golden(monkeypatch, fuse_gru):
    from eraft_amd.model import BasicUpdateBlock, SepConvGRU
    from test_conv import _block, _block_inputs, _run
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(SepConvGRU, "fused", fuse_gru)
    g = load("update_reference")
    m = _block(DEV)
    for k, (seed, B, H, W) in enumerate(g["cases"].tolist()):
        out = _run(m, _block_inputs(seed, B, H, W))
        for nm, o in zip(("net", "mask", "delta_flow"), out):
            e = norm_rel(o, g[f"{nm}{k}"])
            print(f"update golden with the tail kernels B={B} {H}x{W} fused GRU={fuse_gru} {nm}: {e:.2e}")
            assert e <= REL_TOL, (nm, k)


# ----------------------------------------------------------------------------------------------
# GPU: the whole forward
# ----------------------------------------------------------------------------------------------
def _all_switches(monkeypatch, on):
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    for cls in (BasicEncoder, BasicUpdateBlock, SepConvGRU):
        monkeypatch.setattr(cls, "fused", on)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", on)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", True)


# The smallest image whose four pyramid levels all have two cells a side: 16 x 16 cells.  A 64 x 96
# image (8 x 12 cells) passes the size check, but its 1 x 1 last level makes the lookup NaN with
# every switch on or off, as it does in the reference (include/corr_mi355x.h: a level of height or
# width 1 divides by W_l - 1 = 0), so no flow could be compared there.
IMAGE = (128, 128)


@pytest.mark.gpu
def test_whole_forward_without_a_torch_convolution(monkeypatch):
    """ERAFT in eval mode with all four switches on: after one warm-up forward (the packs),
    torch.nn.functional.conv2d is made to raise and the forward still completes; its flow agrees
    with an all-switches-off forward of the same model within EPE_TOL."""
    from test_e2e import EPE_TOL, _epe, _model
    model = _model(15).to(DEV)
    im1 = torch.from_numpy(prng.voxel_grid(31, (1, 15) + IMAGE)).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(33, (1, 15) + IMAGE)).to(DEV)
    _all_switches(monkeypatch, False)
    with torch.no_grad():
        low_p, ups_p = model(im1, im2, iters=3)
    _all_switches(monkeypatch, True)
    with torch.no_grad():
        model(im1, im2, iters=3)

        def refuse(*a, **k):
            raise AssertionError("torch.nn.functional.conv2d was called")

        monkeypatch.setattr(F, "conv2d", refuse)
        low, ups = model(im1, im2, iters=3)
    errs = [_epe(low.cpu().numpy(), low_p.cpu().numpy())] + [_epe(u.cpu().numpy(), p.cpu().numpy())
                                                              for u, p in zip(ups, ups_p)]
    print("whole forward, all switches on against all off: EPE low / predictions "
          + " ".join(f"{e:.2e}" for e in errs) + " px")
    assert len(ups) == 3 and ups[-1].shape == (1, 2) + IMAGE and bool(torch.isfinite(low).all())
    assert all(e <= EPE_TOL for e in errs)


@pytest.mark.gpu
def test_e2e_with_all_switches_matches_reference(monkeypatch):
    """The g_e2e_dsec golden, cold and warm start, with all four switches on."""
    from test_e2e import EPE_TOL, _epe, _model
    _all_switches(monkeypatch, True)
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
    print(f"e2e with all four switches: cold low/up {errs[0]:.2e}/{errs[1]:.2e}, "
          f"warm low/up {errs[2]:.2e}/{errs[3]:.2e} px")
    assert all(e <= EPE_TOL for e in errs)
