"""The encoders around their residual stages on the project's kernels (corr_enc_stem_*, corr_enc_pw_*,
corr_enc_join_affine, csrc/corr_enc_front.hip) and the module built on them (eraft_amd/encoder.py).

CPU: the exports, the size functions, the argument validation (all before any HIP call), the
wrappers' refusal of CPU tensors, and that the module switch is inert on CPU tensors.  GPU: parity
of the stem and of the pointwise convolution with an fp64 CPU F.conv2d within REL_TOL
(norm-relative), that stride 2 reads even positions only, the statistics, the join, determinism,
graph capture, buffer discipline, and the module: no torch convolution or norm left, the
reference's golden, the per-piece fallbacks and the end-to-end golden.

Measured on an MI355X (norm_rel against fp64; torch's own fp32 GPU result beside it): see
DESIGN.md §18.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import prng
from _util import REL_TOL, bit_equal, load, norm_rel
from make_golden_encoder import CASES as GOLDEN_CASES, NORMS, OUTPUT_DIM, encoder_input, fill

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAMES = ("corr_enc_stem_weights_bytes", "corr_enc_stem_pack_weights", "corr_enc_stem_forward",
         "corr_enc_pw_weights_bytes", "corr_enc_pw_pack_weights", "corr_enc_pw_forward", "corr_enc_join_affine")
NEW_KEYS = ("stem", "layer2.proj", "layer3.proj", "head")
DEV = "cuda:0"
EPS = 1e-5


# ----------------------------------------------------------------------------------------------
# shared data (read-only by convention)
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(kind, cin, cout):
    k = 7 if kind == "stem" else 1
    return (prng.param_init(f"{kind}_{cin}_{cout}.weight", (cout, cin, k, k)),
            prng.param_init(f"{kind}_{cin}_{cout}.bias", (cout,)))


@functools.lru_cache(maxsize=None)
def _input(seed, B, C, H, W, mean=0.0):
    return (mean + prng.gauss(seed, (B, C, H, W))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _affine_pair(seed, B, C, per_batch):
    shape = (B, C) if per_batch else (C,)
    return ((1.0 + 0.5 * prng.gauss(seed + 1, shape)).astype(np.float32),
            (0.3 * prng.gauss(seed + 2, shape)).astype(np.float32))


@functools.lru_cache(maxsize=None)
def _ref64(kind, seed, B, H, W, cin, cout, stride, mean):
    w, bias = _weights(kind, cin, cout)
    x = _input(seed, B, cin, H, W, mean).astype(np.float64)
    return F.conv2d(torch.from_numpy(x), torch.from_numpy(w).double(), torch.from_numpy(bias).double(),
                    stride=stride, padding=3 if kind == "stem" else 0).numpy()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _stem(x, w, bias, stats=False):
    from eraft_amd import _lib
    return _lib.enc_stem_forward(_gpu(x), _lib.enc_stem_pack_weights(_gpu(w)), _gpu(bias), w.shape[0], stats)


def _pw(x, w, bias, stride, stats=False):
    from eraft_amd import _lib
    return _lib.enc_pw_forward(_gpu(x), _lib.enc_pw_pack_weights(_gpu(w)), _gpu(bias), w.shape[0], stride, stats)


def _bcast(t, B, C):
    return t.reshape((B, C, 1, 1) if t.ndim == 2 else (1, C, 1, 1))


def _encoder(norm, C, dev="cpu"):
    from eraft_amd.model import BasicEncoder
    return fill(BasicEncoder(output_dim=OUTPUT_DIM, norm_fn=norm, n_first_channels=C).eval()).to(dev)


def _run(m, x, dev=DEV):
    with torch.no_grad():
        return m(torch.from_numpy(x).to(dev)).cpu().numpy()


def _all_keys(monkeypatch, value=True):
    from eraft_amd import encoder
    for k in encoder.USE_KERNEL:
        monkeypatch.setitem(encoder.USE_KERNEL, k, value)


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
    assert lib.corr_version() == 202


def test_size_functions(lib):
    """The packs hold at least three bf16 pieces (6 bytes) per weight of the padded K."""
    for cout, cin in ((64, 15), (64, 5), (64, 3), (1, 1), (64, 16), (1024, 16)):
        assert lib.corr_enc_stem_weights_bytes(cout, cin) >= cout * 16 * 49 * 6
    for cout, cin in ((96, 64), (128, 96), (256, 128), (1, 32), (1024, 1024)):
        assert lib.corr_enc_pw_weights_bytes(cout, cin) >= cout * cin * 6
    for bad in ((0, 15), (64, 0), (-1, 15), (64, -3), (1025, 15), (64, 17)):
        assert lib.corr_enc_stem_weights_bytes(*bad) == 0, bad
    for bad in ((0, 64), (96, 0), (-1, 64), (96, -32), (96, 48), (1025, 64), (96, 1056)):
        assert lib.corr_enc_pw_weights_bytes(*bad) == 0, bad


# (fake pointers, far enough apart that no buffer of these sizes overlaps another)
# corr_enc_stem_forward(in, cin, B, H, W, packed, bias, cout, out, stats, stats_bytes, stream)
_STEM = dict(inp=0x10000000, cin=15, B=2, H=6, W=7, packed=0x30000000, bias=0x40000000, cout=64, out=0x50000000,
             stats=0x60000000, stats_bytes=2 * 64 * 8, stream=None)
# corr_enc_pw_forward(in, cin, B, H, W, stride, packed, bias, cout, out, stats, stats_bytes, stream)
_PW = dict(inp=0x10000000, cin=64, B=2, H=6, W=7, stride=2, packed=0x30000000, bias=0x40000000, cout=96,
           out=0x50000000, stats=0x60000000, stats_bytes=2 * 96 * 8, stream=None)
# corr_enc_join_affine(y, scale, shift, norm_per_batch, skip, skip_scale, skip_shift, skip_per_batch, skip_relu,
#                      B, C, H, W, out, stream)
_JOIN = dict(y=16, scale=32, shift=48, nb=1, skip=64, kscale=80, kshift=96, knb=0, krelu=1, B=2, C=96, H=3, W=4,
             out=112, stream=None)


@pytest.mark.parametrize("change,code,msg", [
    (dict(cin=0), EINVAL, "cin must be >= 1"),
    (dict(cin=-2), EINVAL, "cin must be >= 1"),
    (dict(cin=17), EUNSUPPORTED, "cin <= 16"),
    (dict(cout=0), EUNSUPPORTED, "1 <= cout"),
    (dict(cout=1025), EUNSUPPORTED, "cout <= 1024"),
    (dict(inp=None), EINVAL, "in is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(out=None), EINVAL, "out is NULL"),
    (dict(stats_bytes=2 * 64 * 8 - 1), EINVAL, "stats of"),
    (dict(W=40, stats_bytes=2 * 64 * 8), EINVAL, "stats of"),   # 3 x 20 outputs are two tiles
    (dict(packed=0x30000004), EINVAL, "packed is not 16-byte aligned"),
    (dict(B=0), EINVAL, "B, H, W"),
    (dict(H=0), EINVAL, "B, H, W"),
    (dict(W=-3), EINVAL, "B, H, W"),
    (dict(out=0x10000000), EINVAL, "overlap"),
    (dict(out=0x10000000 + 4 * (2 * 15 * 42 - 1)), EINVAL, "overlap"),   # the last float of in
    (dict(out=0x10000000 - 4 * (2 * 64 * 12 - 1)), EINVAL, "overlap"),   # out's last float is in's first
])
def test_stem_validation(lib, change, code, msg):
    """Every refusal comes before any HIP call (the pointers are never dereferenced)."""
    a = dict(_STEM, **change)
    assert lib.corr_enc_stem_forward(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


@pytest.mark.parametrize("change,code,msg", [
    (dict(stride=0), EUNSUPPORTED, "stride"),
    (dict(stride=3), EUNSUPPORTED, "stride"),
    (dict(cin=0), EUNSUPPORTED, "multiple of 32"),
    (dict(cin=48), EUNSUPPORTED, "multiple of 32"),
    (dict(cin=1056), EUNSUPPORTED, "32 .. 1024"),
    (dict(cout=0), EUNSUPPORTED, "1 <= cout"),
    (dict(cout=1025), EUNSUPPORTED, "cout <= 1024"),
    (dict(inp=None), EINVAL, "in is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(out=None), EINVAL, "out is NULL"),
    (dict(stats_bytes=2 * 96 * 8 - 1), EINVAL, "stats of"),
    (dict(stride=1, stats_bytes=2 * 96 * 8), EINVAL, "stats of"),   # 6x7 at stride 1 is two tiles
    (dict(packed=0x30000004), EINVAL, "packed is not 16-byte aligned"),
    (dict(B=0), EINVAL, "B, H, W"),
    (dict(H=0), EINVAL, "B, H, W"),
    (dict(W=-3), EINVAL, "B, H, W"),
    (dict(out=0x10000000), EINVAL, "overlap"),
    (dict(out=0x10000000 + 4 * (2 * 64 * 42 - 1)), EINVAL, "overlap"),
    (dict(out=0x10000000 - 4 * (2 * 96 * 12 - 1)), EINVAL, "overlap"),
])
def test_pw_validation(lib, change, code, msg):
    a = dict(_PW, **change)
    assert lib.corr_enc_pw_forward(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


@pytest.mark.parametrize("change,msg", [
    (dict(y=None), "y is NULL"), (dict(scale=None), "scale is NULL"), (dict(shift=None), "shift is NULL"),
    (dict(skip=None), "skip is NULL"), (dict(out=None), "out is NULL"),
    (dict(kscale=None), "skip_scale and skip_shift"), (dict(kshift=None), "skip_scale and skip_shift"),
    (dict(nb=2), "0 or 1"), (dict(knb=-1), "0 or 1"), (dict(krelu=2), "0 or 1"),
    (dict(B=0), "B, C, H, W"), (dict(C=0), "B, C, H, W"), (dict(H=0), "B, C, H, W"), (dict(W=0), "B, C, H, W"),
])
def test_join_affine_validation(lib, change, msg):
    a = dict(_JOIN, **change)
    assert lib.corr_enc_join_affine(*a.values()) == EINVAL
    assert msg in lib.corr_last_error().decode()


def test_pack_validation(lib):
    for fn, cin in ((lib.corr_enc_stem_pack_weights, 15), (lib.corr_enc_pw_pack_weights, 64)):
        assert fn(None, 64, cin, 0x30000000, None) == EINVAL and "w is NULL" in lib.corr_last_error().decode()
        assert fn(16, 64, cin, None, None) == EINVAL and "packed is NULL" in lib.corr_last_error().decode()
        assert fn(16, 64, cin, 0x30000008, None) == EINVAL and "aligned" in lib.corr_last_error().decode()
        assert fn(16, 0, cin, 0x30000000, None) == EUNSUPPORTED
    assert lib.corr_enc_stem_pack_weights(16, 64, 17, 0x30000000, None) == EUNSUPPORTED
    assert lib.corr_enc_stem_pack_weights(16, 64, 0, 0x30000000, None) == EINVAL
    assert lib.corr_enc_pw_pack_weights(16, 64, 48, 0x30000000, None) == EUNSUPPORTED


def test_validation_accepts_what_it_should(lib):
    """No statistics, no bias, the channel bounds themselves, and buffers that touch without sharing
    a byte are fine: the refusal below comes from the last check (the pack's alignment, the join's
    flags), not from these."""
    for good, fn, touch in ((_STEM, lib.corr_enc_stem_forward, 4 * 2 * 15 * 42), (_PW, lib.corr_enc_pw_forward, 4 * 2 * 64 * 42)):
        changes = [dict(stats=None, stats_bytes=0), dict(bias=None), dict(out=0x10000000 + touch), dict(cout=1),
                   dict(cout=1024, stats=None)]
        changes += [dict(cin=1), dict(cin=16)] if good is _STEM else [dict(cin=32), dict(cin=1024), dict(stride=1, stats=None)]
        for change in changes:
            a = dict(good, packed=0x30000008, **change)
            assert fn(*a.values()) == EINVAL and "aligned" in lib.corr_last_error().decode(), change
    for change in (dict(kscale=None, kshift=None), dict(nb=0), dict(knb=1), dict(out=16), dict(out=64)):
        a = dict(_JOIN, **change)
        a["krelu"] = 7
        assert lib.corr_enc_join_affine(*a.values()) == EINVAL and "0 or 1" in lib.corr_last_error().decode(), change


def test_python_layer_refuses_cpu_tensors():
    from eraft_amd import _lib
    z = torch.zeros
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_stem_pack_weights(z(64, 15, 7, 7))
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_pw_pack_weights(z(96, 64, 1, 1))
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_stem_forward(z(1, 15, 8, 8), z(16), None, 64)
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_pw_forward(z(1, 64, 4, 4), z(16), None, 96, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_join_affine(z(1, 32, 4, 4), z(32), z(32), z(1, 32, 4, 4), z(32), z(32), True)


@pytest.mark.parametrize("norm", NORMS)
def test_module_switch_is_inert_on_cpu(monkeypatch, norm):
    from eraft_amd import encoder
    from eraft_amd.model import BasicEncoder
    assert all(k in encoder.USE_KERNEL and isinstance(encoder.USE_KERNEL[k], bool) for k in NEW_KEYS)
    _all_keys(monkeypatch)
    seed, B, C, H, W = GOLDEN_CASES[1]
    m, x = _encoder(norm, C), encoder_input(seed, B, C, H, W)
    monkeypatch.setattr(BasicEncoder, "fused", False, raising=False)
    a = _run(m, x, "cpu")
    monkeypatch.setattr(BasicEncoder, "fused", True, raising=False)
    assert bit_equal(a, _run(m, x, "cpu"))


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
STEM_CASES = [((1, 1, 1, 1), 64),      # one pixel: only the centre tap is inside the map
              ((1, 15, 2, 2), 64),     # below the kernel extent
              ((1, 5, 7, 40), 64),     # two column tiles
              ((2, 15, 13, 19), 64),   # odd sizes, B > 1, two row tiles
              ((1, 16, 9, 70), 64),    # three column tiles, the last partial; no padding channel
              ((2, 3, 34, 50), 64),    # the golden's second input
              ((1, 15, 3, 33), 1)]     # one output row of the pack


@pytest.mark.gpu
@pytest.mark.parametrize("shape,cout", STEM_CASES)
def test_stem_parity(shape, cout):
    """Inputs of positive mean: a wrong padding shows at every border."""
    B, cin, H, W = shape
    seed = 111
    w, bias = _weights("stem", cin, cout)
    x = _input(seed, B, cin, H, W, 0.5)
    ref = _ref64("stem", seed, B, H, W, cin, cout, 2, 0.5)
    got = _stem(x, w, bias).cpu().numpy()
    e_torch = norm_rel(F.conv2d(_gpu(x), _gpu(w), _gpu(bias), stride=2, padding=3).cpu().numpy(), ref)
    assert got.shape == (B, cout, (H - 1) // 2 + 1, (W - 1) // 2 + 1) and np.isfinite(got).all()
    e = norm_rel(got, ref)
    print(f"enc stem B={B} cin={cin} {H}x{W} cout={cout}: fused {e:.2e}, torch fp32 {e_torch:.2e}")
    assert e <= REL_TOL


PW_SHAPES = [(1, 1, 1), (2, 7, 9), (1, 5, 35), (1, 13, 5), (1, 8, 32)]
PW_CHANNELS = [(64, 96), (96, 128), (128, 256), (32, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("chan", PW_CHANNELS)
@pytest.mark.parametrize("shape", PW_SHAPES)
def test_pw_parity(shape, chan, stride):
    (B, H, W), (cin, cout) = shape, chan
    seed = 113
    w, bias = _weights("pw", cin, cout)
    x = _input(seed, B, cin, H, W)
    ref = _ref64("pw", seed, B, H, W, cin, cout, stride, 0.0)
    got = _pw(x, w, bias, stride).cpu().numpy()
    e_torch = norm_rel(F.conv2d(_gpu(x), _gpu(w), _gpu(bias), stride=stride).cpu().numpy(), ref)
    assert got.shape == (B, cout, (H - 1) // stride + 1, (W - 1) // stride + 1) and np.isfinite(got).all()
    e = norm_rel(got, ref)
    print(f"enc pw B={B} {H}x{W} cin={cin} cout={cout} stride={stride}: fused {e:.2e}, torch fp32 {e_torch:.2e}")
    assert e <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 8, 32), (1, 5, 35)])
def test_pw_stride2_reads_even_positions_only(shape):
    """Every odd row and column at 1e30 or at 0: the same bits, in the output and the statistics."""
    B, H, W = shape
    w, bias = _weights("pw", 64, 96)
    x0 = _input(115, B, 64, H, W).copy()
    x0[:, :, 1::2, :] = 0.0
    x0[:, :, :, 1::2] = 0.0
    x1 = x0.copy()
    x1[:, :, 1::2, :] = 1e30
    x1[:, :, :, 1::2] = 1e30
    (a, sa), (b, sb) = _pw(x0, w, bias, 2, stats=True), _pw(x1, w, bias, 2, stats=True)
    assert np.isfinite(a.cpu().numpy()).all()
    assert bit_equal(a.cpu().numpy(), b.cpu().numpy()) and bit_equal(sa.cpu().numpy(), sb.cpu().numpy())


def _normalised(y, scale, shift):
    """(y * scale + shift in fp32 numpy, the fp64 instance norm of that same y)."""
    a = y * scale[:, :, None, None] + shift[:, :, None, None]
    assert a.dtype == np.float32
    y64 = y.astype(np.float64)
    mean, var = y64.mean((2, 3), keepdims=True), y64.var((2, 3), keepdims=True)
    return a, (y64 - mean) / np.sqrt(var + EPS)


def _with_stats(kind, seed, B, H, W, bias300=False, zero_bias=False):
    """(y, stats, cout) of the stem on a [B, 15, 2H - 1, 2W] input or the pointwise kernel (64 ->
    96, stride 2) on a [B, 64, 2H, 2W - 1] one: an H x W output either way."""
    cin, cout = (15, 64) if kind == "stem" else (64, 96)
    w, bias = _weights(kind, cin, cout)
    if bias300:
        bias = np.full_like(bias, 300.0)
    if zero_bias:
        bias = np.zeros_like(bias)
    if kind == "stem":
        y, st = _stem(_input(seed, B, cin, 2 * H - 1, 2 * W, 0.5), w, bias, stats=True)
    else:
        y, st = _pw(_input(seed, B, cin, 2 * H, 2 * W - 1), w, bias, 2, stats=True)
    assert y.shape == (B, cout, H, W)
    return y, st, cout


@pytest.mark.gpu
@pytest.mark.parametrize("bias300", [False, True])
@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 5, 35), (1, 13, 5)])
@pytest.mark.parametrize("kind", ["stem", "pw"])
def test_statistics(kind, shape, bias300):
    """test_encoder.test_statistics for the two new producers, with its bound: the per-tile (sum,
    M2) pairs and their fp64 merge give the instance norm of the kernel's own output, also with
    every bias at 300, where the mean dwarfs the deviations."""
    from eraft_amd import _lib
    B, H, W = shape
    y, st, cout = _with_stats(kind, 117, B, H, W, bias300)
    scale, shift = _lib.enc_norm_finalize(st, B, cout, H, W, EPS)
    assert scale.shape == shift.shape == (B, cout)
    a, b = _normalised(y.cpu().numpy(), scale.cpu().numpy(), shift.cpu().numpy())
    e = norm_rel(a, b)
    print(f"enc {kind} statistics B={B} {H}x{W} bias300={int(bias300)}: {e:.2e}")
    assert e <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["stem", "pw"])
def test_statistics_of_a_single_pixel(kind):
    """Ho * Wo = 1: the tile's sum is the pixel and its M2 exactly 0, so scale = 1 / sqrt(eps), and
    y * scale + shift is 0 up to rounding (test_encoder's bound: |y| <= 4 times 316 at a few fp32
    ulp is about 3e-4)."""
    from eraft_amd import _lib
    y, st, cout = _with_stats(kind, 119, 2, 1, 1, zero_bias=True)
    yb, sb = y.cpu().numpy(), st.cpu().numpy().reshape(2, cout, 1, 2)
    assert bit_equal(sb[..., 0], yb.reshape(2, cout, 1)) and (sb[..., 1] == 0.0).all()
    scale, shift = _lib.enc_norm_finalize(st, 2, cout, 1, 1, EPS)
    assert np.allclose(scale.cpu().numpy(), 1.0 / np.sqrt(np.float64(np.float32(EPS))), rtol=1e-6)
    a, _ = _normalised(yb, scale.cpu().numpy(), shift.cpu().numpy())
    print(f"enc {kind} statistics, one pixel: max |y| {np.abs(yb).max():.2f}, max |normalised| {np.abs(a).max():.2e}")
    assert np.abs(yb).max() <= 4.0 and np.abs(a).max() <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("skip_relu", [False, True])
@pytest.mark.parametrize("skip_per_batch", [True, False])
@pytest.mark.parametrize("per_batch", [True, False])
def test_join_affine(per_batch, skip_per_batch, skip_relu, alias):
    from eraft_amd import _lib
    B, C, H, W = 2, 96, 7, 9
    y, skip = _input(121, B, C, H, W), _input(122, B, C, H, W)
    scale, shift = _affine_pair(121, B, C, per_batch)
    ksc, ksh = _affine_pair(125, B, C, skip_per_batch)
    f64 = lambda a: a.astype(np.float64)
    s = f64(skip) * _bcast(f64(ksc), B, C) + _bcast(f64(ksh), B, C)
    if skip_relu:
        s = np.maximum(s, 0.0)
    ref = np.maximum(s + np.maximum(f64(y) * _bcast(f64(scale), B, C) + _bcast(f64(shift), B, C), 0.0), 0.0)
    yg = _gpu(y)
    out = _lib.enc_join_affine(yg, _gpu(scale), _gpu(shift), _gpu(skip), _gpu(ksc), _gpu(ksh), skip_relu,
                               out=yg if alias else None)
    assert (out is yg) == alias
    if not alias:
        assert bit_equal(yg.cpu().numpy(), y)
    e = norm_rel(out.cpu().numpy(), ref)
    print(f"enc join_affine per_batch={per_batch} skip_per_batch={skip_per_batch} skip_relu={skip_relu} "
          f"alias={alias}: {e:.2e}")
    assert e <= REL_TOL and (ref > 0).any() and (ref == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("identity", ["ones", "none"])
def test_join_affine_with_an_identity_skip_is_enc_join(identity):
    from eraft_amd import _lib
    B, C, H, W = 2, 96, 7, 9
    y, skip = _gpu(_input(121, B, C, H, W)), _gpu(np.abs(_input(122, B, C, H, W)))
    scale, shift = (_gpu(a) for a in _affine_pair(121, B, C, True))
    one, zero = (torch.ones(C, device=DEV), torch.zeros(C, device=DEV)) if identity == "ones" else (None, None)
    a = _lib.enc_join_affine(y, scale, shift, skip, one, zero, False)
    assert bit_equal(a.cpu().numpy(), _lib.enc_join(y, scale, shift, skip).cpu().numpy())


@pytest.mark.gpu
def test_deterministic_and_capturable():
    from eraft_amd import _lib
    B, cin, H, W = 2, 15, 25, 41   # -> 13 x 21
    w0, b0 = _weights("stem", cin, 64)
    w1, b1 = prng.param_init("front_3x3.weight", (64, 64, 3, 3)), prng.param_init("front_3x3.bias", (64,))
    w2, b2 = _weights("pw", 64, 96)
    xg = _gpu(_input(127, B, cin, H, W, 0.5))
    b0g, b1g, b2g = _gpu(b0), _gpu(b1), _gpu(b2)
    p0, p1, p2 = _lib.enc_stem_pack_weights(_gpu(w0)), _lib.conv_pack_weights(_gpu(w1)), _lib.enc_pw_pack_weights(_gpu(w2))

    def chain():
        y0, st0 = _lib.enc_stem_forward(xg, p0, b0g, 64, stats=True)
        sc0, sh0 = _lib.enc_norm_finalize(st0, B, 64, 13, 21, EPS)
        y1, st1 = _lib.enc_conv_forward(y0, p1, b1g, 64, 1, sc0, sh0, stats=True)
        sc1, sh1 = _lib.enc_norm_finalize(st1, B, 64, 13, 21, EPS)
        x1 = _lib.enc_join_affine(y1, sc1, sh1, y0, sc0, sh0, True)
        p, stp = _lib.enc_pw_forward(x1, p2, b2g, 96, 2, stats=True)
        return x1, sc0, sh0, p, stp

    a, b = chain(), chain()
    for u, v in zip(a, b):
        assert bit_equal(u.cpu().numpy(), v.cpu().numpy())
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        c = chain()
    gph.replay()
    torch.cuda.synchronize()
    for u, v in zip(a, c):
        assert bit_equal(u.cpu().numpy(), v.cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["stem", "pw1", "pw2"])
def test_buffer_discipline(kind):
    """Guard words around out, the statistics and the pack stay as they were, every word between
    them is written, and the input is unchanged.  The stem's input has exactly cin = 15 planes and
    ends where its allocation ends: a 16th channel does not exist."""
    from eraft_amd import _lib
    lib = _lib.load()
    stem = kind == "stem"
    stride = 2 if kind != "pw1" else 1
    B, H, W = 2, 13, 19
    cin, cout = (15, 64) if stem else (64, 96)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    w, bias = _weights("stem" if stem else "pw", cin, cout)
    sentinel, guard = 0x7FC12345, 4096   # a NaN pattern: no finite result has these bits
    x = _input(129, B, cin, H, W, 0.5)
    n_in = x.size
    xbuf = torch.full((guard + n_in,), float("nan"), dtype=torch.float32, device=DEV)
    xin = xbuf[guard:]
    xin.copy_(torch.from_numpy(x.reshape(-1)))
    wg, bg = _gpu(w), _gpu(bias)
    n_pk = (lib.corr_enc_stem_weights_bytes if stem else lib.corr_enc_pw_weights_bytes)(cout, cin) // 4
    n_out, n_st = B * cout * Ho * Wo, lib.corr_enc_stats_bytes(B, cout, Ho, Wo) // 4
    full = lambda n: torch.full((guard + n + guard,), sentinel, dtype=torch.int32, device=DEV)
    pk, out, st = full(n_pk), full(n_out), full(n_st)
    at = lambda t: t.data_ptr() + 4 * guard
    stream = torch.cuda.current_stream().cuda_stream
    rc = (lib.corr_enc_stem_pack_weights if stem else lib.corr_enc_pw_pack_weights)(wg.data_ptr(), cout, cin, at(pk), stream)
    assert rc == OK, lib.corr_last_error().decode()
    torch.cuda.synchronize()
    pk0 = pk.cpu().numpy().copy()
    if stem:
        rc = lib.corr_enc_stem_forward(xin.data_ptr(), cin, B, H, W, at(pk), bg.data_ptr(), cout, at(out), at(st),
                                       n_st * 4, stream)
    else:
        rc = lib.corr_enc_pw_forward(xin.data_ptr(), cin, B, H, W, stride, at(pk), bg.data_ptr(), cout, at(out), at(st),
                                     n_st * 4, stream)
    assert rc == OK, lib.corr_last_error().decode()
    torch.cuda.synchronize()
    for name, t, n in (("pack", pk, n_pk), ("out", out, n_out), ("stats", st, n_st)):
        v = t.cpu().numpy()
        assert (v[:guard] == sentinel).all() and (v[guard + n:] == sentinel).all(), name
        assert (v[guard:guard + n] != sentinel).all(), name
    assert np.array_equal(pk.cpu().numpy(), pk0)
    assert bit_equal(xin.cpu().numpy(), x.reshape(-1)) and bit_equal(wg.cpu().numpy(), w)
    ref = _ref64("stem" if stem else "pw", 129, B, H, W, cin, cout, stride, 0.5)
    got = out.cpu().numpy()[guard:guard + n_out].view(np.float32).reshape(ref.shape)
    assert norm_rel(got, ref) <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_module_leaves_no_torch_op(monkeypatch, norm):
    """With every piece on its kernel, BasicEncoder.forward calls no torch convolution and no torch
    norm (and so stores no normalised map)."""
    from eraft_amd.model import BasicEncoder
    seed, B, C, H, W = GOLDEN_CASES[1]
    m, x = _encoder(norm, C, DEV), encoder_input(seed, B, C, H, W)
    monkeypatch.setattr(BasicEncoder, "fused", False)
    plain = _run(m, x)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    _all_keys(monkeypatch)

    def never(self, *a, **k):
        raise AssertionError(f"{type(self).__name__}.forward ran under the switch")
    for cls in (nn.Conv2d, nn.InstanceNorm2d, nn.BatchNorm2d):
        monkeypatch.setattr(cls, "forward", never)
    fused = _run(m, x)
    assert fused.shape == plain.shape and norm_rel(fused, plain) <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_module_matches_reference_golden(monkeypatch, norm):
    from eraft_amd.model import BasicEncoder
    _all_keys(monkeypatch)
    g = load("encoder_reference")
    for k, (seed, B, C, H, W) in enumerate(GOLDEN_CASES):
        m, x = _encoder(norm, C, DEV), encoder_input(seed, B, C, H, W)
        monkeypatch.setattr(BasicEncoder, "fused", False)
        plain = _run(m, x)
        monkeypatch.setattr(BasicEncoder, "fused", True)
        fused = _run(m, x)
        e, e_plain, e_sw = norm_rel(fused, g[f"{norm}{k}"]), norm_rel(plain, g[f"{norm}{k}"]), norm_rel(fused, plain)
        print(f"encoder front golden {norm} B={B} C={C} {H}x{W}: fused {e:.2e}, torch fp32 {e_plain:.2e}, "
              f"fused against torch {e_sw:.2e}")
        assert e <= REL_TOL and e_sw <= REL_TOL, (norm, k)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_each_piece_falls_back_to_torch(monkeypatch, norm):
    from eraft_amd import encoder
    from eraft_amd.model import BasicEncoder
    monkeypatch.setattr(BasicEncoder, "fused", True)
    _all_keys(monkeypatch)
    seed, B, C, H, W = GOLDEN_CASES[1]
    m, x = _encoder(norm, C, DEV), encoder_input(seed, B, C, H, W)
    full = _run(m, x)
    for key in NEW_KEYS:
        monkeypatch.setitem(encoder.USE_KERNEL, key, False)
        e = norm_rel(_run(m, x), full)
        monkeypatch.setitem(encoder.USE_KERNEL, key, True)
        print(f"encoder front {norm}: {key} on torch against all kernels {e:.2e}")
        assert e <= REL_TOL, key


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_stem_wider_than_the_kernel_runs_on_torch(monkeypatch, norm):
    """n_first_channels = 20 is beyond corr_enc_stem_forward (cin <= 16): the stem alone runs on
    torch, the rest on the kernels."""
    from eraft_amd import _lib, encoder
    from eraft_amd.model import BasicEncoder
    _all_keys(monkeypatch)
    assert _lib.load().corr_enc_stem_weights_bytes(64, 20) == 0 and encoder.STEM_MAX_CIN == 16
    m, x = _encoder(norm, 20, DEV), encoder_input(131, 1, 20, 32, 40)
    monkeypatch.setattr(BasicEncoder, "fused", False)
    plain = _run(m, x)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    with torch.no_grad():
        assert m._fusable(torch.from_numpy(x).to(DEV))
    fused = _run(m, x)
    e = norm_rel(fused, plain)
    print(f"encoder front {norm}, 20 input channels: fused against torch {e:.2e}")
    assert not bit_equal(plain, fused) and e <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("others", [False, True])
def test_e2e_matches_reference(monkeypatch, others):
    """The g_e2e_dsec golden, cold and warm start, with the whole encoders on the kernels; once
    alone and once with the fused GRU, update block and mask head as well."""
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    from test_e2e import EPE_TOL, _epe, _model
    _all_keys(monkeypatch)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    monkeypatch.setattr(BasicUpdateBlock, "fused", others)
    monkeypatch.setattr(SepConvGRU, "fused", others)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", others)
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
    print(f"e2e encoder front (other three switches={others}): cold low/up {errs[0]:.2e}/{errs[1]:.2e}, "
          f"warm low/up {errs[2]:.2e}/{errs[3]:.2e} px")
    assert all(e <= EPE_TOL for e in errs)
