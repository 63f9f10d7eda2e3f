"""The encoders' residual stages on the 3x3 kernel (corr_enc_*, csrc/corr_conv.hip) and the module
built on them (eraft_amd/encoder.py, BasicEncoder.fused).

CPU: the exports, the size function and the argument validation (all before any HIP call), that
the module switch is inert on CPU tensors, and that the repository's BasicEncoder agrees with the
reference's own (tests/golden/encoder_reference.npz, make_golden_encoder.py).  GPU: parity of
enc_conv_forward (stride 1 and 2, norm on load off / per batch item / per channel) with an fp64
CPU F.conv2d of the same formula within REL_TOL (norm-relative), the statistics and their merge,
the join, determinism, graph capture, buffer discipline, the module switch, the reference's
BasicEncoder and the end-to-end golden.

Measured on an MI355X (norm_rel against fp64; torch's own fp32 GPU result beside it): see
DESIGN.md §16.
"""
import copy
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import prng
from _util import REL_TOL, bit_equal, load, norm_rel
from make_golden_encoder import CASES as GOLDEN_CASES, NORMS, OUTPUT_DIM, encoder_input, fill

OK, EINVAL, EUNSUPPORTED = 0, -1, -2
NAMES = ("corr_enc_stats_bytes", "corr_enc_conv_forward", "corr_enc_norm_finalize", "corr_enc_join")
DEV = "cuda:0"
EPS = 1e-5


# ----------------------------------------------------------------------------------------------
# shared data (read-only by convention)
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(cin, cout):
    return prng.param_init(f"enc_{cin}_{cout}.weight", (cout, cin, 3, 3)), prng.param_init(f"enc_{cin}_{cout}.bias", (cout,))


@functools.lru_cache(maxsize=None)
def _input(seed, B, C, H, W):
    return prng.gauss(seed, (B, C, H, W))


@functools.lru_cache(maxsize=None)
def _norm(seed, B, C, per_batch):
    """(scale, shift) for the norm on load: any-sign scales, shifts of positive mean (so that the
    normalised value of a padded zero, relu(shift), is not zero)."""
    shape = (B, C) if per_batch else (C,)
    return ((1.0 + 0.5 * prng.gauss(seed + 1, shape)).astype(np.float32),
            (0.5 + np.abs(prng.gauss(seed + 2, shape))).astype(np.float32))


def _apply64(x, scale, shift):
    """relu(x * scale + shift) in fp64; scale, shift [B, C] or [C]."""
    v = scale.shape + (1, 1) if scale.ndim == 2 else (1,) + scale.shape + (1, 1)
    return np.maximum(x.astype(np.float64) * scale.astype(np.float64).reshape(v) + shift.astype(np.float64).reshape(v), 0.0)


@functools.lru_cache(maxsize=None)
def _ref64(seed, B, H, W, cin, cout, stride, norm):
    w, bias = _weights(cin, cout)
    x = _input(seed, B, cin, H, W).astype(np.float64)
    if norm != "off":
        x = _apply64(_input(seed, B, cin, H, W), *_norm(seed, B, cin, norm == "batch"))
    return F.conv2d(torch.from_numpy(x), torch.from_numpy(w).double(), torch.from_numpy(bias).double(),
                    stride=stride, padding=1).numpy()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _conv(x, w, bias, stride=1, norm=None, stats=False):
    from eraft_amd import _lib
    sc, sh = (None, None) if norm is None else (_gpu(norm[0]), _gpu(norm[1]))
    return _lib.enc_conv_forward(_gpu(x), _lib.conv_pack_weights(_gpu(w)), _gpu(bias), w.shape[0], stride, sc, sh, stats)


def _encoder(norm, C, dev="cpu"):
    from eraft_amd.model import BasicEncoder
    return fill(BasicEncoder(output_dim=OUTPUT_DIM, norm_fn=norm, n_first_channels=C).eval()).to(dev)


def _run(m, x, dev=DEV, dtype=torch.float32):
    with torch.no_grad():
        return m(torch.from_numpy(x).to(device=dev, dtype=dtype)).cpu().numpy()


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


def test_abi_version_is_unchanged(lib):
    assert lib.corr_version() == 202


def test_stats_bytes(lib):
    for B, cout, Ho, Wo in ((2, 96, 7, 9), (1, 64, 240, 320), (1, 128, 5, 35), (3, 1, 1, 1), (1, 96, 4, 16), (1, 96, 5, 17)):
        assert lib.corr_enc_stats_bytes(B, cout, Ho, Wo) >= B * cout * ((Ho + 3) // 4) * ((Wo + 15) // 16) * 8
    for bad in ((0, 96, 7, 9), (2, 0, 7, 9), (2, 96, 0, 9), (2, 96, 7, -1)):
        assert lib.corr_enc_stats_bytes(*bad) == 0, bad


# corr_enc_conv_forward(in, cin, B, H, W, stride, in_scale, in_shift, norm_per_batch, packed, bias, cout, out,
#                       stats, stats_bytes, stream)
# (fake pointers, far enough apart that no buffer of these sizes overlaps another)
_GOOD = dict(inp=0x10000000, cin=64, B=2, H=6, W=7, stride=2, in_scale=0x20000000, in_shift=0x21000000,
             norm_per_batch=1, packed=0x30000000, bias=0x40000000, cout=96, out=0x50000000, stats=0x60000000,
             stats_bytes=2 * 96 * 1 * 1 * 8, stream=None)


@pytest.mark.parametrize("change,code,msg", [
    (dict(stride=0), EUNSUPPORTED, "stride"),
    (dict(stride=3), EUNSUPPORTED, "stride"),
    (dict(cin=0), EUNSUPPORTED, "ca >= 32"),
    (dict(cin=48), EUNSUPPORTED, "multiples of 32"),
    (dict(cin=1056), EUNSUPPORTED, "<= 1024"),
    (dict(cout=0), EUNSUPPORTED, "1 <= cout"),
    (dict(cout=1025), EUNSUPPORTED, "cout <= 1024"),
    (dict(inp=None), EINVAL, "in is NULL"),
    (dict(packed=None), EINVAL, "packed is NULL"),
    (dict(out=None), EINVAL, "out is NULL"),
    (dict(in_scale=None), EINVAL, "in_scale and in_shift"),
    (dict(in_shift=None), EINVAL, "in_scale and in_shift"),
    (dict(stats_bytes=2 * 96 * 8 - 1), EINVAL, "stats of"),
    (dict(stride=1, stats_bytes=2 * 96 * 8), EINVAL, "stats of"),   # 6x7 at stride 1 is two tiles
    (dict(packed=0x30000004), EINVAL, "packed is not 16-byte aligned"),
    (dict(B=0), EINVAL, "B, H, W"),
    (dict(H=0), EINVAL, "B, H, W"),
    (dict(W=-3), EINVAL, "B, H, W"),
    (dict(out=0x10000000), EINVAL, "overlap"),
    (dict(out=0x10000000 + 4 * (2 * 64 * 42 - 1)), EINVAL, "overlap"),   # the last float of in
    (dict(out=0x10000000 - 4 * (2 * 96 * 12 - 1)), EINVAL, "overlap"),   # out's last float is in's first
])
def test_conv_validation(lib, change, code, msg):
    """Every refusal comes before any HIP call (the pointers are never dereferenced)."""
    a = dict(_GOOD, **change)
    assert lib.corr_enc_conv_forward(*a.values()) == code
    assert msg in lib.corr_last_error().decode()


def test_conv_validation_accepts_what_it_should(lib):
    """No norm (both NULL), no statistics, and buffers that touch without sharing a byte are fine:
    the refusals below come from a later check, not from these."""
    for change in (dict(in_scale=None, in_shift=None), dict(stats=None, stats_bytes=0),
                   dict(out=0x10000000 + 4 * 2 * 64 * 42), dict(bias=None)):
        a = dict(_GOOD, packed=0x30000008, **change)
        assert lib.corr_enc_conv_forward(*a.values()) == EINVAL and "aligned" in lib.corr_last_error().decode()


def test_finalize_and_join_validation(lib):
    f32 = ctypes.c_float
    assert lib.corr_enc_norm_finalize(None, 2, 96, 3, 4, f32(EPS), 16, 32, None) == EINVAL
    assert "stats is NULL" in lib.corr_last_error().decode()
    assert lib.corr_enc_norm_finalize(16, 2, 96, 3, 4, f32(EPS), None, 32, None) == EINVAL
    assert lib.corr_enc_norm_finalize(16, 2, 96, 3, 4, f32(EPS), 16, None, None) == EINVAL
    assert lib.corr_enc_norm_finalize(16, 2, 96, 3, 4, f32(0.0), 16, 32, None) == EINVAL
    assert "eps" in lib.corr_last_error().decode()
    for bad in ((0, 96, 3, 4), (2, 0, 3, 4), (2, 96, 0, 4), (2, 96, 3, 0)):
        assert lib.corr_enc_norm_finalize(16, *bad, f32(EPS), 16, 32, None) == EINVAL, bad
        assert lib.corr_enc_join(16, 32, 48, 1, 64, *bad, 80, None) == EINVAL, bad
    good = [16, 32, 48, 1, 64, 2, 96, 3, 4, 80, None]
    for k, nm in ((0, "y"), (1, "scale"), (2, "shift"), (4, "skip"), (9, "out")):
        a = list(good)
        a[k] = None
        assert lib.corr_enc_join(*a) == EINVAL
        assert f"{nm} is NULL" in lib.corr_last_error().decode()


def test_python_layer_refuses_cpu_tensors():
    from eraft_amd import _lib
    from eraft_amd.encoder import encoder_forward
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_conv_forward(torch.zeros(1, 32, 4, 4), torch.zeros(16), None, 1)
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_norm_finalize(torch.zeros(64), 1, 32, 2, 2)
    with pytest.raises(RuntimeError, match="MI355X"):
        _lib.enc_join(torch.zeros(1, 32, 4, 4), torch.zeros(32), torch.zeros(32), torch.zeros(1, 32, 4, 4))
    with pytest.raises(RuntimeError, match="MI355X"):
        encoder_forward(_encoder("instance", 3), torch.zeros(1, 3, 16, 16))


def test_switch_follows_the_environment_and_defaults_to_off():
    import os
    from eraft_amd.model import BasicEncoder
    assert BasicEncoder.fused is (os.environ.get("ERAFT_AMD_FUSE_ENCODER", "0") == "1")


@pytest.mark.parametrize("norm", NORMS)
def test_module_switch_is_inert_on_cpu(monkeypatch, norm):
    from eraft_amd.model import BasicEncoder
    seed, B, C, H, W = GOLDEN_CASES[1]
    m, x = _encoder(norm, C), encoder_input(seed, B, C, H, W)
    monkeypatch.setattr(BasicEncoder, "fused", False, raising=False)
    a = _run(m, x, "cpu")
    monkeypatch.setattr(BasicEncoder, "fused", True, raising=False)
    assert bit_equal(a, _run(m, x, "cpu"))


@pytest.mark.parametrize("norm", NORMS)
def test_cpu_encoder_matches_reference_golden(norm):
    """The restated module and the fixture agree before any GPU test leans on either."""
    g = load("encoder_reference")
    assert g["cases"].tolist() == [list(c) for c in GOLDEN_CASES]
    for k, (seed, B, C, H, W) in enumerate(GOLDEN_CASES):
        out = _run(_encoder(norm, C), encoder_input(seed, B, C, H, W), "cpu")
        assert out.shape == g[f"{norm}{k}"].shape == (B, OUTPUT_DIM, (H + 7) // 8, (W + 7) // 8)
        assert norm_rel(out, g[f"{norm}{k}"]) <= REL_TOL, (norm, k)


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
SHAPES = [(1, 1, 1),    # only the centre tap is inside the map
          (1, 2, 2),    # one output pixel at stride 2
          (1, 3, 4),    # the halo covers the whole map
          (2, 7, 9),    # odd sizes, partial tiles, B > 1
          (1, 5, 35),   # more than two tiles along W (stride 2: two)
          (1, 13, 5),   # more than two tiles along H (stride 2: two)
          (1, 8, 32)]   # whole tiles only
CHANNELS = [(64, 64), (64, 96), (96, 96),   # 96 rows: the pack pads them to 128
            (96, 128), (128, 128), (32, 1)]
CASES = [(s, (64, 96)) for s in SHAPES] + [((2, 7, 9), c) for c in CHANNELS if c != (64, 96)]


@pytest.mark.gpu
@pytest.mark.parametrize("norm", ["off", "batch", "channel"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape,chan", CASES)
def test_conv_parity(shape, chan, stride, norm):
    (B, H, W), (cin, cout) = shape, chan
    seed = 91
    w, bias = _weights(cin, cout)
    x = _input(seed, B, cin, H, W)
    nrm = None if norm == "off" else _norm(seed, B, cin, norm == "batch")
    ref = _ref64(seed, B, H, W, cin, cout, stride, norm)
    got = _conv(x, w, bias, stride, nrm).cpu().numpy()
    xt = _gpu(x)
    if nrm is not None:
        v = (B, cin, 1, 1) if norm == "batch" else (1, cin, 1, 1)
        xt = F.relu(xt * _gpu(nrm[0]).view(v) + _gpu(nrm[1]).view(v))
    e_torch = norm_rel(F.conv2d(xt, _gpu(w), _gpu(bias), stride=stride, padding=1).cpu().numpy(), ref)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    assert got.shape == (B, cout, Ho, Wo) and np.isfinite(got).all()
    e = norm_rel(got, ref)
    print(f"enc conv B={B} {H}x{W} cin={cin} cout={cout} stride={stride} norm={norm}: fused {e:.2e}, "
          f"torch fp32 {e_torch:.2e}")
    assert e <= REL_TOL


def _normalised(y, scale, shift):
    """(y * scale + shift in fp32 numpy, the fp64 instance norm of that same y)."""
    a = y * scale[:, :, None, None] + shift[:, :, None, None]
    assert a.dtype == np.float32
    y64 = y.astype(np.float64)
    mean, var = y64.mean((2, 3), keepdims=True), y64.var((2, 3), keepdims=True)
    return a, (y64 - mean) / np.sqrt(var + EPS)


@pytest.mark.gpu
@pytest.mark.parametrize("bias300", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(2, 7, 9), (1, 5, 35), (1, 13, 5)])
def test_statistics(shape, stride, bias300):
    """The per-tile (sum, M2) pairs and their fp64 merge give the instance norm of the kernel's own
    output.  With every bias at 300 the mean dwarfs the deviations: a tile-wise (mean, M2) merge
    stays <= 7.3e-6 there, a plain fp32 sum / sum of squares gives >= 6.7e-3 (numpy, n = 12 .. 4800)."""
    from eraft_amd import _lib
    B, H, W = shape
    cin, cout = 64, 96
    w, bias = _weights(cin, cout)
    if bias300:
        bias = np.full_like(bias, 300.0)
    y, st = _conv(_input(93, B, cin, H, W), w, bias, stride, None, stats=True)
    scale, shift = _lib.enc_norm_finalize(st, B, cout, y.shape[2], y.shape[3], EPS)
    assert scale.shape == shift.shape == (B, cout)
    a, b = _normalised(y.cpu().numpy(), scale.cpu().numpy(), shift.cpu().numpy())
    e = norm_rel(a, b)
    print(f"enc statistics B={B} {H}x{W} stride={stride} bias300={int(bias300)}: {e:.2e}")
    assert e <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("shape,stride", [((1, 1, 1), 1), ((2, 2, 2), 2)])
def test_statistics_of_a_single_pixel(shape, stride):
    """Ho * Wo = 1: the variance is 0, scale = 1 / sqrt(eps), and y * scale + shift is 0 up to
    rounding: |y| <= 4 times 316 at a few fp32 ulp is about 3e-4."""
    from eraft_amd import _lib
    B, H, W = shape
    w, bias = _weights(64, 96)
    y, st = _conv(_input(95, B, 64, H, W), w, np.zeros_like(bias), stride, None, stats=True)
    assert y.shape == (B, 96, 1, 1)
    scale, shift = _lib.enc_norm_finalize(st, B, 96, 1, 1, EPS)
    assert np.allclose(scale.cpu().numpy(), 1.0 / np.sqrt(np.float64(np.float32(EPS))), rtol=1e-6)
    a, _ = _normalised(y.cpu().numpy(), scale.cpu().numpy(), shift.cpu().numpy())
    print(f"enc statistics, one pixel: max |y| {np.abs(y.cpu().numpy()).max():.2f}, max |normalised| {np.abs(a).max():.2e}")
    assert np.abs(a).max() <= 1e-3


@pytest.mark.gpu
@pytest.mark.parametrize("alias", [False, True])
@pytest.mark.parametrize("per_batch", [True, False])
def test_join(per_batch, alias):
    from eraft_amd import _lib
    B, C, H, W = 2, 96, 7, 9
    y, skip = _input(97, B, C, H, W), _input(98, B, C, H, W)
    scale, shift = _norm(97, B, C, per_batch)
    ref = np.maximum(skip.astype(np.float64) + _apply64(y, scale, shift), 0.0)
    yg = _gpu(y)
    out = _lib.enc_join(yg, _gpu(scale), _gpu(shift), _gpu(skip), out=yg if alias else None)
    assert (out is yg) == alias
    if not alias:
        assert bit_equal(yg.cpu().numpy(), y)
    e = norm_rel(out.cpu().numpy(), ref)
    print(f"enc join per_batch={per_batch} alias={alias}: {e:.2e}")
    assert e <= REL_TOL and (ref > 0).any() and (ref == 0).any()


@pytest.mark.gpu
def test_deterministic_and_capturable():
    from eraft_amd import _lib
    B, H, W, cin, cout = 2, 13, 21, 64, 96
    w, bias = _weights(cin, cout)
    xg, bg, skip = _gpu(_input(99, B, cin, H, W)), _gpu(bias), _gpu(_input(100, B, cout, 7, 11))
    packed = _lib.conv_pack_weights(_gpu(w))  # outside the capture

    def chain():
        y, st = _lib.enc_conv_forward(xg, packed, bg, cout, 2, stats=True)
        scale, shift = _lib.enc_norm_finalize(st, B, cout, 7, 11, EPS)
        return _lib.enc_join(y, scale, shift, skip), scale, shift

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
@pytest.mark.parametrize("stride", [1, 2])
def test_buffer_discipline(stride):
    """Every element of out [B][cout][Ho][Wo] is written, nothing after it is, and the statistics
    end at corr_enc_stats_bytes."""
    from eraft_amd import _lib
    lib = _lib.load()
    B, H, W, cin, cout = 2, 7, 9, 64, 96
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    w, bias = _weights(cin, cout)
    xg, bg, packed = _gpu(_input(101, B, cin, H, W)), _gpu(bias), _lib.conv_pack_weights(_gpu(w))
    sc, sh = (_gpu(a) for a in _norm(101, B, cin, True))
    sentinel, guard = 0x7FC12345, 4096   # a NaN pattern: no finite result has these bits
    n_out, n_st = B * cout * Ho * Wo, lib.corr_enc_stats_bytes(B, cout, Ho, Wo) // 4
    out = torch.full((n_out + guard,), sentinel, dtype=torch.int32, device=DEV)
    st = torch.full((n_st + guard,), sentinel, dtype=torch.int32, device=DEV)
    rc = lib.corr_enc_conv_forward(xg.data_ptr(), cin, B, H, W, stride, sc.data_ptr(), sh.data_ptr(), 1,
                                   packed.data_ptr(), bg.data_ptr(), cout, out.data_ptr(), st.data_ptr(), n_st * 4,
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == OK, lib.corr_last_error().decode()
    torch.cuda.synchronize()
    ob, sb = out.cpu().numpy(), st.cpu().numpy()
    assert (ob[:n_out] != sentinel).all() and (ob[n_out:] == sentinel).all()
    assert (sb[:n_st] != sentinel).all() and (sb[n_st:] == sentinel).all()
    ref = _ref64(101, B, H, W, cin, cout, stride, "batch")
    assert norm_rel(ob[:n_out].view(np.float32).reshape(ref.shape), ref) <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_module_matches_reference_golden(monkeypatch, norm):
    from eraft_amd.model import BasicEncoder
    g = load("encoder_reference")
    for k, (seed, B, C, H, W) in enumerate(GOLDEN_CASES):
        m, x = _encoder(norm, C, DEV), encoder_input(seed, B, C, H, W)
        monkeypatch.setattr(BasicEncoder, "fused", False)
        plain = _run(m, x)
        monkeypatch.setattr(BasicEncoder, "fused", True)
        fused = _run(m, x)
        e, e_plain, e_sw = norm_rel(fused, g[f"{norm}{k}"]), norm_rel(plain, g[f"{norm}{k}"]), norm_rel(fused, plain)
        print(f"encoder golden {norm} B={B} C={C} {H}x{W}: fused {e:.2e}, torch fp32 {e_plain:.2e}, "
              f"fused against torch {e_sw:.2e}")
        assert not bit_equal(plain, fused)  # the kernels did run
        assert e <= REL_TOL and e_sw <= REL_TOL, (norm, k)


@pytest.mark.gpu
@pytest.mark.parametrize("norm", NORMS)
def test_module_takes_the_torch_path_when_it_must(monkeypatch, norm):
    """Autograd recording, and a batch norm in train() mode: the code that runs today."""
    import eraft_amd.encoder
    from eraft_amd.model import BasicEncoder
    seed, B, C, H, W = GOLDEN_CASES[1]
    m = _encoder(norm, C, DEV)
    # (MIOpen's deterministic solvers, so that two runs of the same torch code can be compared bit
    # for bit)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    x = torch.from_numpy(encoder_input(seed, B, C, H, W)).to(DEV).requires_grad_(True)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    out_f = m(x)
    monkeypatch.setattr(BasicEncoder, "fused", False)
    out_p = m(x)
    assert out_f.grad_fn is not None
    assert bit_equal(out_f.detach().cpu().numpy(), out_p.detach().cpu().numpy())
    if norm == "batch":
        def never(*a, **k):
            raise AssertionError("a batch norm in train() mode took the kernel path")
        monkeypatch.setattr(eraft_amd.encoder, "encoder_forward", never)
        monkeypatch.setattr(BasicEncoder, "fused", True)
        t = copy.deepcopy(m).train()
        with torch.no_grad():
            assert m._fusable(x.detach()) and not t._fusable(x.detach())
            t(x.detach())


@pytest.mark.gpu
def test_running_statistics_changed_in_place_are_picked_up(monkeypatch):
    from eraft_amd.model import BasicEncoder
    monkeypatch.setattr(BasicEncoder, "fused", True)
    seed, B, C, H, W = GOLDEN_CASES[1]
    m, x = _encoder("batch", C, DEV), encoder_input(seed, B, C, H, W)
    before = _run(m, x)
    with torch.no_grad():
        m.layer2[0].norm1.running_var.mul_(4.0)
        m.layer3[1].norm2.running_mean.add_(0.5)
    after = _run(m, x)
    assert norm_rel(after, before) > 100 * REL_TOL
    assert norm_rel(after, _run(copy.deepcopy(m).cpu().double(), x, "cpu", torch.float64)) <= REL_TOL


@pytest.mark.gpu
def test_pair_input(monkeypatch):
    from eraft_amd.model import BasicEncoder
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    seed, B, C, H, W = GOLDEN_CASES[1]
    m = _encoder("instance", C, DEV)
    x1, x2 = (torch.from_numpy(encoder_input(seed + k, 1, C, H, W)).to(DEV) for k in (0, 1))
    with torch.no_grad():
        monkeypatch.setattr(BasicEncoder, "fused", False)
        p1, p2 = m([x1, x2])
        monkeypatch.setattr(BasicEncoder, "fused", True)
        f = m([x1, x2])
        whole = m(torch.cat([x1, x2]))
    assert isinstance(f, tuple) and len(f) == 2 and f[0].shape == p1.shape and f[1].shape == p2.shape
    assert bit_equal(torch.cat(f).cpu().numpy(), whole.cpu().numpy())
    assert norm_rel(f[0].cpu().numpy(), p1.cpu().numpy()) <= REL_TOL
    assert norm_rel(f[1].cpu().numpy(), p2.cpu().numpy()) <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("others", [False, True])
def test_e2e_with_fused_encoder_matches_reference(monkeypatch, others):
    """The g_e2e_dsec golden, cold and warm start, with the encoders' residual stages on the
    kernels; once alone and once with the fused GRU and update block as well."""
    from eraft_amd.model import BasicEncoder, BasicUpdateBlock, SepConvGRU
    from test_e2e import EPE_TOL, _epe, _model
    monkeypatch.setattr(BasicEncoder, "fused", True)
    monkeypatch.setattr(BasicUpdateBlock, "fused", others)
    monkeypatch.setattr(SepConvGRU, "fused", others)
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
    print(f"e2e fused encoder (fused GRU and update block={others}): cold low/up {errs[0]:.2e}/{errs[1]:.2e}, "
          f"warm low/up {errs[2]:.2e}/{errs[3]:.2e} px")
    assert all(e <= EPE_TOL for e in errs)
