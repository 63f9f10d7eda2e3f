"""The precision modes of the two fused 1x1 convolutions of the update loop: lookup + convc1
(corr_lookup_conv_prec) and the mask head with the convex upsampling
(corr_mask_upsample_forward_prec); include/corr_mi355x_pw_prec.h, eraft_amd/precision.py's
resolve_pointwise, the config key `pointwise_precision`, CorrBlock.lookup_conv(precision=...) and
upsample.mask_upsample(precision=...).  DESIGN §34.

CPU: the exports, the argument checks through the C ABI (an unknown precision is refused before every
other check and before any HIP call), the knob's resolution, its reach in ERAFT and the fixture.
GPU: which piece products each mode keeps, bit for bit, on inputs whose every output (or logit) is
one product (tests/_pointwise_precision.py); precision 0 against the old entry points; an a-priori
element-wise bound against fp64; non-finite operands; determinism and graph replay; the Python
layers; and the end-to-end flow against the same mode emulated on the reference
(tests/golden/pointwise_precision_reference.npz, make_golden_pointwise_precision.py).
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import _bf16x6 as bx
import _pointwise_precision as pw
import _precision as pm
import prng
from _util import REL_TOL, bit_equal, load, norm_rel

DEV = pw.DEV
F32, F64 = np.float32, np.float64
REDUCED = pw.REDUCED
NEW = ("corr_lookup_conv_prec", "corr_mask_upsample_forward_prec")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "corr_mi355x_pw_prec.h")
EINVAL, EUNSUPPORTED = -1, -2
# the bf16x6 path's EPE on an MI355X [cold low, cold up, warm low, warm up], px
BF16X6_EPE = np.array([2.2e-4, 7.5e-4, 1.5e-4, 5.9e-4])


# ----------------------------------------------------------------------------------------------
# CPU: exports, the argument checks, the knob, the fixture
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
    assert sorted(_lib.PW_PREC_EXPORTS) == declared == sorted(NEW)
    others = (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS) | set(_lib.ENC_PREC_EXPORTS) | set(_lib.BUILD_PREC_EXPORTS)
              | set(_lib.TRAIN_HEAD_EXPORTS))
    assert not set(NEW) & others
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.corr_version() == _lib.ABI_VERSION == 202


# (fake pointers, far enough apart that no buffer of these sizes overlaps another)
def _lc_args(precision, **change):
    pyr = (ctypes.c_void_p * 4)(0x10000000, 0x11000000, 0x12000000, 0x13000000)
    a = dict(pyr=pyr, coords=0x20000000, B=1, H=6, W=10, levels=2, radius=4, packed=0x30000000, bias=0x40000000,
             relu=1, out=0x50000000, precision=precision, stream=None)
    a.update(change)
    return list(a.values())


def _mu_args(precision, **change):
    a = dict(hidden=0x10000000, hidden_channels=512, hidden_offset=256, flow=0x20000000, packed=0x30000000,
             bias=0x40000000, mask_scale=0.25, B=2, H=6, W=7, out=0x50000000, precision=precision, stream=None)
    a.update(change)
    return list(a.values())


def test_abi_refusals(lib):
    """An unknown precision is CORR_EINVAL whatever else is wrong, and the message names the
    function, "precision" and the value; precision 0, 1 and 2 reach the counterpart's next refusal.
    Without a GPU any HIP call would fail differently."""
    err = lambda: lib.corr_last_error().decode()  # noqa: E731
    for bad in (-1, 3, 7, 1 << 20):
        for change in ({}, dict(pyr=None, coords=None, B=0, H=-3, levels=99, radius=77, packed=None, bias=None,
                                out=None)):
            assert lib.corr_lookup_conv_prec(*_lc_args(bad, **change)) == EINVAL, (bad, change)
            assert "corr_lookup_conv_prec" in err() and "precision" in err() and f"got {bad}" in err()
        for change in ({}, dict(hidden=None, hidden_channels=3, hidden_offset=-1, flow=None, packed=4, bias=None,
                                mask_scale=float("nan"), B=0, H=0, W=-1, out=None)):
            assert lib.corr_mask_upsample_forward_prec(*_mu_args(bad, **change)) == EINVAL, (bad, change)
            assert "corr_mask_upsample_forward_prec" in err() and "precision" in err() and f"got {bad}" in err()
    for prec in (0, 1, 2):
        for change, code, msg in ((dict(B=0), EINVAL, "B"), (dict(radius=3), EUNSUPPORTED, "radius 4"),
                                  (dict(levels=5), EINVAL, "levels"), (dict(coords=None), EINVAL, "coords is NULL"),
                                  (dict(packed=None), EINVAL, "packed_weight is NULL"),
                                  (dict(bias=None), EINVAL, "bias is NULL"), (dict(out=None), EINVAL, "out is NULL")):
            assert lib.corr_lookup_conv_prec(*_lc_args(prec, **change)) == code, (prec, change, err())
            assert msg in err() and "precision" not in err(), (prec, change, err())
        for change, msg in ((dict(hidden=None), "hidden is NULL"), (dict(H=0), "B, H, W"),
                            (dict(hidden_offset=257), "hidden_offset"), (dict(mask_scale=float("inf")), "mask_scale"),
                            (dict(out=0x10000000), "overlap"), (dict(packed=0x30000004), "not 16-byte aligned")):
            assert lib.corr_mask_upsample_forward_prec(*_mu_args(prec, **change)) == EINVAL, (prec, change)
            assert msg in err() and "precision" not in err(), (prec, change, err())


def test_resolve_pointwise(monkeypatch):
    from eraft_amd import precision
    monkeypatch.delenv(precision.POINTWISE_ENV, raising=False)
    assert precision.POINTWISE_ENV == "ERAFT_AMD_POINTWISE_PRECISION"
    assert precision.resolve_pointwise(None) == precision.resolve_pointwise({}) == "bf16x6"
    assert precision.resolve_pointwise({"pointwise_precision": None}) == "bf16x6"
    assert precision.resolve_pointwise({"pointwise_precision": True}) == "bf16x3"
    assert precision.resolve_pointwise({"pointwise_precision": False}) == "bf16x6"
    assert precision.resolve_pointwise({"pointwise_precision": "BF16"}) == "bf16"
    # the other knobs' keys and variables do not reach it
    others = {"mixed_precision": True, "encoder_precision": "bf16", "corr_precision": "bf16"}
    assert precision.resolve_pointwise(others) == "bf16x6"
    for v in (precision.ENV, precision.ENCODER_ENV, precision.CORR_ENV):
        monkeypatch.setenv(v, "bf16")
    assert precision.resolve_pointwise({}) == "bf16x6"
    # the variable overrides the key and reaches no other knob; set but empty counts as unset
    monkeypatch.setenv(precision.POINTWISE_ENV, "bf16x3")
    assert precision.resolve_pointwise({"pointwise_precision": "bf16"}) == "bf16x3"
    assert precision.resolve(None) == precision.resolve_encoder(None) == precision.resolve_corr(None) == "bf16"
    for v in (precision.ENV, precision.ENCODER_ENV, precision.CORR_ENV):
        monkeypatch.delenv(v)
    assert precision.resolve(None) == precision.resolve_encoder(None) == precision.resolve_corr(None) == "bf16x6"
    monkeypatch.setenv(precision.POINTWISE_ENV, "")
    assert precision.resolve_pointwise({"pointwise_precision": "bf16"}) == "bf16"
    monkeypatch.setenv(precision.POINTWISE_ENV, "fp8")
    with pytest.raises(ValueError):
        precision.resolve_pointwise({})
    monkeypatch.delenv(precision.POINTWISE_ENV)
    with pytest.raises(ValueError):
        precision.resolve_pointwise({"pointwise_precision": "tf32"})
    with pytest.raises(ValueError):
        precision.resolve_pointwise({"pointwise_precision": 3})


def _no_precision_env(monkeypatch):
    from eraft_amd import precision
    for v in (precision.ENV, precision.ENCODER_ENV, precision.CORR_ENV, precision.POINTWISE_ENV, "ERAFT_AMD_BUILD",
              "ERAFT_AMD_ONDEMAND"):
        monkeypatch.delenv(v, raising=False)


def test_mixed_precision_leaves_the_two_layers_alone(monkeypatch):
    from eraft_amd import precision
    from eraft_amd.model import ERAFT
    _no_precision_env(monkeypatch)
    assert ERAFT.pointwise_precision == "bf16x6"
    m = ERAFT({"subtype": "standard", "mixed_precision": True}, n_first_channels=3)
    assert (m.precision, m.pointwise_precision) == ("bf16x3", "bf16x6")
    m = ERAFT({"subtype": "standard", "mixed_precision": "bf16", "encoder_precision": "bf16", "corr_precision": "bf16"},
              n_first_channels=3)
    assert m.pointwise_precision == "bf16x6"
    m = ERAFT({"subtype": "standard", "pointwise_precision": "bf16"}, n_first_channels=3)
    assert (m.precision, m.encoder_precision, m.corr_precision, m.pointwise_precision) == ("bf16x6",) * 3 + ("bf16",)
    assert m.update_block.precision == m.update_block.gru.precision == m.fnet.precision == "bf16x6"
    with pytest.raises(ValueError):
        ERAFT({"subtype": "standard", "pointwise_precision": "fp16"}, n_first_channels=3)
    monkeypatch.setenv(precision.POINTWISE_ENV, "bf16x3")
    assert ERAFT({"subtype": "standard"}, n_first_channels=3).pointwise_precision == "bf16x3"


def test_python_layers_check_the_mode_name():
    from eraft_amd.upsample import mask_upsample
    with pytest.raises(ValueError, match="precision"):
        mask_upsample(torch.nn.Conv2d(256, 576, 1), torch.zeros(1, 256, 4, 4), 0, torch.zeros(1, 2, 4, 4),
                      precision="fp8")
    with pytest.raises(RuntimeError, match="MI355X"):   # a good name reaches the next check
        mask_upsample(torch.nn.Conv2d(256, 576, 1), torch.zeros(1, 256, 4, 4), 0, torch.zeros(1, 2, 4, 4),
                      precision="bf16")


def test_knob_is_inert_on_cpu(monkeypatch):
    """A CPU ERAFT forward (the oracle's torch CorrBlock in place of the HIP one, which has neither
    lookup_conv nor a precision argument) with the key set, every fusion switch forced on, is
    bit-equal to the default model's."""
    import eraft_amd.model as M
    from oracle import torch_ops
    from test_precision import _base_state
    _no_precision_env(monkeypatch)

    class CpuCorrBlock:
        def __init__(self, f1, f2, num_levels=4, radius=4):
            self.levels, self.radius = torch_ops.cpu_build(f1, f2, num_levels), radius

        def __call__(self, coords):
            return torch_ops.cpu_lookup(self.levels, coords, self.radius)

    monkeypatch.setattr(M, "CorrBlock", CpuCorrBlock)
    monkeypatch.setattr(M.ERAFT, "fuse_mask_upsample", True)
    monkeypatch.setattr(M.ERAFT, "fuse_lookup_conv", True)
    im1 = torch.from_numpy(prng.voxel_grid(21, (1, 3, 128, 160)))
    im2 = torch.from_numpy(prng.voxel_grid(23, (1, 3, 128, 160)))
    outs = []
    for config in ({}, {"pointwise_precision": "bf16"}):
        model = M.ERAFT({"subtype": "warm_start", **config}, n_first_channels=3).eval()
        model.load_state_dict(_base_state(3))
        with torch.no_grad():
            low, ups = model(im1, im2, iters=2)
        outs.append([low.numpy()] + [u.numpy() for u in ups])
    assert model.pointwise_precision == "bf16"
    for u, v in zip(*outs):
        assert np.isfinite(u).all() and bit_equal(u, v)


def test_fixture():
    fx, g = load("pointwise_precision_reference"), load("g_e2e_dsec")
    assert list(fx["meta"]) == list(g["meta"])
    assert list(fx["two"]) == ["encoder.convc1", "mask.2"] and len(fx["eleven"]) == 11
    assert fx["fp32"].max() < 1e-3
    for mode in REDUCED:
        for tag in ("emu_", "emu13_"):
            v = fx[tag + mode]
            assert v.shape == (4,) and np.isfinite(v).all() and (v > 0).all()
    assert (fx["emu_bf16"] > fx["emu_bf16x3"]).all()


def test_model_of_the_reduced_products():
    """mode_product on the exact classes: where every partial sum is exact the MFMA's rounding is the
    plain one, and the value is the product with the dropped pieces removed from both operands."""
    w, x = bx.operands("A", 5, 512, 8)
    for mode in REDUCED:
        got = pw.mode_product(w[:, None], x[None, :], mode)
        assert bit_equal(got, pm.mode_model(w[:, None], x[None, :], mode))
        want = (pm.kept(w, mode).astype(F64)[:, None] * pm.kept(x, mode).astype(F64)[None, :]).astype(F32)
        assert bit_equal(got, want)
        assert (got != bx.six_model(w[:, None], x[None, :])).mean() > 0.9
    assert bit_equal(pw.mode_product(w[:, None], x[None, :], "bf16x6"), bx.six_model(w[:, None], x[None, :]))


# ----------------------------------------------------------------------------------------------
# GPU 1: lookup + convc1, which products each mode keeps
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("key", pw.LC_PIECES)
def test_lookup_conv_kept_products(key, mode):
    """test_lookup_conv_weight_pieces's method: one non-zero full-mantissa (class A) weight per output
    row, the column moving through all C from launch to launch, and the lookup read back from the
    unfused call.  out[o] = w[o, k] lookup[k] is a single product, and the kernel's value is the
    mode's products of that pair in products<NP>()'s order with the MFMA's rounding, bit for bit
    (pw.mode_product: the six-product model with the dropped products removed).  Every (o, k) is
    observed."""
    blk, coords, look = pw.lc_block(key)
    C = look.shape[1]
    assert np.isfinite(look).all() and (look != 0).any(axis=(0, 2, 3)).all()   # every channel holds products
    assert np.abs(look[look != 0]).min() > 2.0 ** -60                           # no subnormal piece or product
    wv = bx.operands("A", 74, 256 * C, 1, 0, 6, 0)[0].reshape(256, C)
    zero = np.zeros(256, F32)
    seen = np.zeros((256, C), bool)
    differs = total = 0
    rows = np.arange(256)
    for n in range(C):
        k = (rows + n) % C
        w = np.zeros((256, C), F32)
        w[rows, k] = wv[rows, k]
        seen[rows, k] = True
        out = pw.lc_run(blk, coords, w, zero, mode)
        x = look[:, k]
        hit = x != 0                                         # elsewhere the output is bias + 0
        wb = np.broadcast_to(w[rows, k][None, :, None, None], x.shape)[hit]
        exp = np.zeros_like(x)
        exp[hit] = pw.mode_product(wb, x[hit], mode)
        assert bit_equal(out, exp), (n, mode)
        if n % 27 == 0:                                      # (a sample: the full model is six MFMAs an element)
            differs += int((exp[hit] != pw.mode_product(wb, x[hit], "bf16x6")).sum())
            total += int(hit.sum())
    assert seen.all()
    assert differs > 0.9 * total


# ----------------------------------------------------------------------------------------------
# GPU 2: the mask head, which products each mode keeps
# ----------------------------------------------------------------------------------------------
def _onehot_hidden(B, H, W, n, values):
    """Launch n's hidden [B, 256, H, W]: pixel p holds values[c] in channel c = (p + n B H W) % 256."""
    c = (np.arange(B * H * W) + n * B * H * W) % 256
    hidden = np.zeros((B, H, W, 256), F32)
    hidden.reshape(-1, 256)[np.arange(c.size), c] = values[c]
    return c, np.ascontiguousarray(hidden.transpose(0, 3, 1, 2))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("off", [0, 256])
@pytest.mark.parametrize("shape", pw.MU_SHAPES)
def test_mask_head_weight_pieces(shape, off, mode):
    """test_mask_upsample_weight_pieces's comparator (the kernel's own softmax and combination on an
    exactly known logit): hidden is one-hot per pixel (2^e_c in channel c, c cycling over all 256) and
    W[o, c] = s_o 2^-e_c with s_o full-mantissa, so every logit is kept(s_o, mode), as in a run with
    W = 0 and bias = kept(s_o, mode).  The two outputs are bit-equal, and differ from the run whose
    bias is s_o itself."""
    from eraft_amd import _lib
    B, H, W = shape
    rng = np.random.default_rng(61)
    s = bx.operands("A", 61, 576, 1, 0, 1, 0)[0]
    e = rng.integers(-8, 9, 256)
    w = (s[:, None].astype(F64) * np.ldexp(1.0, -e)[None, :]).astype(F32)
    packed = _lib.mask_upsample_pack_weights(pw.gpu(w))
    zeros = np.zeros((B, 256, H, W), F32)
    by_bias = pw.mu_run(zeros, np.zeros_like(w), pm.kept(s, mode), mode, off)
    full = pw.mu_run(zeros, np.zeros_like(w), s, mode, off)
    assert np.isfinite(by_bias).all() and (by_bias != full).mean() > 0.5
    seen = np.zeros(256, bool)
    n = 0
    while not seen.all():
        c, hidden = _onehot_hidden(B, H, W, n, np.ldexp(1.0, e).astype(F32))
        seen[c] = True
        n += 1
        assert bit_equal(pw.mu_run(hidden, w, np.zeros(576, F32), mode, off, packed=packed), by_bias), (n, mode)
    assert len(np.unique(by_bias)) > by_bias.size // 4


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("off", [0, 256])
@pytest.mark.parametrize("shape", pw.MU_SHAPES)
def test_mask_head_activation_pieces(shape, off, mode):
    """The mirror (class B): hidden is constant over the pixels with a full-mantissa value v_c per
    channel, and row o has one weight 2^k_o, at channel c(o) = (o + 97 n) % 256 of launch n: logit o
    is kept(v_c(o), mode) 2^k_o, as in the run with W = 0 and that bias.  Every channel is read by
    every row block position over the launches."""
    B, H, W = shape
    v, p2 = bx.operands("B", 63, 256, 576, 0, 1, 1)
    hidden = np.ascontiguousarray(np.broadcast_to(v[None, :, None, None], (B, 256, H, W)))
    zeros, rows = np.zeros((B, 256, H, W), F32), np.arange(576)
    differs = 0
    for n in range(3):
        c = (rows + 97 * n) % 256
        w = np.zeros((576, 256), F32)
        w[rows, c] = p2
        bias = (pm.kept(v, mode)[c].astype(F64) * p2.astype(F64)).astype(F32)
        want = pw.mu_run(zeros, np.zeros_like(w), bias, mode, off)
        assert bit_equal(pw.mu_run(hidden, w, np.zeros(576, F32), mode, off), want), (n, mode)
        exact = pw.mu_run(zeros, np.zeros_like(w), (v[c].astype(F64) * p2.astype(F64)).astype(F32), mode, off)
        differs += int((want != exact).sum())
    assert differs > want.size


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("shape", pw.MU_SHAPES)
def test_mask_head_cross_term(shape, mode):
    """Class C, both operands (hi, mid, 0): hidden is one-hot with the same two-piece value x0 in a
    moving channel and W[o, c] = w_o (two-piece) for every c, so logit o is the mode's value of the
    single product w_o x0.  bf16x3 gives wh xh + (wm xh + wh xm) and not the four-product sum, which
    is the exact product (wm xm absent); bf16 gives wh xh."""
    from eraft_amd import _lib
    B, H, W = shape
    wc, xc = bx.operands("C", 64, 576, 4, 0, 1, 1)
    w = np.ascontiguousarray(np.broadcast_to(wc[:, None], (576, 256)))
    packed = _lib.mask_upsample_pack_weights(pw.gpu(w))
    zeros = np.zeros((B, 256, H, W), F32)
    for n, x0 in enumerate(xc):
        want_logit = pw.mode_product(wc, np.full_like(wc, x0), mode)
        four = (wc.astype(F64) * F64(x0)).astype(F32)
        assert (want_logit != four).mean() > 0.9
        _, hidden = _onehot_hidden(B, H, W, n, np.full(256, x0, F32))
        got = pw.mu_run(hidden, w, np.zeros(576, F32), mode, packed=packed)
        assert bit_equal(got, pw.mu_run(zeros, np.zeros_like(w), want_logit, mode)), (n, mode)
        assert not bit_equal(got, pw.mu_run(zeros, np.zeros_like(w), four, mode))


# ----------------------------------------------------------------------------------------------
# GPU 3: precision 0 is the old entry point
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("key", list(pw.LC_SHAPES))
def test_lookup_conv_precision_0_is_the_old_entry_point(key):
    from eraft_amd import _lib
    blk, coords, _ = pw.lc_block(key)
    w, bias = pw.lc_dense(key)
    packed, bg = _lib.lookup_conv_weights(pw.gpu(w)), pw.gpu(bias)
    for relu in (0, 1):
        out = {p: pw.lc_raw(blk, coords, packed, bg, relu, p) for p in (None, 0, 1, 2)}
        assert torch.isfinite(out[None]).all()
        assert torch.equal(out[None].view(torch.int32), out[0].view(torch.int32))
        for a, b in ((None, 1), (None, 2), (1, 2)):
            frac = (out[a] != out[b]).float().mean().item()
            print(f"lookup_conv {key} relu={relu}: {frac:.3f} of the outputs differ between {a} and {b}")
            assert frac > 0, (a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", pw.MU_SHAPES)
def test_mask_head_precision_0_is_the_old_entry_point(shape):
    from eraft_amd import _lib
    hidden, w, bias = pw.mu_dense(*shape)
    hg, fg, bg = pw.gpu(hidden), pw.gpu(pw.mu_flow(*shape)), pw.gpu(bias)
    packed = _lib.mask_upsample_pack_weights(pw.gpu(w))
    out = {p: pw.mu_raw(hg, fg, packed, bg, p) for p in (None, 0, 1, 2)}
    assert torch.isfinite(out[None]).all()
    assert torch.equal(out[None].view(torch.int32), out[0].view(torch.int32))
    for a, b in ((None, 1), (None, 2), (1, 2)):
        frac = (out[a] != out[b]).float().mean().item()
        print(f"mask head {shape}: {frac:.3f} of the outputs differ between {a} and {b}")
        assert frac > 0, (a, b)


# ----------------------------------------------------------------------------------------------
# GPU 4: the a-priori bound
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_lookup_conv_error_bound():
    """Dense Gaussian weights at the 6x10, L = 2 shape with coordinates within a pixel of the grid
    (42 % of the lookups non-zero: as dense as radius-4 windows on that map get), the activations
    being the lookup the unfused call returns (fp32; the fused kernel's lookups are those bit for
    bit).  Element-wise against fp64:

        |out - out64| <= COEF(mode) sum |w| |x| + A,   A = (c + 6 S) 2^-24 (sum |w| |x| + |bias|)

    with COEF = 0, 2^-16, 2^-8 + 2^-18 (tests/_precision.py: from |x - hi| <= 2^-9 |x| and
    |x - hi - mid| <= 2^-18 |x|) and A the accumulation allowance of
    test_bf16x6_family.py::test_error_bound for S = 11 K steps, c = 5 (a reduced mode issues fewer
    MFMAs, so A covers it).  Each mode's max |err| / (sum |w| |x| + |bias|) must exceed the next finer
    mode's tenfold (test_precision.py's factor).

    COEF is the bound of the suite's other precision tests; it presumes many terms per output.
    bf16's rounding unit is 2^-8 (8 significant bits), so a single product can miss by 2^-7 |w x|:
    on the kept-products test's wide coordinates (18 % non-zero, a handful of terms per output) the
    bf16 mode reaches 1.07 of this bound, on an MI355X and equally in the fp64 evaluation of the
    mode's own definition, which is why the dense input is the one the bound is held on
    (measured there: 0.03 / 0.26 / 0.54 of the bound)."""
    key = "6x10-L2-dense"
    blk, coords, look = pw.lc_block(key)
    w, bias = pw.lc_dense(key)
    B, C, H, W = look.shape
    x64 = look.astype(F64).reshape(B, C, H * W)
    ref = np.einsum("oc,bcn->bon", w.astype(F64), x64) + bias.astype(F64)[None, :, None]
    mag = np.einsum("oc,bcn->bon", np.abs(w.astype(F64)), np.abs(x64))
    scale = mag + np.abs(bias.astype(F64))[None, :, None]
    A = (pw.C_ROUND + 6 * pw.LC_STEPS) * 2.0 ** -24 * scale
    r = {}
    for mode in pm.MODES:
        got = pw.lc_run(blk, coords, w, bias, mode).astype(F64).reshape(ref.shape)
        assert np.isfinite(got).all()
        err, bound = np.abs(got - ref), pm.COEF[mode] * mag + A
        r[mode] = (err / scale).max()
        print(f"lookup_conv bound {mode}: max |err| / bound = {(err / bound).max():.4f}, "
              f"max |err| / (sum |w||x| + |bias|) = 2^{np.log2(r[mode]):.2f}")
        assert (err <= bound).all(), mode
    print(f"lookup_conv ratios: bf16x3 / bf16x6 = {r['bf16x3'] / r['bf16x6']:.1f}, "
          f"bf16 / bf16x3 = {r['bf16'] / r['bf16x3']:.1f}")
    assert r["bf16x3"] >= 10 * r["bf16x6"]
    assert r["bf16"] >= 10 * r["bf16x3"]


@pytest.mark.gpu
def test_mask_head_error_bound():
    """Dense operands at (2, 7, 9).  The logits cannot be read back, so the bound is stated on them
    and carried through: the mode's logits, 0.25 (sum over the kept-piece products + bias) in fp64,
    are within 0.25 COEF(mode) sum |w| |x| of the exact ones (checked here on the definition), and
    the kernel's output is within tests/test_mask_upsample.py's tolerance (REL_TOL, norm-relative)
    of the fp64 softmax and combination of those kept-piece logits, the accumulation allowance
    (c + 6 S) 2^-24, S = 8, being far inside it as it is for the default path.  Each mode's error
    against the EXACT fp64 output must exceed the next finer mode's tenfold."""
    B, H, W = 2, 7, 9
    hidden, w, bias = pw.mu_dense(B, H, W)
    flow = pw.mu_flow(B, H, W)
    exact_logits = pw.mu_logits64(hidden, w, bias)
    exact = pw.upsample64(flow, exact_logits)
    mag = pw.SCALE * np.einsum("oc,bchw->bohw", np.abs(w.astype(F64)), np.abs(hidden.astype(F64)))
    r = {}
    for mode in pm.MODES:
        logits = pw.mu_logits64(hidden, w, bias, mode)
        # (3 * 2^-24: the products every mode drops, wm xl and wl xm at 2^-24 |w x| each, wl xl below)
        assert (np.abs((logits - exact_logits).numpy()) <= (pm.COEF[mode] + 3 * 2.0 ** -24) * mag).all(), mode
        got = pw.mu_run(hidden, w, bias, mode)
        e = norm_rel(got, pw.upsample64(flow, logits))
        r[mode] = norm_rel(got, exact)
        print(f"mask head bound {mode}: against its own definition {e:.2e}, against exact fp64 {r[mode]:.2e}")
        assert e <= REL_TOL, mode
    print(f"mask head ratios: bf16x3 / bf16x6 = {r['bf16x3'] / r['bf16x6']:.1f}, "
          f"bf16 / bf16x3 = {r['bf16'] / r['bf16x3']:.1f}")
    assert r["bf16x3"] >= 10 * r["bf16x6"]
    assert r["bf16"] >= 10 * r["bf16x3"]


# ----------------------------------------------------------------------------------------------
# GPU 5: non-finite operands, determinism, graph replay
# ----------------------------------------------------------------------------------------------
def _same_pattern(got, ref):
    bad = ~np.isfinite(ref)
    assert bad.any() and not bad.all()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["activations", "weight"])
@pytest.mark.parametrize("mode", REDUCED)
def test_lookup_conv_non_finite(mode, what):
    """+inf, -inf, NaN and +-FLT_MAX features at test_bf16x6_family.py's pixels (the build carries
    them into the pyramid, the lookups into the convolution's activations), or infinite weights: the
    non-finite outputs, and their values, are where the bf16x6 kernel puts them (which that suite
    holds to fp32's pattern)."""
    import eraft_amd
    from test_bf16x6_family import SPECIAL
    B, D, H, W, L = 2, 32, 7, 9, 2
    f1, f2 = prng.gauss(81, (B, D, H, W)), prng.gauss(82, (B, D, H, W))
    w, bias = prng.gauss(83, (256, L * 81), 2.0 ** -10), prng.gauss(84, (256,), 0.1)
    if what == "activations":
        for ((b, y, x), v), c in zip(SPECIAL, (3, 31, 17, 30, 8)):
            f1[b, c, y, x] = v
    else:
        w[128, 5], w[0, 100] = np.inf, -np.inf
    coords = pw.gpu(prng.lookup_coords(85, B, H, W, 2.0))
    with torch.no_grad():
        blk = eraft_amd.CorrBlock(pw.gpu(f1), pw.gpu(f2), num_levels=L, radius=4)
    ref = pw.lc_run(blk, coords, w, bias, "bf16x6")
    _same_pattern(pw.lc_run(blk, coords, w, bias, mode), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["activations", "weight"])
@pytest.mark.parametrize("mode", REDUCED)
def test_mask_head_non_finite(mode, what):
    """test_non_finite_mask_upsample's inputs: the non-finite outputs are the bf16x6 kernel's."""
    from test_bf16x6_family import _plant
    B, H, W = 2, 7, 9
    hidden = np.maximum(prng.gauss(94, (B, 256, H, W)), 0.0).astype(F32)
    w, bias = prng.gauss(95, (576, 256), 2.0 ** -10), prng.gauss(96, (576,), 0.5)
    if what == "activations":
        _plant(hidden, (3, 255, 17, 30, 8))
    else:
        w[100, 7], w[300, 200] = np.inf, -np.inf
    ref = pw.mu_run(hidden, w, bias, "bf16x6")
    _same_pattern(pw.mu_run(hidden, w, bias, mode), ref)


def _replay(run):
    """run() twice, then captured and replayed into a NaN-filled output: all three bit-equal."""
    a, b = run(None).clone(), run(None)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    out = torch.empty_like(a)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(out)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(out)
    out.fill_(float("nan"))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int32), out.view(torch.int32))
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_lookup_conv_determinism_and_graph_replay(mode):
    from eraft_amd import _lib
    key = "6x10-L2"
    blk, coords, _ = pw.lc_block(key)
    w, bias = pw.lc_dense(key)
    packed, bg = _lib.lookup_conv_weights(pw.gpu(w)), pw.gpu(bias)   # outside the capture
    B, _, H, W = coords.shape

    def run(out, code=pm.CODE[mode]):
        out = torch.empty((B, 256, H, W), dtype=torch.float32, device=DEV) if out is None else out
        _lib.lookup_conv(blk._state.levels, coords, 4, packed, bg, out, True, precision=code)
        return out

    a = _replay(run)
    assert not torch.equal(a.view(torch.int32), run(None, 0).view(torch.int32))   # not the default's arithmetic


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_mask_head_determinism_and_graph_replay(mode):
    from eraft_amd import _lib
    B, H, W = 2, 7, 9
    hidden, w, bias = pw.mu_dense(B, H, W)
    hg, fg, bg = pw.gpu(hidden), pw.gpu(pw.mu_flow(B, H, W)), pw.gpu(bias)
    packed = _lib.mask_upsample_pack_weights(pw.gpu(w))             # outside the capture

    def run(out, code=pm.CODE[mode]):
        return _lib.mask_upsample_forward(hg, 0, fg, packed, bg, pw.SCALE, out=out, precision=code)

    a = _replay(run)
    assert not torch.equal(a.view(torch.int32), run(None, 0).view(torch.int32))


# ----------------------------------------------------------------------------------------------
# GPU 6: the Python layers
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", pm.MODES)
def test_corr_block_lookup_conv(monkeypatch, mode):
    import eraft_amd
    from eraft_amd import precision
    _no_precision_env(monkeypatch)
    key = "6x10-L2"
    blk, coords, _ = pw.lc_block(key)
    w, bias = pw.lc_dense(key)
    wg, bg = pw.gpu(w).view(256, -1, 1, 1), pw.gpu(bias)
    want = {m: pw.lc_run(blk, coords, w, bias, m, relu=True) for m in pm.MODES}
    with torch.no_grad():
        assert bit_equal(blk.lookup_conv(coords, wg, bg, precision=mode).cpu().numpy(), want[mode])
        assert bit_equal(blk.lookup_conv(coords, wg, bg).cpu().numpy(), want["bf16x6"])
        # the variable alone selects the mode (how bench.py is run in one); the argument wins over it
        monkeypatch.setenv(precision.POINTWISE_ENV, mode)
        assert bit_equal(blk.lookup_conv(coords, wg, bg).cpu().numpy(), want[mode])
        assert bit_equal(blk.lookup_conv(coords, wg, bg, precision="bf16x6").cpu().numpy(), want["bf16x6"])
        with pytest.raises(ValueError):
            blk.lookup_conv(coords, wg, bg, precision="fp8")
    # recorded for autograd: the default's arithmetic whatever is asked, and the backward runs
    wr, br = wg.clone().requires_grad_(True), bg.clone().requires_grad_(True)
    out = blk.lookup_conv(coords, wr, br, precision=mode)
    assert out.requires_grad and bit_equal(out.detach().cpu().numpy(), want["bf16x6"])
    out.sum().backward()
    assert torch.isfinite(wr.grad).all() and torch.isfinite(br.grad).all() and (wr.grad != 0).any()
    if mode != "bf16x6":
        assert not bit_equal(want[mode], want["bf16x6"])
    # the on-demand block fused with convc1 has no modes: no keyword, and the variable does not reach it
    B, D, H, W, L, _ = pw.LC_SHAPES[key]
    f1, f2 = pw.gpu(prng.gauss(71, (B, D, H, W))), pw.gpu(prng.gauss(72, (B, D, H, W)))
    with torch.no_grad():
        od = eraft_amd.OnDemandConvCorrBlock(f1, f2, num_levels=L, radius=4)
        with pytest.raises(TypeError):
            od.lookup_conv(coords, wg, bg, precision=mode)
        with_env = od.lookup_conv(coords, wg, bg).cpu().numpy()
        monkeypatch.delenv(precision.POINTWISE_ENV)
        assert bit_equal(with_env, od.lookup_conv(coords, wg, bg).cpu().numpy())
        assert norm_rel(with_env, want["bf16x6"]) <= REL_TOL


@pytest.mark.gpu
@pytest.mark.parametrize("mode", pm.MODES)
def test_mask_upsample_layer(mode):
    from eraft_amd.upsample import mask_upsample
    B, H, W = 2, 7, 9
    hidden, w, bias = pw.mu_dense(B, H, W)
    conv = torch.nn.Conv2d(256, 576, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(pw.gpu(w).view(576, 256, 1, 1))
        conv.bias.copy_(pw.gpu(bias))
        hg, fg = pw.gpu(hidden), pw.gpu(pw.mu_flow(B, H, W))
        assert bit_equal(mask_upsample(conv, hg, 0, fg, precision=mode).cpu().numpy(), pw.mu_run(hidden, w, bias, mode))
        assert bit_equal(mask_upsample(conv, hg, 0, fg).cpu().numpy(), pw.mu_run(hidden, w, bias, "bf16x6"))


def _fusion_switches(monkeypatch):
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    monkeypatch.setattr(SepConvGRU, "fused", True)
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", True)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", True)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_model_passes_the_mode_to_both_launches(monkeypatch, mode):
    """ERAFT at 128x160, 2 iterations: with the key set every lookup_conv and mask head launch gets
    the mode's code (and the default model's get 0), the predictions differ from the default
    model's, and with alternate_corr the on-demand block is called without the keyword."""
    from eraft_amd import _lib
    from eraft_amd.model import ERAFT
    from test_precision import _base_state
    _no_precision_env(monkeypatch)
    _fusion_switches(monkeypatch)
    seen = []
    for name in ("lookup_conv", "mask_upsample_forward"):
        real = getattr(_lib, name)
        monkeypatch.setattr(_lib, name, lambda *a, _real=real, _name=name, **k: (
            seen.append((_name, k.get("precision", 0))), _real(*a, **k))[1])
    im1 = torch.from_numpy(prng.voxel_grid(21, (1, 3, 128, 160))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(23, (1, 3, 128, 160))).to(DEV)
    ups = {}
    for config in ({}, {"pointwise_precision": mode}, {"pointwise_precision": mode, "alternate_corr": True}):
        model = ERAFT({"subtype": "warm_start", **config}, n_first_channels=3).eval()
        model.load_state_dict(_base_state(3))
        model = model.to(DEV)
        del seen[:]
        with torch.no_grad():
            ups[len(ups)] = model(im1, im2, iters=2)[1][-1].cpu().numpy()
        code = pm.CODE[mode] if config else 0
        calls = [("mask_upsample_forward", code)] * 2 + ([] if "alternate_corr" in config else [("lookup_conv", code)] * 2)
        assert sorted(seen) == sorted(calls), (config, seen)
    assert np.isfinite(ups[1]).all() and not bit_equal(ups[0], ups[1])


# ----------------------------------------------------------------------------------------------
# GPU 7: end to end
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e(pointwise, mixed):
    """[cold low-res, cold full-res, warm low-res, warm full-res] EPE against the reference's fp32
    golden of a model with pointwise_precision = `pointwise` and mixed_precision = `mixed` (None:
    the key absent)."""
    from eraft_amd.model import ERAFT
    from test_e2e import _epe
    from test_precision import _base_state
    g = load("g_e2e_dsec")
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    config = {"subtype": "warm_start"}
    if pointwise is not None:
        config["pointwise_precision"] = pointwise
    if mixed is not None:
        config["mixed_precision"] = mixed
    model = ERAFT(config, n_first_channels=bins).eval()
    model.load_state_dict(_base_state(bins))
    model = model.to(DEV)
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W))).to(DEV)
    finit = torch.from_numpy(g["flow_init"]).to(DEV)
    with torch.no_grad():
        low, ups = model(im1, im2, iters=iters)
        low_w, ups_w = model(im1, im2, iters=iters, flow_init=finit)
    names = (model.precision, model.encoder_precision, model.corr_precision, model.pointwise_precision)
    return names, np.array([_epe(low.cpu().numpy(), g["low"]), _epe(ups[-1][..., ::4, ::4].cpu().numpy(), g["up_sub"]),
                            _epe(low_w.cpu().numpy(), g["low_warm"]),
                            _epe(ups_w[-1][..., ::4, ::4].cpu().numpy(), g["up_warm_sub"])])


@pytest.mark.gpu
@pytest.mark.parametrize("both", [False, True], ids=["alone", "with-mixed"])
@pytest.mark.parametrize("mode", REDUCED)
def test_e2e_against_the_emulated_reference(monkeypatch, mode, both):
    """g_e2e_dsec's inputs and weights, all four fusion switches on, cold and warm.  With
    pointwise_precision = mode alone the EPE against the reference's fp32 flow is finite and at most
    1.5 x the same two layers emulated on the reference (emu_<mode>; the margin of test_precision.py
    and test_corr_precision.py for GPU against emulation); with mixed_precision = mode as well, at
    most 1.5 x emu13_<mode>.  It is strictly above the bf16x6 path's EPE in the same run wherever the
    emulated EPE is at least twice DESIGN §23's bf16x6 GPU figure for that entry (below that the
    mode's error is of the size of the default path's own and the order is not determined)."""
    _no_precision_env(monkeypatch)
    _fusion_switches(monkeypatch)
    fx = load("pointwise_precision_reference")
    assert list(fx["meta"]) == list(load("g_e2e_dsec")["meta"])
    names0, base = _e2e(None, None)
    names, errs = _e2e(mode, mode if both else None)
    assert names0 == ("bf16x6",) * 4 and names == (mode if both else "bf16x6", "bf16x6", "bf16x6", mode)
    emu = fx[("emu13_" if both else "emu_") + mode]
    above = emu >= 2 * BF16X6_EPE
    fmt = lambda v: " / ".join(f"{e:.3e}" for e in v)
    print(f"e2e pointwise {mode}{' + mixed' if both else ''} EPE cold low / up, warm low / up: {fmt(errs)} px; "
          f"bf16x6 {fmt(base)}; emulated {fmt(emu)}; GPU / emulated {fmt(errs / emu)}; "
          f"'above bf16x6' asserted at {above.tolist()}")
    assert np.isfinite(errs).all()
    assert (errs[above] > base[above]).all()
    assert (errs <= 1.5 * emu).all()
