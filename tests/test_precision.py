"""The reduced precision modes of the per-iteration kernels (corr_gru_half_step_prec,
corr_conv_forward_prec, eraft_amd/precision.py, the config key `mixed_precision`).

CPU: the exports, the validation (an unknown precision is refused before any HIP call), the switch
and its resolver, that the mode is inert off the GPU, the numpy model of the modes
(tests/_precision.py) and the fixture's conditions on its own emulated numbers.  GPU: which products
each mode keeps, bit for bit, with tests/test_bf16x6_family.py's method; an a-priori element-wise
error bound from the split's definition; the GRU half step against its own definition per launch;
the non-finite rule; determinism and graph capture; the module path; and the end-to-end flow against
the reference's own mixed precision (tests/golden/precision_reference.npz,
make_golden_precision.py).
"""
import copy
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bf16x6 as bx
import _precision as pm
import prng
import test_bf16x6_family as fam
from _util import REL_TOL, bit_equal, load, norm_rel

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
HID = 128
EINVAL = -1
REDUCED = ("bf16x3", "bf16")
NEW = ("corr_gru_half_step_prec", "corr_conv_forward_prec")


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


# ----------------------------------------------------------------------------------------------
# CPU: exports and validation
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def test_exports(lib):
    import re
    from eraft_amd import _lib
    from test_abi import HEADER, _declared
    src = open(HEADER).read()
    for name in NEW:
        assert name in _lib.EXPORTS, name
        assert name in _declared(), name
        assert hasattr(lib, name), name
    for k, name in enumerate(("CORR_PREC_BF16X6", "CORR_PREC_BF16X3", "CORR_PREC_BF16")):
        assert re.search(rf"#define {name} {k}\b", src), name
    assert lib.corr_version() == 202


# the existing entry points' good arguments (tests/test_gru.py, tests/test_conv.py) with `precision`
# before `stream`
_GRU = dict(h=0x1000, x=0x2000, B=1, hidden=HID, input=320, H=6, W=7, dir=0, packed=0x3000, bz=0x4000, br=0x5000,
            bq=0x6000, ws=0x7000, ws_bytes=2 * HID * 42 * 4, h_out=0x8000, precision=0, stream=None)
_CONV = dict(in_a=0x10000000, ca=192, in_b=0x20000000, cb=64, B=2, H=6, W=7, packed=0x30000000, bias=0x40000000,
             cout=126, relu=1, out=0x50000000, out_channels=256, out_offset=128, precision=0, stream=None)


@pytest.mark.parametrize("fn,good", [(NEW[0], _GRU), (NEW[1], _CONV)])
def test_validation(lib, fn, good):
    """Dummy pointers, never dereferenced: an unknown precision is CORR_EINVAL whatever else is
    wrong, and 0, 1, 2 get past that check to the next refusal (B = 0)."""
    call = getattr(lib, fn)
    for bad in (-1, 3):
        for other in ({}, {"B": 0}):
            assert call(*dict(good, precision=bad, **other).values()) == EINVAL
            msg = lib.corr_last_error().decode()
            assert fn in msg and "precision" in msg and str(bad) in msg
    for ok in (0, 1, 2):
        assert call(*dict(good, precision=ok, B=0).values()) == EINVAL
        msg = lib.corr_last_error().decode()
        assert "B, H, W" in msg and "precision" not in msg


# ----------------------------------------------------------------------------------------------
# CPU: the switch
# ----------------------------------------------------------------------------------------------
def _eraft(config=None, bins=3):
    from eraft_amd.model import ERAFT
    return ERAFT(dict({"subtype": "standard"}, **(config or {})), n_first_channels=bins).eval()


def test_resolver(monkeypatch):
    from eraft_amd import precision
    monkeypatch.delenv("ERAFT_AMD_PRECISION", raising=False)
    assert [precision.code(n) for n in pm.MODES] == [0, 1, 2]
    for bad in ("fp16", "BF16X3 ", "", None, 1, True):
        with pytest.raises(ValueError):
            precision.code(bad)
    assert precision.resolve({}) == precision.resolve({"mixed_precision": False}) == "bf16x6"
    assert precision.resolve(None) == "bf16x6"
    assert precision.resolve({"mixed_precision": True}) == "bf16x3"
    assert precision.resolve({"mixed_precision": "bf16"}) == "bf16"
    for bad in ("float16", 2, 0.5):
        with pytest.raises(ValueError):
            precision.resolve({"mixed_precision": bad})


def test_config_key_and_environment(monkeypatch):
    from eraft_amd.model import ERAFT, BasicUpdateBlock, SepConvGRU
    monkeypatch.delenv("ERAFT_AMD_PRECISION", raising=False)
    assert ERAFT.precision == BasicUpdateBlock.precision == SepConvGRU.precision == "bf16x6"
    assert "precision" not in vars(SepConvGRU()) and "precision" not in vars(BasicUpdateBlock())
    for config, want in (({}, "bf16x6"), ({"mixed_precision": False}, "bf16x6"), ({"mixed_precision": True}, "bf16x3"),
                         ({"mixed_precision": "bf16"}, "bf16"), ({"mixed_precision": "bf16x6"}, "bf16x6")):
        m = _eraft(config)
        assert m.precision == m.update_block.precision == m.update_block.gru.precision == want, config
    with pytest.raises(ValueError):
        _eraft({"mixed_precision": "fp16"})
    # the environment overrides the key, as ERAFT_AMD_ONDEMAND overrides alternate_corr
    monkeypatch.setenv("ERAFT_AMD_PRECISION", "bf16")
    for config in ({}, {"mixed_precision": True}, {"mixed_precision": "bf16x6"}):
        m = _eraft(config)
        assert m.precision == m.update_block.precision == m.update_block.gru.precision == "bf16"
    monkeypatch.setenv("ERAFT_AMD_PRECISION", "bf16x6")
    assert _eraft({"mixed_precision": True}).precision == "bf16x6"
    monkeypatch.setenv("ERAFT_AMD_PRECISION", "half")
    with pytest.raises(ValueError):
        _eraft({})
    monkeypatch.setenv("ERAFT_AMD_PRECISION", "")   # set but empty: as unset
    assert _eraft({}).precision == "bf16x6" and _eraft({"mixed_precision": True}).precision == "bf16x3"


def test_mode_is_inert_on_cpu(monkeypatch):
    """The update block (the GRU inside it) of a model with mixed_precision=True, on CPU tensors with
    the fused switches on, is the torch path: bit-identical to a model without the key."""
    from eraft_amd.model import BasicUpdateBlock, SepConvGRU
    from test_conv import _block_inputs
    monkeypatch.delenv("ERAFT_AMD_PRECISION", raising=False)
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(SepConvGRU, "fused", True)
    plain = _eraft({})
    arrs = [torch.from_numpy(a) for a in _block_inputs(5, 1, 6, 7)]
    for key in (True, "bf16"):
        mixed = _eraft({"mixed_precision": key})
        want = "bf16x3" if key is True else key
        assert mixed.precision == mixed.update_block.precision == mixed.update_block.gru.precision == want
        mixed.load_state_dict(plain.state_dict())
        with torch.no_grad():
            a, b = plain.update_block(*arrs), mixed.update_block(*arrs)
        assert all(bit_equal(u.numpy(), v.numpy()) for u, v in zip(a, b))


# ----------------------------------------------------------------------------------------------
# CPU: the model of the modes, and the fixture
# ----------------------------------------------------------------------------------------------
def test_model_of_the_modes():
    """Class C (pieces (hi, mid, 0) in both operands): bf16x3 is six() without wm xm, bit for bit, and
    differs from six().  Class A (full-mantissa w against +-2^e): bf16x3 gives (wh + wm) x and bf16
    wh x, both exact in fp32.  These are the expected values of the GPU tests."""
    for seed in (1, 2, 3):
        full, point = bx.operands("C", seed, 3000, 48)
        w, x = full[:, None], point[None, :]
        three = pm.mode_model(w, x, "bf16x3")
        assert bx.bits_equal(three, bx.six_model(w, x, drop="wm_xm"))
        assert not (three.view(np.uint32) == bx.six_model(w, x).view(np.uint32)).any()
        assert bx.bits_equal(pm.mode_model(w, x, "bf16x6"), bx.six_model(w, x))
        full, point = bx.operands("A", seed, 3000, 48)
        w, x = full[:, None], point[None, :]
        wh, wm, wl = (p.astype(F64) for p in bx.split3(w))
        for mode, exact in (("bf16x3", (wh + wm) * x), ("bf16", wh * x)):
            got = pm.mode_model(w, x, mode)
            assert (got.astype(F64) == exact).all(), mode
            assert bx.bits_equal(got, pm.kept(w, mode) * x)
            assert not (got == bx.six_model(w, x)).any()
    # the non-finite rule is split_sum's in every mode
    for mode in pm.MODES:
        assert pm.mode_model(np.array([np.inf], F32), np.array([2.0], F32), mode)[0] == np.inf
        assert pm.mode_model(np.array([-3.0], F32), np.array([np.inf], F32), mode)[0] == -np.inf
        assert np.isnan(pm.mode_model(np.array([np.nan], F32), np.array([1.0], F32), mode)[0])


def test_fixture_conditions():
    """The margins that test_e2e_against_the_references_mixed_precision applies hold on the fixture's
    own emulated EPEs (cold and warm, low-res and full-res), and the fixture is the issue's table."""
    g = load("precision_reference")
    for key in ("emu_bf16x3", "emu_bf16", "autocast_float16", "autocast_bfloat16"):
        assert g[key].shape == (4,) and np.isfinite(g[key]).all() and (g[key] > 0).all(), key
    assert (g["emu_bf16x3"] <= g["autocast_float16"] / 8).all()
    assert (g["emu_bf16"] <= 1.5 * g["autocast_bfloat16"]).all()
    assert g["emu_bf16x3"][1] <= 7.7e-3 <= 0.716 / 8 and g["emu_bf16"][1] <= 2.32 <= 1.5 * 2.878
    assert np.allclose(g["autocast_float16"], [0.208, 0.716, 0.168, 0.646], atol=1e-3)
    assert np.allclose(g["autocast_bfloat16"], [0.906, 2.878, 0.799, 2.806], atol=1e-3)
    assert (g["emu_bf16x3"] < g["emu_bf16"] / 100).all()
    assert list(g["meta"]) == list(load("g_e2e_dsec")["meta"])
    assert len(g["eleven"]) == 11


# ----------------------------------------------------------------------------------------------
# GPU: which products each mode keeps, bit for bit (corr_conv_forward_prec)
# ----------------------------------------------------------------------------------------------
CONV_X, CONV_W = (2, 32, 7, 9), (33, 32, 3, 3)


def _conv(x, w, mode, bias=None, relu=False):
    from eraft_amd import _lib
    cout = w.shape[0]
    packed = _lib.conv_pack_weights(_gpu(w))
    bg = _gpu(np.zeros(cout, F32) if bias is None else bias)
    return _lib.conv_forward(_gpu(x), None, packed, bg, cout, relu, precision=pm.CODE[mode]).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_conv_weight_pieces(mode):
    """Class A weights against impulses +-2^e: the output is the product with the weight's lo piece
    (bf16x3), or its mid and lo pieces (bf16), removed, exactly; every (cout, cin, tap) is observed."""
    w, plan, launches = fam.impulse_launches("A", 101, CONV_X, CONV_W, 1, 1)
    wk, seen = pm.kept(w, mode), np.zeros(CONV_W, bool)
    for x, sites, exp6 in launches:
        bx.observe(plan, sites, exp6, seen)
        exp = bx.expected_conv(x, wk, 1, 1)
        assert not bit_equal(exp, exp6)
        assert bit_equal(_conv(x, w, mode), exp)
    assert seen.all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_conv_activation_pieces(mode):
    """Class B activations under one-hot weights +-2^e: the same on the activation's side."""
    x, launches = fam.onehot_launches(102, CONV_X, CONV_W, 1, 1)
    fam._assert_onehot_coverage(launches, CONV_W)
    xk = pm.kept(x, mode)
    for w, exp6 in launches:
        exp = bx.expected_conv(xk, w, 1, 1)
        assert not bit_equal(exp, exp6)
        assert bit_equal(_conv(x, w, mode), exp)


@pytest.mark.gpu
def test_conv_cross_terms():
    """Class C in both operands: bf16x3 is the three-product sum (six() without wm xm), not the
    four-product one; bf16 is wh xh."""
    w, plan, launches = fam.impulse_launches("C", 103, CONV_X, CONV_W, 1, 1, max_launches=9, full=False)
    for x, sites, exp6 in launches:
        three = fam._model_conv(x, w, 1, 1, drop="wm_xm")
        assert np.count_nonzero(exp6) >= CONV_W[0] and not bit_equal(three, exp6)
        assert bit_equal(_conv(x, w, "bf16x3"), three)
        assert bit_equal(_conv(x, w, "bf16"), bx.expected_conv(pm.kept(x, "bf16"), pm.kept(w, "bf16"), 1, 1))
        assert bit_equal(_conv(x, w, "bf16x6"), exp6)


@pytest.mark.gpu
def test_conv_precision_zero_is_the_old_entry_point():
    from eraft_amd import _lib
    lib = _lib.load()
    for (B, H, W), ca, cb, cout in (((2, 7, 9), 192, 64, 126), ((1, 5, 35), 128, 0, 512)):
        x, w = prng.gauss(111, (B, ca + cb, H, W)), prng.gauss(112, (cout, ca + cb, 3, 3), 0.1)
        bias = _gpu(prng.gauss(113, (cout,), 0.1))
        xg = _gpu(x)
        a, b = xg[:, :ca].contiguous(), (xg[:, ca:].contiguous() if cb else None)
        packed = _lib.conv_pack_weights(_gpu(w))
        new = _lib.conv_forward(a, b, packed, bias, cout, True, precision=0)
        old = torch.empty_like(new)
        torch.cuda.synchronize()
        rc = lib.corr_conv_forward(a.data_ptr(), ca, b.data_ptr() if cb else None, cb, B, H, W, packed.data_ptr(),
                                   bias.data_ptr(), cout, 1, old.data_ptr(), cout, 0, None)
        torch.cuda.synchronize()
        assert rc == 0, lib.corr_last_error().decode()
        assert bit_equal(new.cpu().numpy(), old.cpu().numpy())
        for mode in REDUCED:
            assert not bit_equal(_lib.conv_forward(a, b, packed, bias, cout, True, precision=pm.CODE[mode]).cpu().numpy(),
                                 old.cpu().numpy()), mode


# ----------------------------------------------------------------------------------------------
# GPU: the same for the GRU's candidate convolution (gates saturated: h' = tanhf(s))
# ----------------------------------------------------------------------------------------------
GRU_CASES = [(0, (2, 7, 9)), (1, (1, 13, 5))]


def _gru(h, x, d, ws, bs, mode, workspace=None):
    """gru_half_step of numpy inputs in `mode`; ws = (wz, wr, wq) [128, C, kh, kw] (None: zero)."""
    from eraft_amd import _lib
    k, _ = fam._gru_geo(d)
    zero = torch.zeros((HID, h.shape[1] + x.shape[1]) + k, device=DEV)
    packed = _lib.gru_pack_weights(*(zero if w is None else _gpu(w) for w in ws))
    bg = [_gpu(np.broadcast_to(F32(b), (HID,))) for b in bs]
    return _lib.gru_half_step(_gpu(h), _gpu(x), d, packed, *bg, workspace=workspace,
                              precision=pm.CODE[mode]).cpu().numpy()


def _q(x, d, wq, mode):
    return _gru(x[:, :HID], x[:, HID:], d, (None, None, wq), (100.0, 100.0, 0.0), mode)


def _moved(a, b):
    """Some element of a is more than two ulps from b: one ulp of slack cannot hide the difference."""
    return (np.abs(a.astype(F64) - b.astype(F64)) > 2 * np.spacing(np.abs(b)).astype(F64)).any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("d,shape", GRU_CASES)
def test_gru_q_weight_pieces(d, shape, mode):
    """Class A candidate weights against impulses, z = r = 1: h' = tanhf(s) within one ulp of the
    product without the weight's dropped pieces (a dropped lo piece moves s by up to 128 ulp)."""
    k, pad = fam._gru_geo(d)
    B, H, W = shape
    w, plan, launches = fam.impulse_launches("A", 31 + d, (B, fam.GRU_C, H, W), (HID, fam.GRU_C) + k, 1, pad,
                                             **fam.GRU_SCALE, max_launches=6, full=False)
    wk = pm.kept(w, mode)
    for x, sites, exp6 in launches:
        exp = bx.expected_conv(x, wk, 1, pad)
        fam._assert_tanh_is_identity(exp)
        assert _moved(exp, exp6)
        fam._assert_within_one_ulp(_q(x, d, w, mode), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("d,shape", GRU_CASES)
def test_gru_q_activation_pieces(d, shape, mode):
    """Class B h and x under one-hot candidate weights: the same on the activation's side."""
    k, pad = fam._gru_geo(d)
    B, H, W = shape
    C = fam.GRU_C
    xv, pv = bx.operands("B", 41 + d, B * C * H * W, 1024, fam.GRU_SCALE["scale"], *fam.GRU_SCALE["spread"])
    x = xv.reshape(B, C, H, W)
    xk = pm.kept(x, mode)
    for n in (0, 7, 17):   # r h channels, x channels, the last (channel, tap) pairs
        o = np.arange(HID)
        j = (n * HID + o) % (C * 5)
        w = np.zeros((HID, C, 5), F32)
        w[o, j // 5, j % 5] = pv[(n * HID + o) % pv.size]
        w = w.reshape((HID, C) + k)
        exp = bx.expected_conv(xk, w, 1, pad)
        fam._assert_tanh_is_identity(exp)
        assert _moved(exp, bx.expected_conv(x, w, 1, pad))
        fam._assert_within_one_ulp(_q(x, d, w, mode), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("d,shape", GRU_CASES)
def test_gru_q_cross_terms(d, shape):
    """Class C in both operands: bf16x3 is the three-product sum, not the four-product one."""
    k, pad = fam._gru_geo(d)
    B, H, W = shape
    w, plan, launches = fam.impulse_launches("C", 31 + d, (B, fam.GRU_C, H, W), (HID, fam.GRU_C) + k, 1, pad,
                                             **fam.GRU_SCALE, max_launches=5, full=False)
    for x, sites, exp6 in launches:
        three = fam._model_conv(x, w, 1, pad, drop="wm_xm")
        fam._assert_tanh_is_identity(three)
        assert _moved(three, exp6)
        fam._assert_within_one_ulp(_q(x, d, w, "bf16x3"), three)
        fam._assert_within_one_ulp(_q(x, d, w, "bf16"), bx.expected_conv(pm.kept(x, "bf16"), pm.kept(w, "bf16"), 1, pad))


@pytest.mark.gpu
@pytest.mark.parametrize("d", [0, 1])
def test_gru_precision_zero_is_the_old_entry_point(d):
    from eraft_amd import _lib
    from test_gru import _inputs, _to, _weights
    lib = _lib.load()
    B, H, W, inp = 2, 7, 9, 320
    ws, bs = _weights(inp, "12"[d])
    (hg, xg), wg, bg = _to(_inputs(11 + d, B, inp, H, W), DEV, torch.float32), _to(ws, DEV, torch.float32), _to(bs, DEV, torch.float32)
    packed = _lib.gru_pack_weights(*(w.reshape(HID, -1, *fam._gru_geo(d)[0]) for w in wg))
    new = _lib.gru_half_step(hg, xg, d, packed, *bg, precision=0)
    need = lib.corr_gru_workspace(B, HID, H, W)
    wsp, old = torch.empty(need // 4, dtype=torch.float32, device=DEV), torch.empty_like(new)
    torch.cuda.synchronize()
    rc = lib.corr_gru_half_step(hg.data_ptr(), xg.data_ptr(), B, HID, inp, H, W, d, packed.data_ptr(),
                                *(b.data_ptr() for b in bg), wsp.data_ptr(), need, old.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.corr_last_error().decode()
    assert bit_equal(new.cpu().numpy(), old.cpu().numpy())
    for mode in REDUCED:
        assert not bit_equal(_lib.gru_half_step(hg, xg, d, packed, *bg, precision=pm.CODE[mode]).cpu().numpy(),
                             old.cpu().numpy()), mode


# ----------------------------------------------------------------------------------------------
# GPU: the error bound, from the split's definition
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 7, 9), (2, 1, 1)], ids=["7x9", "1x1"])
def test_error_bound(shape):
    """bf16 rounding to nearest is within 2^-9 relative, so |x - hi| <= 2^-9 |x| and
    |x - hi - mid| <= 2^-18 |x|.  A product of the kept pieces misses w x by at most
    (2^-18 + 2^-18 + 2^-18 2^-18) |w x| + |wm xm| (<= 2^-18 |w x|) < 2^-16 |w x| in bf16x3 and by at
    most (2^-9 + 2^-9 + 2^-18) |w x| in bf16, hence for every output

        bf16x3  |out - fp64| <= 2^-16 sum |w| |x| + A
        bf16    |out - fp64| <= (2^-8 + 2^-18) sum |w| |x| + A

    with A = (c + 6 S) 2^-24 (sum |w| |x| + |bias|) the fp32 accumulation allowance of
    test_bf16x6_family.py::test_error_bound for the same K (a reduced mode issues fewer MFMAs, so A
    covers it).  Gaussian inputs, 64 -> 40 channels; at 1x1 every tap but the centre is padding.
    Each mode's error, as max |out - fp64| / (sum |w| |x| + |bias|) over the outputs (the bound's own
    normalisation), must also exceed the next finer mode's tenfold: a mode that silently ran the
    finer arithmetic would show nothing."""
    lin = fam.Lin("conv", 64, 40)
    x, w, bias = fam._bound_inputs("gauss", lin, shape)
    t = lambda a: torch.from_numpy(a).double()
    ref = F.conv2d(t(x), t(w), t(bias), 1, 1).numpy()
    mag = F.conv2d(t(np.abs(x)), t(np.abs(w)), None, 1, 1).numpy()
    scale = mag + np.abs(bias.astype(F64))[None, :, None, None]
    A = (lin.c + 6 * lin.S) * 2.0 ** -24 * scale
    r = {}
    for mode in pm.MODES:
        got = _conv(x, w, mode, bias).astype(F64)
        assert np.isfinite(got).all()
        err, bound = np.abs(got - ref), pm.COEF[mode] * mag + A
        r[mode] = (err / scale).max()
        print(f"bound {mode} {shape}: max |err| / bound = {(err / bound).max():.4f}, "
              f"max |err| / (sum |w||x| + |bias|) = 2^{np.log2(r[mode]):.2f}")
        assert (err <= bound).all(), mode
    print(f"ratios {shape}: bf16x3 / bf16x6 = {r['bf16x3'] / r['bf16x6']:.1f}, bf16 / bf16x3 = {r['bf16'] / r['bf16x3']:.1f}")
    assert r["bf16x3"] >= 10 * r["bf16x6"]
    assert r["bf16"] >= 10 * r["bf16x3"]


# ----------------------------------------------------------------------------------------------
# GPU: the GRU half step against its own definition, launch by launch
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("d", [0, 1])
@pytest.mark.parametrize("B,H,W,inp", [(1, 1, 1, 320), (2, 7, 9, 320), (1, 5, 70, 320), (1, 70, 5, 320), (2, 7, 9, 32)])
def test_half_step_definition(B, H, W, inp, d, mode):
    """z and r*h are read back from the workspace.  The gates launch is compared with the fp64
    evaluation of its formulas on (h, x) with the mode's kept pieces; the candidate launch with that
    of its own on the r*h and z the GPU wrote (its actual fp32 inputs), so a rounding flip of r*h
    does not leak into the tolerance.  Norm-relative, REL_TOL."""
    from eraft_amd import _lib
    from test_gru import _inputs, _weights
    k, pad = fam._gru_geo(d)
    (wz, wr, wq), (bz, br, bq) = _weights(inp, "12"[d])
    wz, wr, wq = (w.reshape((HID, HID + inp) + k) for w in (wz, wr, wq))
    h, x = _inputs(11 + d, B, inp, H, W)
    need = _lib.load().corr_gru_workspace(B, HID, H, W)
    wsp = torch.zeros(need // 4, dtype=torch.float32, device=DEV)
    got = _gru(h, x, d, (wz, wr, wq), (bz, br, bq), mode, workspace=wsp)
    n = B * HID * H * W
    z, rh = (wsp[o:o + n].cpu().numpy().reshape(B, HID, H, W) for o in (0, need // 8))
    hx = np.concatenate([h, x], 1)
    z64 = pm.sigmoid64(pm.conv64(hx, wz, mode, pad, bz))
    rh64 = pm.sigmoid64(pm.conv64(hx, wr, mode, pad, br)) * h.astype(F64)
    q64 = np.tanh(pm.conv64(np.concatenate([rh, x], 1), wq, mode, pad, bq))
    out64 = (1.0 - z.astype(F64)) * h.astype(F64) + z.astype(F64) * q64
    errs = norm_rel(z, z64), norm_rel(rh, rh64), norm_rel(got, out64)
    print(f"gru {mode} B={B} {H}x{W} C={HID + inp} dir={d}: z {errs[0]:.2e}, r*h {errs[1]:.2e}, h' {errs[2]:.2e}")
    assert np.isfinite(got).all()
    assert all(e <= REL_TOL for e in errs)


# ----------------------------------------------------------------------------------------------
# GPU: non-finite inputs
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_non_finite(mode):
    """+inf and NaN activations, no 3x3 window holding both: the non-finite pattern is the fp32 CPU
    convolution's and the remaining outputs are finite."""
    x, w, bias = prng.gauss(121, (1, 32, 6, 7)), prng.gauss(122, (32, 32, 3, 3), 2.0 ** -10), prng.gauss(123, (32,), 0.1)
    x[0, 3, 1, 1], x[0, 30, 4, 5] = np.inf, np.nan
    got = _conv(x, w, mode, bias)
    t = torch.from_numpy
    ref = F.conv2d(t(x), t(w), t(bias), 1, 1).numpy()
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any()
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
    assert np.isfinite(got[np.isfinite(ref)]).all()


# ----------------------------------------------------------------------------------------------
# GPU: determinism and capture
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_deterministic_and_capturable(mode):
    from eraft_amd.gru import sepconv_gru
    from test_gru import _inputs, _module
    m = _module(320, DEV)
    m.precision = mode
    h, x = (torch.from_numpy(a).cuda() for a in _inputs(31, 2, 320, 7, 9))
    with torch.no_grad():
        a = sepconv_gru(m, h, x)  # also the warm-up: the packs are made here, outside the capture
        b = sepconv_gru(m, h, x)
        assert bit_equal(a.cpu().numpy(), b.cpu().numpy())
        torch.cuda.synchronize()
        gph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gph):
            c = sepconv_gru(m, h, x)
        gph.replay()
        torch.cuda.synchronize()
        assert bit_equal(a.cpu().numpy(), c.cpu().numpy())
        m.precision = "bf16x6"
        assert not bit_equal(a.cpu().numpy(), sepconv_gru(m, h, x).cpu().numpy())


# ----------------------------------------------------------------------------------------------
# GPU: the module path
# ----------------------------------------------------------------------------------------------
# The block's norm-relative tolerance per mode.  A stage's operand rounding is at most COEF |w x| per
# product; over the sign-random products of one output these add like a random walk, so a stage's
# norm-relative error stays below COEF (2.4e-3 measured in numpy for bf16 at 64 channels, COEF = 3.9e-3),
# ReLU and tanh are 1-Lipschitz and the sigmoid 1/4-Lipschitz, and at most eight stages follow one
# another (convc2 | convf2, conv, gates, candidate, gates, candidate, the heads, conv2 | mask[2]), whose
# errors add at worst linearly; REL_TOL is the fp32 part, as for the default mode.
BLOCK_TOL = {mode: REL_TOL + 8 * pm.COEF[mode] for mode in pm.MODES}


@pytest.mark.gpu
def test_module_path(monkeypatch):
    from eraft_amd.model import BasicUpdateBlock, SepConvGRU
    from test_conv import _block, _block64, _block_inputs, _run
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(SepConvGRU, "fused", True)
    m = _block(DEV)
    arrs = _block_inputs(7, 1, 6, 7)
    ref = _block64(m, arrs)
    today = _run(m, arrs)
    out = {}
    for mode in pm.MODES:
        m.precision = m.gru.precision = mode
        out[mode] = _run(m, arrs)
        errs = [norm_rel(a, b) for a, b in zip(out[mode], ref)]
        print(f"update block {mode}: net {errs[0]:.2e}, mask {errs[1]:.2e}, delta {errs[2]:.2e} (tol {BLOCK_TOL[mode]:.2e})")
        assert all(np.isfinite(a).all() for a in out[mode])
        assert all(e <= BLOCK_TOL[mode] for e in errs), mode
    assert all(bit_equal(a, b) for a, b in zip(out["bf16x6"], today))
    for mode in REDUCED:
        assert not any(bit_equal(a, b) for a, b in zip(out[mode], today)), mode
    # the GRU follows its own module's mode
    m.precision, m.gru.precision = "bf16x6", "bf16"
    assert not bit_equal(_run(m, arrs)[0], today[0])


# ----------------------------------------------------------------------------------------------
# GPU: end to end against the reference's own mixed precision
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e(key):
    """The four EPEs (cold low-res / full-res, warm low-res / full-res) against the reference's fp32
    golden of a model with config key mixed_precision = `key` (None: absent)."""
    from eraft_amd.model import ERAFT
    from test_e2e import _epe
    g = load("g_e2e_dsec")
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    config = {"subtype": "warm_start"}
    if key is not None:
        config["mixed_precision"] = key
    model = ERAFT(config, n_first_channels=bins).eval()
    model.load_state_dict(_base_state(bins))
    model = model.to(DEV)
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W))).to(DEV)
    finit = torch.from_numpy(g["flow_init"]).to(DEV)
    with torch.no_grad():
        low, ups = model(im1, im2, iters=iters)
        low_w, ups_w = model(im1, im2, iters=iters, flow_init=finit)
    return model.precision, np.array([_epe(low.cpu().numpy(), g["low"]), _epe(ups[-1][..., ::4, ::4].cpu().numpy(), g["up_sub"]),
                                      _epe(low_w.cpu().numpy(), g["low_warm"]),
                                      _epe(ups_w[-1][..., ::4, ::4].cpu().numpy(), g["up_warm_sub"])])


@functools.lru_cache(maxsize=None)
def _base_state(bins):
    from test_e2e import _model
    return copy.deepcopy(_model(bins).state_dict())


@pytest.mark.gpu
@pytest.mark.parametrize("key,mode", [(True, "bf16x3"), ("bf16", "bf16")])
def test_e2e_against_the_references_mixed_precision(monkeypatch, key, mode):
    """The g_e2e_dsec inputs with all four fusion switches on, cold and warm.  mixed_precision=True
    (bf16x3): EPE <= the reference's fp16-autocast EPE / 8 (operands keep at least 16 significant bits
    against fp16's 11, a factor of 32, a quarter of which is left for the twelve recurrent iterations).
    mixed_precision="bf16": EPE <= 1.5 x the reference's bf16-autocast EPE (the autocast rounds more
    than this mode does, the encoders and every activation too; one run of a chaotic amplification is
    one sample, hence the half on top).  Both: strictly above the bf16x6 path's EPE on the same
    inputs."""
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    monkeypatch.delenv("ERAFT_AMD_PRECISION", raising=False)
    monkeypatch.setattr(SepConvGRU, "fused", True)
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", True)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", True)
    fx = load("precision_reference")
    name0, base = _e2e(None)
    name, errs = _e2e(key)
    assert (name0, name) == ("bf16x6", mode)
    yard = fx["autocast_float16"] / 8 if mode == "bf16x3" else 1.5 * fx["autocast_bfloat16"]
    fmt = lambda v: " / ".join(f"{e:.3e}" for e in v)
    print(f"e2e {mode} EPE cold low / up, warm low / up: {fmt(errs)} px; bf16x6 {fmt(base)}; limit {fmt(yard)}; "
          f"emulated {fmt(fx['emu_' + mode])}")
    assert np.isfinite(errs).all()
    assert (errs <= yard).all()
    assert (errs > base).all()
