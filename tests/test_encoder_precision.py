"""The reduced precision modes of the encoders' convolutions (corr_enc_conv_forward_prec,
corr_enc_stem_forward_prec, corr_enc_pw_forward_prec: include/corr_mi355x_enc_prec.h; the config key
`encoder_precision`, eraft_amd/precision.py: resolve_encoder).

CPU: the exports, the refusals (an unknown precision first; every refusal of the old entry points
through the new ones), the resolver and the knob, that the knob is inert off the GPU path, and the
fixture's conditions on its own emulated numbers.  GPU, per kind and reduced mode: which products a
mode keeps, bit for bit, with tests/test_bf16x6_family.py's method (plain and norm-on-load forms);
precision 0 against the old entry points; the statistics of a launch against its own output; an
a-priori element-wise error bound and the ordering of the modes; the non-finite rule, determinism,
graph capture and the four buffer and stream properties of tests/test_core_discipline.py; the module
path; and the end-to-end flow against the reference's own mixed precision
(tests/golden/encoder_precision_reference.npz, make_golden_encoder_precision.py).
"""
import copy
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bf16x6 as bx
import _precision as pm
import prng
import test_bf16x6_family as fam
from _util import REL_TOL, bit_equal, load, norm_rel
from test_core_discipline import Arena, _clones, _ok, _ordered_on_the_callers_stream, _run_case, _same, _stream
from test_core_discipline import gpu, side  # noqa: F401  (fixtures)

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
EINVAL, EUNSUPPORTED = -1, -2
EPS = 1e-5
REDUCED = ("bf16x3", "bf16")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "corr_mi355x_enc_prec.h")
NEW = ("corr_enc_conv_forward_prec", "corr_enc_stem_forward_prec", "corr_enc_pw_forward_prec")
KINDS = ("enc_conv", "stem", "pw")

# tests/test_bf16x6_family.py's cases of the three kinds: enc_conv 64 -> 96 at stride 1 (EDGE) and 2
# (EDGE2) and 32 -> 1; stem 15 -> 64 (EDGE2) and 16 -> 1; pw 64 -> 96 at stride 1 and 2 and 32 -> 1
CASES = [c for c in fam.CASES if c.values[0].kind in KINDS]
FIRST = [c for c in fam.FIRST if c.values[0].kind in KINDS]
assert len(CASES) == 18 and len(FIRST) == 8


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


def _bind(lin, w, mode):
    """Packs w once; returns run(x, bias=None, norm=None, stats=False) -> numpy out (or (out, stats
    tensor)) of the kind's kernel in `mode`, through the new entry point."""
    from eraft_amd import _lib
    wg = _gpu(w)
    packed = {"enc_conv": _lib.conv_pack_weights, "stem": _lib.enc_stem_pack_weights,
              "pw": _lib.enc_pw_pack_weights}[lin.kind](wg)

    def run(x, bias=None, norm=None, stats=False):
        bg, xg, p = _gpu(np.zeros(lin.cout, F32) if bias is None else bias), _gpu(x), pm.CODE[mode]
        if lin.kind == "enc_conv":
            sc, sh = (None, None) if norm is None else (_gpu(norm[0]), _gpu(norm[1]))
            out = _lib.enc_conv_forward(xg, packed, bg, lin.cout, lin.stride, sc, sh, stats=stats, precision=p)
        elif lin.kind == "stem":
            out = _lib.enc_stem_forward(xg, packed, bg, lin.cout, stats=stats, precision=p)
        else:
            out = _lib.enc_pw_forward(xg, packed, bg, lin.cout, lin.stride, stats=stats, precision=p)
        return (out[0].cpu().numpy(), out[1]) if stats else out.cpu().numpy()
    return run


# ----------------------------------------------------------------------------------------------
# CPU: exports and refusals
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(re.findall(r"\b(corr_\w+)\s*\(", src))


def test_exports(lib):
    from eraft_amd import _lib
    assert sorted(_lib.ENC_PREC_EXPORTS) == _declared() == sorted(NEW)
    assert not set(_lib.ENC_PREC_EXPORTS) & (set(_lib.EXPORTS) | set(_lib.TRAIN_EXPORTS))
    for name in _lib.ENC_PREC_EXPORTS:
        assert hasattr(lib, name), name
    assert lib.corr_version() == 202


# good arguments (fake pointers, never dereferenced: every call below is refused before any HIP call)
_CONV = dict(inp=0x10000000, cin=64, B=2, H=6, W=7, stride=2, in_scale=0x20000000, in_shift=0x21000000,
             norm_per_batch=1, packed=0x30000000, bias=0x40000000, cout=96, out=0x50000000, stats=0x60000000,
             stats_bytes=1 << 20, precision=0, stream=None)
_STEM = dict(inp=0x10000000, cin=15, B=2, H=6, W=7, packed=0x30000000, bias=0x40000000, cout=64, out=0x50000000,
             stats=0x60000000, stats_bytes=1 << 20, precision=0, stream=None)
_PW = dict(inp=0x10000000, cin=64, B=2, H=6, W=7, stride=2, packed=0x30000000, bias=0x40000000, cout=96,
           out=0x50000000, stats=0x60000000, stats_bytes=1 << 20, precision=0, stream=None)
_GOOD = dict(zip(NEW, (_CONV, _STEM, _PW)))
# one broken argument each (what the old entry points refuse: tests/test_encoder.py, test_encoder_front.py)
_BROKEN = {
    NEW[0]: [{"B": 0}, {"H": 0}, {"W": -1}, {"stride": 3}, {"stride": 0}, {"cin": 33}, {"cin": 0}, {"cout": 0},
             {"cout": 1025}, {"inp": None}, {"packed": None}, {"out": None}, {"in_shift": None}, {"in_scale": None},
             {"stats_bytes": 8}, {"packed": 0x30000004}, {"out": 0x10000000}, {"B": 1 << 20, "H": 1 << 10, "W": 1 << 10}],
    NEW[1]: [{"B": 0}, {"H": 0}, {"cin": 0}, {"cin": 17}, {"cout": 0}, {"cout": 1025}, {"inp": None}, {"packed": None},
             {"out": None}, {"stats_bytes": 8}, {"packed": 0x30000008}, {"out": 0x10000000}],
    NEW[2]: [{"B": 0}, {"W": 0}, {"stride": 3}, {"cin": 48}, {"cin": 2048}, {"cout": 0}, {"inp": None}, {"packed": None},
             {"out": None}, {"stats_bytes": 8}, {"packed": 0x30000004}, {"out": 0x10000000}],
}


@pytest.mark.parametrize("fn", NEW)
def test_refusals(lib, fn):
    """An unknown precision is CORR_EINVAL before anything else, with otherwise valid and with
    otherwise invalid arguments; 0, 1, 2 get past that check; and every refusal of the old entry
    point comes back through the new one, in every mode, with the same status and message."""
    call, old, good = getattr(lib, fn), getattr(lib, fn[:-len("_prec")]), _GOOD[fn]
    for bad in (-1, 3):
        for other in [{}] + _BROKEN[fn]:
            assert call(*dict(good, precision=bad, **other).values()) == EINVAL
            msg = lib.corr_last_error().decode()
            assert fn in msg and "precision" in msg and str(bad) in msg, msg
    for other in _BROKEN[fn]:
        args = dict(good, **other)
        del args["precision"]
        rc0 = old(*args.values())
        msg0 = lib.corr_last_error().decode()
        assert rc0 in (EINVAL, EUNSUPPORTED) and fn[:-len("_prec")] in msg0, (other, rc0, msg0)
        for ok in (0, 1, 2):
            assert call(*dict(good, precision=ok, **other).values()) == rc0, (other, ok)
            msg = lib.corr_last_error().decode()
            assert "precision" not in msg and msg.replace(fn, fn[:-len("_prec")]) == msg0, (other, msg, msg0)


# ----------------------------------------------------------------------------------------------
# CPU: the resolver and the knob
# ----------------------------------------------------------------------------------------------
def _eraft(config=None, bins=3):
    from eraft_amd.model import ERAFT
    return ERAFT(dict({"subtype": "standard"}, **(config or {})), n_first_channels=bins).eval()


def test_resolver(monkeypatch):
    from eraft_amd import precision
    monkeypatch.delenv("ERAFT_AMD_PRECISION", raising=False)
    monkeypatch.delenv("ERAFT_AMD_ENCODER_PRECISION", raising=False)
    r = precision.resolve_encoder
    assert r(None) == r({}) == r({"encoder_precision": None}) == r({"encoder_precision": False}) == "bf16x6"
    assert r({"encoder_precision": True}) == "bf16x3"
    for name in pm.MODES:
        assert r({"encoder_precision": name}) == r({"encoder_precision": name.upper()}) == name
    for bad in ("float16", "fp16", 2, 0.5, ("bf16",)):
        with pytest.raises(ValueError):
            r({"encoder_precision": bad})
    # each knob reads its own key and its own variable
    assert r({"mixed_precision": True}) == "bf16x6" and precision.resolve({"encoder_precision": True}) == "bf16x6"
    monkeypatch.setenv("ERAFT_AMD_PRECISION", "bf16")
    assert r({}) == "bf16x6" and precision.resolve({}) == "bf16"
    monkeypatch.delenv("ERAFT_AMD_PRECISION")
    monkeypatch.setenv("ERAFT_AMD_ENCODER_PRECISION", "bf16")
    assert r({}) == r({"encoder_precision": True}) == r({"encoder_precision": "bf16x6"}) == "bf16"
    assert precision.resolve({}) == "bf16x6"
    monkeypatch.setenv("ERAFT_AMD_ENCODER_PRECISION", "BF16X3")
    assert r({}) == "bf16x3"
    monkeypatch.setenv("ERAFT_AMD_ENCODER_PRECISION", "half")
    with pytest.raises(ValueError):
        r({})
    monkeypatch.setenv("ERAFT_AMD_ENCODER_PRECISION", "")   # set but empty: as unset
    assert r({}) == "bf16x6" and r({"encoder_precision": True}) == "bf16x3"


def test_config_key_and_environment(monkeypatch):
    from eraft_amd.model import ERAFT, BasicEncoder
    monkeypatch.delenv("ERAFT_AMD_PRECISION", raising=False)
    monkeypatch.delenv("ERAFT_AMD_ENCODER_PRECISION", raising=False)
    assert ERAFT.encoder_precision == BasicEncoder.precision == "bf16x6"
    assert "precision" not in vars(BasicEncoder())

    def modes(m):
        assert m.fnet.precision == m.cnet.precision == m.encoder_precision
        assert m.update_block.precision == m.update_block.gru.precision == m.precision
        return m.precision, m.encoder_precision

    for config, want in (({}, ("bf16x6", "bf16x6")), ({"encoder_precision": None}, ("bf16x6", "bf16x6")),
                         ({"encoder_precision": True}, ("bf16x6", "bf16x3")),
                         ({"encoder_precision": "bf16"}, ("bf16x6", "bf16")),
                         ({"mixed_precision": True}, ("bf16x3", "bf16x6")),
                         ({"mixed_precision": "bf16"}, ("bf16", "bf16x6")),
                         ({"mixed_precision": True, "encoder_precision": "bf16"}, ("bf16x3", "bf16"))):
        assert modes(_eraft(config)) == want, config
    with pytest.raises(ValueError):
        _eraft({"encoder_precision": "fp16"})
    monkeypatch.setenv("ERAFT_AMD_ENCODER_PRECISION", "bf16")
    assert modes(_eraft({})) == modes(_eraft({"encoder_precision": "bf16x6"})) == ("bf16x6", "bf16")
    assert modes(_eraft({"mixed_precision": True})) == ("bf16x3", "bf16")
    monkeypatch.setenv("ERAFT_AMD_ENCODER_PRECISION", "half")
    with pytest.raises(ValueError):
        _eraft({})
    monkeypatch.setenv("ERAFT_AMD_ENCODER_PRECISION", "")
    assert modes(_eraft({"encoder_precision": True})) == ("bf16x6", "bf16x3")
    monkeypatch.setenv("ERAFT_AMD_PRECISION", "bf16")
    assert modes(_eraft({})) == ("bf16", "bf16x6")


@pytest.mark.parametrize("norm", ["instance", "batch"])
def test_knob_is_inert_off_the_kernel_path(monkeypatch, norm):
    """On CPU tensors with the switch on, and with the switch off, an encoder in a reduced mode is
    the torch code: bit-identical to the default mode."""
    from eraft_amd.model import BasicEncoder
    from test_encoder import _encoder, _run
    m, x = _encoder(norm, 3), prng.gauss(5, (2, 3, 32, 40))
    assert BasicEncoder.precision == m.precision == "bf16x6"  # the knob exists and is off
    for fused in (True, False):
        monkeypatch.setattr(BasicEncoder, "fused", fused)
        base = _run(m, x, "cpu")
        for mode in REDUCED:
            r = copy.deepcopy(m)
            r.precision = mode
            assert bit_equal(_run(r, x, "cpu"), base), (fused, mode)


def test_fixture_conditions():
    """The margins that the end-to-end test applies hold on the fixture's own emulated EPEs (cold and
    warm, low-res and full-res), and the fixture is the issue's table."""
    g, yard = load("encoder_precision_reference"), load("precision_reference")
    bar = {"bf16x3": yard["autocast_float16"] / 8, "bf16": 1.5 * yard["autocast_bfloat16"]}
    for mode in REDUCED:
        enc, both = g[f"emu_enc_{mode}"], g[f"emu_all_{mode}"]
        for v in (enc, both):
            assert v.shape == (4,) and np.isfinite(v).all() and (v > 0).all()
            assert (v <= bar[mode]).all(), mode
        assert (both >= enc).all(), mode
    for tag in ("enc", "all"):
        assert (g[f"emu_{tag}_bf16x3"] < g[f"emu_{tag}_bf16"] / 100).all(), tag
    assert list(g["meta"]) == list(load("g_e2e_dsec")["meta"])
    assert len(g["convs"]) == len(set(g["convs"])) == 32
    assert sum(n.startswith("fnet.") for n in g["convs"]) == sum(n.startswith("cnet.") for n in g["convs"]) == 16
    assert g["fp32"].shape == (4,) and g["fp32"].max() < 1e-3
    assert np.allclose(g["emu_enc_bf16x3"], [1.98e-3, 6.97e-3, 1.39e-3, 5.45e-3], rtol=5e-3)
    assert np.allclose(g["emu_enc_bf16"], [0.564, 1.813, 0.459, 1.633], atol=1e-3)
    assert np.allclose(g["emu_all_bf16x3"], [2.85e-3, 9.86e-3, 2.06e-3, 8.02e-3], rtol=5e-3)
    assert np.allclose(g["emu_all_bf16"], [0.796, 2.615, 0.701, 2.503], atol=1e-3)


# ----------------------------------------------------------------------------------------------
# GPU: which products each mode keeps, bit for bit
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("lin,shape", CASES)
def test_weight_pieces(lin, shape, mode):
    """Class A weights against impulses +-2^e: the output is the product with the weight's lo piece
    (bf16x3), or its mid and lo pieces (bf16), removed, exactly; every (cout, cin, tap) is observed."""
    xs, ws = fam._lin_shapes(lin, shape)
    w, plan, launches = fam.impulse_launches("A", fam._seed(lin, shape), xs, ws, lin.stride, lin.pad)
    run, wk, seen = _bind(lin, w, mode), pm.kept(w, mode), np.zeros(ws, bool)
    for x, sites, exp6 in launches:
        bx.observe(plan, sites, exp6, seen)
        exp = bx.expected_conv(x, wk, lin.stride, lin.pad)
        assert not bit_equal(exp, exp6)
        assert bit_equal(run(x), exp)
    assert seen.all()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("lin,shape", CASES)
def test_activation_pieces(lin, shape, mode):
    """Class B activations under one-hot weights +-2^e: the same on the activation's side."""
    xs, ws = fam._lin_shapes(lin, shape)
    x, launches = fam.onehot_launches(fam._seed(lin, shape) + 1, xs, ws, lin.stride, lin.pad)
    fam._assert_onehot_coverage(launches, ws)
    xk = pm.kept(x, mode)
    for w, exp6 in launches:
        exp = bx.expected_conv(xk, w, lin.stride, lin.pad)
        assert not bit_equal(exp, exp6)
        assert bit_equal(_bind(lin, w, mode)(x), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("lin,shape", FIRST)
def test_cross_terms(lin, shape):
    """Class C in both operands: bf16x3 is the three-product sum (six() without wm xm), not the
    four-product one; bf16 is wh xh; precision 0 is the six products."""
    xs, ws = fam._lin_shapes(lin, shape)
    w, plan, launches = fam.impulse_launches("C", fam._seed(lin, shape) + 2, xs, ws, lin.stride, lin.pad,
                                             max_launches=min(lin.k * lin.k, 9), full=False)
    runs = {mode: _bind(lin, w, mode) for mode in pm.MODES}
    for x, sites, exp6 in launches:
        three = fam._model_conv(x, w, lin.stride, lin.pad, drop="wm_xm")
        one = bx.expected_conv(pm.kept(x, "bf16"), pm.kept(w, "bf16"), lin.stride, lin.pad)
        assert np.count_nonzero(exp6) >= lin.cout and not bit_equal(three, exp6) and not bit_equal(one, three)
        assert bit_equal(runs["bf16x3"](x), three)
        assert bit_equal(runs["bf16"](x), one)
        assert bit_equal(runs["bf16x6"](x), exp6)


def _pow2_norm(seed, B, cin, per_batch):
    """(scale, shift): per-channel scales +-2^k, k in -3 .. 3, both signs, and shift 0: the norm on
    load relu(x * scale) is exact, and it zeroes the values whose sign is not the scale's."""
    rng = np.random.default_rng(seed)
    shape = (B, cin) if per_batch else (cin,)
    scale = (np.ldexp(1.0, rng.integers(-3, 4, shape)) * rng.choice([-1.0, 1.0], shape)).astype(F32)
    assert (scale > 0).any() and (scale < 0).any()
    return scale, np.zeros(shape, F32)


def _normalised(x, scale):
    v = scale[:, :, None, None] if scale.ndim == 2 else scale[None, :, None, None]
    out = np.maximum(x * v, F32(0)).astype(F32)
    assert (out.astype(F64) == np.maximum(x.astype(F64) * v, 0)).all()
    return out + F32(0)  # (-0 -> +0)


NORM_CASES = [c for c in FIRST if c.values[0].kind == "enc_conv"]  # 64 -> 96 at stride 1 and 2, 32 -> 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("lin,shape", NORM_CASES)
def test_norm_on_load_pieces(lin, shape, mode):
    """The NORM_IN forms: power-of-two scales of both signs and shift 0, so the normalised input is
    known exactly and half of it is zero.  Weight pieces (class A against impulses), activation
    pieces (class B under one-hot weights) and the cross term (class C), each bit-equal to the
    expectation on the normalised input's kept pieces, with a [B, C] and with a [C] table."""
    xs, ws = fam._lin_shapes(lin, shape)
    for per_batch in (True, False):
        scale, shift = _pow2_norm(7 + per_batch, xs[0], lin.cin, per_batch)
        w, plan, launches = fam.impulse_launches("A", fam._seed(lin, shape), xs, ws, lin.stride, lin.pad,
                                                 max_launches=9, full=False)
        run, wk, hit = _bind(lin, w, mode), pm.kept(w, mode), 0
        for x, sites, _ in launches:
            xn = _normalised(x, scale)
            exp, exp6 = bx.expected_conv(xn, wk, lin.stride, lin.pad), bx.expected_conv(xn, w, lin.stride, lin.pad)
            hit += np.count_nonzero(exp)
            assert not bit_equal(exp, exp6) and 0 < np.count_nonzero(xn) < np.count_nonzero(x)
            assert bit_equal(run(x, norm=(scale, shift)), exp)
        assert hit >= lin.cout
        x, launches = fam.onehot_launches(fam._seed(lin, shape) + 1, xs, ws, lin.stride, lin.pad)
        xn = _normalised(x, scale)
        assert 0.25 < np.count_nonzero(xn) / xn.size < 0.75
        for w1, _ in launches:
            exp = bx.expected_conv(pm.kept(xn, mode), w1, lin.stride, lin.pad)
            assert not bit_equal(exp, bx.expected_conv(xn, w1, lin.stride, lin.pad))
            assert bit_equal(_bind(lin, w1, mode)(x, norm=(scale, shift)), exp)
    w, plan, launches = fam.impulse_launches("C", fam._seed(lin, shape) + 2, xs, ws, lin.stride, lin.pad,
                                             max_launches=3, full=False)
    run = _bind(lin, w, mode)
    for x, sites, _ in launches:
        xn = _normalised(x, scale)
        exp = (fam._model_conv(xn, w, lin.stride, lin.pad, drop="wm_xm") if mode == "bf16x3" else
               bx.expected_conv(pm.kept(xn, mode), pm.kept(w, mode), lin.stride, lin.pad))
        assert not bit_equal(exp, fam._model_conv(xn, w, lin.stride, lin.pad))
        assert bit_equal(run(x, norm=(scale, shift)), exp)


# ----------------------------------------------------------------------------------------------
# GPU: precision 0, the statistics, the error bound
# ----------------------------------------------------------------------------------------------
def _gauss_case(lin, shape):
    xs, ws = fam._lin_shapes(lin, shape)
    return prng.gauss(111, xs), prng.gauss(112, ws, 0.1), prng.gauss(113, (lin.cout,), 0.1)


@pytest.mark.gpu
@pytest.mark.parametrize("lin,shape", FIRST)
def test_precision_zero_is_the_old_entry_point(lin, shape):
    """Through the new entry point, precision 0 gives the bits of the old one (output and
    statistics; the norm-on-load form too), and both reduced modes differ from it."""
    from eraft_amd import _lib
    lib = _lib.load()
    x, w, bias = _gauss_case(lin, shape)
    B, cin, H, W = x.shape
    norms = [None] + ([(1.0 + 0.5 * prng.gauss(5, (B, cin)), 0.5 + np.abs(prng.gauss(6, (B, cin))))]
                      if lin.kind == "enc_conv" else [])
    for norm in norms:
        new, st = _bind(lin, w, "bf16x6")(x, bias, norm, stats=True)
        xg, bg = _gpu(x), _gpu(bias)
        packed = {"enc_conv": _lib.conv_pack_weights, "stem": _lib.enc_stem_pack_weights,
                  "pw": _lib.enc_pw_pack_weights}[lin.kind](_gpu(w))
        old, st_old = torch.empty(new.shape, device=DEV), torch.zeros_like(st)
        tail = (packed.data_ptr(), bg.data_ptr(), lin.cout, old.data_ptr(), st_old.data_ptr(), st_old.numel() * 4, None)
        torch.cuda.synchronize()
        if lin.kind == "enc_conv":
            sc, sh = (None, None) if norm is None else (_gpu(norm[0]), _gpu(norm[1]))
            rc = lib.corr_enc_conv_forward(xg.data_ptr(), cin, B, H, W, lin.stride, sc if sc is None else sc.data_ptr(),
                                           sh if sh is None else sh.data_ptr(), 1, *tail)
        elif lin.kind == "stem":
            rc = lib.corr_enc_stem_forward(xg.data_ptr(), cin, B, H, W, *tail)
        else:
            rc = lib.corr_enc_pw_forward(xg.data_ptr(), cin, B, H, W, lin.stride, *tail)
        torch.cuda.synchronize()
        assert rc == 0, lib.corr_last_error().decode()
        assert bit_equal(new, old.cpu().numpy()) and torch.equal(st.view(torch.int32), st_old.view(torch.int32))
        for mode in REDUCED:
            assert not bit_equal(_bind(lin, w, mode)(x, bias, norm), new), mode


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("lin,shape", [c for c in FIRST if c.values[0].cout > 1])
def test_statistics(lin, shape, mode):
    """The STATS forms: the launch's statistics through enc_norm_finalize give the instance norm of
    that launch's own output (tests/test_encoder.py::test_statistics' bar), and the output is the
    plain form's, bit for bit.  enc_conv also in its NORM_IN + STATS form."""
    from eraft_amd import _lib
    from test_encoder import _normalised as normalised
    x, w, bias = _gauss_case(lin, shape)
    B, cin = x.shape[:2]
    norms = [None] + ([(1.0 + 0.5 * prng.gauss(5, (B, cin)), 0.5 + np.abs(prng.gauss(6, (B, cin))))]
                      if lin.kind == "enc_conv" else [])
    run = _bind(lin, w, mode)
    for norm in norms:
        y, st = run(x, bias, norm, stats=True)
        assert bit_equal(y, run(x, bias, norm))
        scale, shift = _lib.enc_norm_finalize(st, B, lin.cout, y.shape[2], y.shape[3], EPS)
        e = norm_rel(*normalised(y, scale.cpu().numpy(), shift.cpu().numpy()))
        print(f"statistics {lin!r} {shape} {mode} norm_in={norm is not None}: {e:.2e}")
        assert e <= REL_TOL


BOUND_CASES = [c for c in FIRST if c.values[0].cout > 1]  # per kind: stride 1 and stride 2 (the stem: 2 only)


@pytest.mark.gpu
@pytest.mark.parametrize("lin,shape", BOUND_CASES)
def test_error_bound(lin, shape):
    """tests/test_precision.py::test_error_bound for the encoder kinds: element-wise

        |out - fp64| <= (c + 6 S) 2^-24 (sum |w| |x| + |bias|) + COEF[mode] sum |w| |x|

    (the allowance of test_bf16x6_family.py::test_error_bound for the same K, plus the operand
    rounding of the kept pieces), and each mode's max |err| / (sum |w| |x| + |bias|) exceeds the
    next finer one's tenfold: a mode that silently ran the finer arithmetic would show nothing."""
    x, w, bias = fam._bound_inputs("gauss", lin, shape)
    t = lambda a: torch.from_numpy(a).double()
    ref = F.conv2d(t(x), t(w), t(bias), lin.stride, lin.pad).numpy()
    mag = F.conv2d(t(np.abs(x)), t(np.abs(w)), None, lin.stride, lin.pad).numpy()
    scale = mag + np.abs(bias.astype(F64))[None, :, None, None]
    A = (lin.c + 6 * lin.S) * 2.0 ** -24 * scale
    r = {}
    for mode in pm.MODES:
        got = _bind(lin, w, mode)(x, bias).astype(F64)
        assert np.isfinite(got).all()
        err, bound = np.abs(got - ref), pm.COEF[mode] * mag + A
        r[mode] = (err / scale).max()
        print(f"bound {lin!r} {shape} {mode}: max |err| / bound = {(err / bound).max():.4f}, "
              f"max |err| / (sum |w||x| + |bias|) = 2^{np.log2(r[mode]):.2f}")
        assert (err <= bound).all(), mode
    print(f"ratios {lin!r}: bf16x3 / bf16x6 = {r['bf16x3'] / r['bf16x6']:.1f}, bf16 / bf16x3 = {r['bf16'] / r['bf16x3']:.1f}")
    assert r["bf16x3"] >= 10 * r["bf16x6"]
    assert r["bf16"] >= 10 * r["bf16x3"]


# ----------------------------------------------------------------------------------------------
# GPU: non-finite inputs, determinism, capture
# ----------------------------------------------------------------------------------------------
ROBUST = [fam.Lin("enc_conv", 64, 96), fam.Lin("enc_conv", 64, 96, stride=2), fam.Lin("stem", 15, 64, stride=2),
          fam.Lin("pw", 64, 96), fam.Lin("pw", 64, 96, stride=2)]


def _robust_shape(lin):
    return fam.EDGE[0] if lin.stride == 1 else fam.EDGE2[0]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("lin", ROBUST, ids=repr)
def test_non_finite(lin, mode):
    """+-inf and NaN activations, no window holding two of them: the non-finite pattern is the fp32
    CPU convolution's (and so the default mode's) and the remaining outputs are finite."""
    xs, ws = fam._lin_shapes(lin, _robust_shape(lin))
    x, w, bias = prng.gauss(121, xs), prng.gauss(122, ws, 2.0 ** -10), prng.gauss(123, (lin.cout,), 0.1)
    x[0, 3, 0, 0], x[0, lin.cin - 2, 4, 8], x[1, 5, 6, 2] = np.inf, np.nan, -np.inf
    t = torch.from_numpy
    ref = F.conv2d(t(x), t(w), t(bias), lin.stride, lin.pad).numpy()
    assert np.isnan(ref).any() and np.isinf(ref).any() and np.isfinite(ref).any()
    for m in (mode, "bf16x6"):
        got = _bind(lin, w, m)(x, bias)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), m
        assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)]), m
        assert np.isfinite(got[np.isfinite(ref)]).all(), m


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
@pytest.mark.parametrize("lin", ROBUST, ids=repr)
def test_deterministic_and_capturable(lin, mode):
    """Two runs are bit-identical (output and statistics), and a captured graph replays to the same
    bits.  The pack is made before the capture."""
    from eraft_amd import _lib
    xs, ws = fam._lin_shapes(lin, _robust_shape(lin))
    xg, bg = _gpu(prng.gauss(131, xs)), _gpu(prng.gauss(133, (lin.cout,), 0.1))
    wg, p = _gpu(prng.gauss(132, ws, 0.1)), pm.CODE[mode]
    if lin.kind == "enc_conv":
        packed = _lib.conv_pack_weights(wg)
        sc, sh = _gpu(1.0 + 0.5 * prng.gauss(5, (lin.cin,))), _gpu(0.5 + np.abs(prng.gauss(6, (lin.cin,))))
        call = lambda: _lib.enc_conv_forward(xg, packed, bg, lin.cout, lin.stride, sc, sh, stats=True, precision=p)
    elif lin.kind == "stem":
        packed = _lib.enc_stem_pack_weights(wg)
        call = lambda: _lib.enc_stem_forward(xg, packed, bg, lin.cout, stats=True, precision=p)
    else:
        packed = _lib.enc_pw_pack_weights(wg)
        call = lambda: _lib.enc_pw_forward(xg, packed, bg, lin.cout, lin.stride, stats=True, precision=p)
    bits = lambda r: [t.cpu().view(torch.int32).numpy().copy() for t in r]
    a, b = bits(call()), bits(call())
    assert all(np.array_equal(u, v) for u, v in zip(a, b))
    torch.cuda.synchronize()
    gph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gph):
        c = call()
    for t in c:
        t.zero_()
    gph.replay()
    torch.cuda.synchronize()
    assert all(np.array_equal(u, v) for u, v in zip(a, bits(c)))


# ----------------------------------------------------------------------------------------------
# GPU: buffer and stream discipline (tests/test_core_discipline.py's four properties)
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _disc_data(kind, stride):
    from eraft_amd import _lib
    lin = fam.Lin(kind, 15 if kind == "stem" else 64, 96 if kind != "stem" else 64, stride=stride)
    B, H, W = (2, 7, 9) if stride == 1 else (2, 13, 17)
    xs, ws = fam._lin_shapes(lin, (B, H, W))
    pack = {"enc_conv": _lib.conv_pack_weights, "stem": _lib.enc_stem_pack_weights,
            "pw": _lib.enc_pw_pack_weights}[kind](_gpu(prng.gauss(142, ws, 0.1)))
    torch.cuda.synchronize()
    return (lin, _gpu(prng.gauss(141, xs)), pack, _gpu(prng.gauss(143, (lin.cout,), 0.1)),
            _gpu(1.0 + 0.5 * prng.gauss(5, (B, lin.cin))), _gpu(0.5 + np.abs(prng.gauss(6, (B, lin.cin)))))


def _disc_case(A, kind, stride, precision):
    """The raw new entry point of `kind` with statistics (enc_conv: with the norm on load too)."""
    from eraft_amd import _lib
    lib = _lib.load()
    lin, x, pack, bias, sc, sh = _disc_data(kind, stride)
    B, cin, H, W = x.shape
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    x, pack, bias = A.inp("in", x), A.inp("packed", pack, align16=True), A.inp("bias", bias)
    if kind == "enc_conv":
        sc, sh = A.inp("in_scale", sc), A.inp("in_shift", sh)
    out = A.out("out", (B, lin.cout, Ho, Wo))
    nst = lib.corr_enc_stats_bytes(B, lin.cout, Ho, Wo)
    st = A.out("stats", (nst // 4,))

    def call():
        tail = (pack.data_ptr(), bias.data_ptr(), lin.cout, out.data_ptr(), st.data_ptr(), nst, precision, _stream())
        if kind == "enc_conv":
            _ok(lib.corr_enc_conv_forward_prec(x.data_ptr(), cin, B, H, W, stride, sc.data_ptr(), sh.data_ptr(), 1, *tail))
        elif kind == "stem":
            _ok(lib.corr_enc_stem_forward_prec(x.data_ptr(), cin, B, H, W, *tail))
        else:
            _ok(lib.corr_enc_pw_forward_prec(x.data_ptr(), cin, B, H, W, stride, *tail))
    return call, _clones(out=out, stats=st)


DISC = {f"corr_enc_{k if k != 'enc_conv' else 'conv'}_forward_prec[s{s}-{m}]": functools.partial(
            _disc_case, kind=k, stride=s, precision=pm.CODE[m])
        for k, s in (("enc_conv", 1), ("enc_conv", 2), ("stem", 2), ("pw", 1), ("pw", 2)) for m in REDUCED}
_DISC_PLAIN = {}


def _disc_plain(name):
    if name not in _DISC_PLAIN:
        _DISC_PLAIN[name] = {k: v.cpu() for k, v in _run_case(DISC[name], Arena()).items()}
    return _DISC_PLAIN[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISC))
def test_buffer_discipline(gpu, name):
    """Properties 1 to 3: writes stay inside guarded windows and every output and statistics word is
    written (the statistics buffer holds exactly corr_enc_stats_bytes); NaN before and after every
    input, aligned to 16 bytes and to 4 only, changes nothing and never reaches a result."""
    arena = Arena(guard_out=True, guard_ws=True)
    got = _run_case(DISC[name], arena)
    arena.check()
    _same(_disc_plain(name), got, name)
    for misalign in (False, True):
        arena = Arena(guard_in=True, misalign=misalign)
        got = _run_case(DISC[name], arena)
        arena.check()
        _same(_disc_plain(name), got, name, clean=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISC))
def test_work_is_ordered_on_the_callers_stream(gpu, side, name):
    """Property 4: the inputs get their values on a side stream behind a long producer."""
    _ordered_on_the_callers_stream(DISC[name], _disc_plain(name), side, name)


# ----------------------------------------------------------------------------------------------
# GPU: the module path
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("norm,shape", [("instance", (2, 3, 64, 96)), ("batch", (1, 3, 64, 96))])
def test_module_path(monkeypatch, norm, shape):
    """encoder_forward on BasicEncoder against the fp64 module, norm-relative.  The default is
    today's fused path bit for bit; bf16x3 <= REL_TOL; bf16 <= 1.5 x the error of torch's own
    autocast("cpu", bfloat16) of the same module on the same input (that autocast rounds every
    operand to bf16 as this mode does, and the activations it stores besides; one run is one sample,
    hence the half on top); the errors are ordered, bf16 >= 100 x bf16x3; a piece that
    USE_KERNEL leaves on torch is not touched by the mode."""
    import eraft_amd.encoder as enc
    from eraft_amd.model import BasicEncoder
    from test_encoder import _encoder, _run
    monkeypatch.setattr(BasicEncoder, "fused", True)
    m, x = _encoder(norm, shape[1], DEV), prng.gauss(77, shape)
    cpu = copy.deepcopy(m).cpu()
    ref = _run(copy.deepcopy(cpu).double(), x, "cpu", torch.float64)
    with torch.no_grad(), torch.autocast("cpu", dtype=torch.bfloat16):
        monkeypatch.setattr(BasicEncoder, "fused", False)
        auto = cpu(torch.from_numpy(x)).float().numpy()
        monkeypatch.setattr(BasicEncoder, "fused", True)
    e_auto = norm_rel(auto, ref)
    today = _run(m, x)
    out, err = {}, {}
    for mode in pm.MODES:
        m.precision = mode
        out[mode] = _run(m, x)
        err[mode] = norm_rel(out[mode], ref)
        assert np.isfinite(out[mode]).all()
    print(f"encoder {norm} {shape}: " + ", ".join(f"{k} {v:.2e}" for k, v in err.items()) + f"; cpu bf16 autocast {e_auto:.2e}")
    assert bit_equal(out["bf16x6"], today)
    assert err["bf16x3"] <= REL_TOL
    assert err["bf16"] <= 1.5 * e_auto
    assert err["bf16x6"] < err["bf16x3"] < err["bf16"] and err["bf16"] >= 100 * err["bf16x3"]
    # with every piece on torch the mode changes nothing; with one piece on torch the others still follow it
    # (MIOpen's deterministic solvers, so that two runs of the same torch code can be compared bit for bit)
    monkeypatch.setattr(torch.backends.cudnn, "deterministic", True)
    monkeypatch.setattr(enc, "USE_KERNEL", {k: False for k in enc.USE_KERNEL})
    m.precision = "bf16x6"
    torch_only = _run(m, x)
    m.precision = "bf16"
    assert bit_equal(_run(m, x), torch_only)
    monkeypatch.setattr(enc, "USE_KERNEL", dict({k: True for k in enc.USE_KERNEL}, head=False))
    assert not bit_equal(_run(m, x), torch_only) and not bit_equal(_run(m, x), out["bf16"])


# ----------------------------------------------------------------------------------------------
# GPU: end to end against the reference's own mixed precision
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _e2e(enc_key, key):
    """The four EPEs (cold low-res / full-res, warm low-res / full-res) against the reference's fp32
    golden of a model with config keys encoder_precision = enc_key and mixed_precision = key (None:
    absent)."""
    from eraft_amd.model import ERAFT
    from test_e2e import _epe
    from test_precision import _base_state
    g = load("g_e2e_dsec")
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    config = {"subtype": "warm_start"}
    if key is not None:
        config["mixed_precision"] = key
    if enc_key is not None:
        config["encoder_precision"] = enc_key
    model = ERAFT(config, n_first_channels=bins).eval()
    model.load_state_dict(_base_state(bins))
    model = model.to(DEV)
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W))).to(DEV)
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W))).to(DEV)
    finit = torch.from_numpy(g["flow_init"]).to(DEV)
    with torch.no_grad():
        low, ups = model(im1, im2, iters=iters)
        low_w, ups_w = model(im1, im2, iters=iters, flow_init=finit)
    return (model.precision, model.encoder_precision), np.array(
        [_epe(low.cpu().numpy(), g["low"]), _epe(ups[-1][..., ::4, ::4].cpu().numpy(), g["up_sub"]),
         _epe(low_w.cpu().numpy(), g["low_warm"]), _epe(ups_w[-1][..., ::4, ::4].cpu().numpy(), g["up_warm_sub"])])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", REDUCED)
def test_e2e_against_the_references_mixed_precision(monkeypatch, mode):
    """The g_e2e_dsec inputs with all four fusion switches on, cold and warm, with encoder_precision
    = mode alone and together with mixed_precision = mode: every EPE is within the mode's bar of
    tests/test_precision.py (the reference's fp16-autocast EPE / 8 for bf16x3, 1.5 x its
    bf16-autocast EPE for bf16: those autocast runs include the reference's reduced-precision
    encoders), and strictly above the EPE of the same setting without encoder_precision."""
    from eraft_amd.model import ERAFT, BasicEncoder, BasicUpdateBlock, SepConvGRU
    monkeypatch.delenv("ERAFT_AMD_PRECISION", raising=False)
    monkeypatch.delenv("ERAFT_AMD_ENCODER_PRECISION", raising=False)
    monkeypatch.setattr(SepConvGRU, "fused", True)
    monkeypatch.setattr(BasicUpdateBlock, "fused", True)
    monkeypatch.setattr(BasicEncoder, "fused", True)
    monkeypatch.setattr(ERAFT, "fuse_mask_upsample", True)
    monkeypatch.setattr(ERAFT, "fuse_lookup_conv", True)
    fx, emu = load("precision_reference"), load("encoder_precision_reference")
    yard = fx["autocast_float16"] / 8 if mode == "bf16x3" else 1.5 * fx["autocast_bfloat16"]
    fmt = lambda v: " / ".join(f"{e:.3e}" for e in v)
    for key, tag in ((None, "enc"), (mode, "all")):
        names0, base = _e2e(None, key)
        names, errs = _e2e(mode, key)
        assert names0 == (key or "bf16x6", "bf16x6") and names == (key or "bf16x6", mode)
        print(f"e2e encoder_precision={mode} mixed_precision={key} EPE cold low / up, warm low / up: {fmt(errs)} px; "
              f"without encoder_precision {fmt(base)}; limit {fmt(yard)}; emulated {fmt(emu[f'emu_{tag}_{mode}'])}")
        assert np.isfinite(errs).all()
        assert (errs <= yard).all()
        assert (errs > base).all()
