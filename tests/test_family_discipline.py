"""Buffer and stream discipline of the convolution families (include/corr_mi355x.h): the update
block's 3x3 convolutions in their three precision modes, the encoders' residual stages, stems,
projections and joins, the mask head fused with the upsampling, convf1 and the flow head, the
on-demand lookup fused with convc1, and the pyramid's import and export.

tests/test_core_discipline.py's four properties (writes stay inside; a workspace, here the
statistics buffer, is as large as its size function says and needs no initialisation; results do
not depend on memory outside the inputs, at 16-byte and at 4-byte alignment; the work is ordered
on the caller's stream) for a table of cases of its own, each calling the raw C-ABI function
through ctypes, each result compared bit for bit with the plain call.  The shapes are the ragged
2 x 7 x 9 and the 1 x 1 x 1 of the family files (a 13 x 17 and a 3 x 4 input for the stem).

Channel windows are a role of their own: where an entry point reads channels offset .. offset + 255
of a wider tensor in place, the other channels hold the sentinel in every run, the plain one
included, so a read outside the window puts the sentinel's payload into a result.  Where an entry
point writes a channel window, the other channels start as the sentinel and the number of words
that changed is a result (0 in the plain call, test_the_plain_call_is_anchored).

Bit equality with a wrong plain call proves nothing, so every case's plain result is anchored
once: the bf16x6 forwards to the family files' own fp64 CPU references within REL_TOL, the packs
word for word to the eraft_amd._lib wrappers' packs, the reduced modes to tests/test_precision.py's
element-wise bound, the rest as their anchors say.

The last GPU test runs each module whose packs go through eraft_amd/_cache.py on two streams: the
pack is made on a side stream behind a long producer and used at once from the default stream.
"""
import copy
import functools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _guard
import _precision as pm
import prng
import test_bf16x6_family as fam
import test_conv as tc
import test_core_discipline as core
import test_encoder as te
import test_encoder_front as tfr
import test_flow_tail as tf
import test_mask_upsample as tm
import test_ondemand_conv as toc
from _util import DEV, REL_TOL, bit_equal, norm_rel
from test_core_discipline import Arena, _clones, _ok, _ordered_on_the_callers_stream, _run_case, _same, _stream
from test_core_discipline import gpu, side  # noqa: F401  (fixtures)
from test_core_discipline import GEO, T, _poison, _ptrs

F64 = np.float64
EPS = 1e-5
SEED = 171
PRECS = {"bf16x3": 1, "bf16": 2}
MODE = {None: "bf16x6", 1: "bf16x3", 2: "bf16"}


def _lib():
    from eraft_amd import _lib as m
    return m.load()


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


# ----------------------------------------------------------------------------------------------
# shared data: built once on the default stream, read-only by convention
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _np_weights(kind, cout, cin):
    """(weight, bias) of the family file that owns `kind`, as numpy."""
    if kind == "conv":
        ws, b = tc._weights(cin, cout)
        return np.concatenate(ws), b
    if kind == "enc_conv":
        return te._weights(cin, cout)
    if kind in ("stem", "pw"):
        return tfr._weights(kind, cin, cout)
    if kind == "mask":
        return tm._head(1)
    if kind == "flow_enc":
        return tf._enc_weights(cout)
    assert kind == "flow_head"
    return tf._head_weights()


@functools.lru_cache(maxsize=None)
def _weights(kind, cout, cin):
    """(weight, bias, pack) on the device; the pack is the eraft_amd._lib wrapper's."""
    from eraft_amd import _lib as L
    w, b = _np_weights(kind, cout, cin)
    pack = {"conv": L.conv_pack_weights, "enc_conv": L.conv_pack_weights, "stem": L.enc_stem_pack_weights,
            "pw": L.enc_pw_pack_weights, "mask": L.mask_upsample_pack_weights, "flow_enc": L.flow_enc_pack_weights,
            "flow_head": L.flow_head_pack_weights}[kind]
    wg = _gpu(w)
    p = pack(wg)
    torch.cuda.synchronize()
    return wg, _gpu(b), p


def _windowed(values, channels, offset):
    """`values` [B, C, H, W] at channels offset .. offset + C - 1 of a [B, channels, H, W] tensor
    whose other channels hold the sentinel: the values of a channel-window input."""
    B, C, H, W = values.shape
    t = _poison(torch.empty((B, channels, H, W), device=DEV))
    t[:, offset:offset + C] = values
    return t


def _window_results(buf, **windows):
    """collect() for an output written through channel windows name=(offset, n): each window, and
    the number of words outside all of them that no longer hold the sentinel."""
    keep = torch.ones(buf.shape[1], dtype=torch.bool)
    for off, n in windows.values():
        keep[off:off + n] = False
    rest = keep.nonzero().flatten().to(DEV)

    def collect():
        res = {name: buf[:, off:off + n].clone() for name, (off, n) in windows.items()}
        if rest.numel():
            other = buf.index_select(1, rest)
            res["words_changed_outside"] = (_guard._bits(other) != _guard.SENTINEL).sum().float().reshape(1)
        return res
    return collect


def _out_hw(H, W, stride):
    return (H - 1) // stride + 1, (W - 1) // stride + 1


# ----------------------------------------------------------------------------------------------
# the packs
# ----------------------------------------------------------------------------------------------
PACKS = {"corr_conv_pack_weights": ("conv", "corr_conv_weights_bytes"),
         "corr_enc_stem_pack_weights": ("stem", "corr_enc_stem_weights_bytes"),
         "corr_enc_pw_pack_weights": ("pw", "corr_enc_pw_weights_bytes"),
         "corr_mask_upsample_pack_weights": ("mask", "corr_mask_upsample_weights_bytes"),
         "corr_flow_enc_pack_weights": ("flow_enc", "corr_flow_enc_weights_bytes"),
         "corr_flow_head_pack_weights": ("flow_head", "corr_flow_head_weights_bytes")}


def _pack_args(pack_fn, cout, cin):
    """The size arguments of a pack entry point (between the weight and the pack)."""
    kind = PACKS[pack_fn][0]
    return {"mask": (), "flow_head": (), "flow_enc": (cout,)}.get(kind, (cout, cin))


def case_pack(A, pack_fn, cout, cin):
    """Every word of the pack is written: the rows padded to a multiple of 64 hold zeros."""
    lib = _lib()
    kind, size_fn = PACKS[pack_fn]
    args = _pack_args(pack_fn, cout, cin)
    w = A.inp("w", _weights(kind, cout, cin)[0])
    n = getattr(lib, size_fn)(*args)
    assert n and n % 4 == 0
    pack = A.out("packed", (n // 4,))

    def call():
        _ok(getattr(lib, pack_fn)(w.data_ptr(), *args, pack.data_ptr(), _stream()))
    return call, _clones(packed=pack)


def anchor_pack(res, pack_fn, cout, cin):
    """Word for word the eraft_amd._lib wrapper's pack of the same weights."""
    want = _weights(PACKS[pack_fn][0], cout, cin)[2].cpu()
    assert res["packed"].numel() == want.numel()
    assert torch.equal(res["packed"].view(torch.int32), want.view(torch.int32))


# ----------------------------------------------------------------------------------------------
# corr_conv_forward, corr_conv_forward_prec
# ----------------------------------------------------------------------------------------------
CONV = {"2x7x9": dict(B=2, H=7, W=9, ca=192, cb=64, cout=126, oc=256, off=128, relu=1, bias=True),
        "1x1x1": dict(B=1, H=1, W=1, ca=32, cb=0, cout=1, oc=1, off=0, relu=0, bias=False)}


@functools.lru_cache(maxsize=None)
def _conv_inputs(shape):
    c = CONV[shape]
    x = _gpu(tc._input(SEED, c["B"], c["ca"] + c["cb"], c["H"], c["W"]))
    return x[:, :c["ca"]].contiguous(), x[:, c["ca"]:].contiguous() if c["cb"] else None


def case_conv_forward(A, shape, precision=None):
    """precision None: corr_conv_forward; otherwise corr_conv_forward_prec in that mode.  2x7x9:
    both input pointers, 126 rows (padded to 128 in the pack) into channels 128 .. 253 of 256.
    1x1x1: in_b and bias NULL."""
    lib, c = _lib(), CONV[shape]
    B, H, W, ca, cb, cout, oc, off = (c[k] for k in ("B", "H", "W", "ca", "cb", "cout", "oc", "off"))
    _, bias, pack = _weights("conv", cout, ca + cb)
    a, b = _conv_inputs(shape)
    a = A.inp("in_a", a)
    b = A.inp("in_b", b) if cb else None
    pack = A.inp("packed", pack, align16=True)
    bias = A.inp("bias", bias) if c["bias"] else None
    out = A.out("out", (B, oc, H, W), full=cout == oc)

    def call():
        args = (a.data_ptr(), ca, None if b is None else b.data_ptr(), cb, B, H, W, pack.data_ptr(),
                None if bias is None else bias.data_ptr(), cout, c["relu"], out.data_ptr(), oc, off)
        if precision is None:
            _ok(lib.corr_conv_forward(*args, _stream()))
        else:
            _ok(lib.corr_conv_forward_prec(*args, precision, _stream()))
    return call, _window_results(out, out=(off, cout))


def anchor_conv_forward(res, shape, precision=None):
    """bf16x6: the fp64 convolution of tests/test_conv.py within REL_TOL.  A reduced mode:
    tests/test_precision.py::test_error_bound's element-wise bound (the ReLU does not widen it)."""
    c = CONV[shape]
    cin = c["ca"] + c["cb"]
    w, bias = _np_weights("conv", c["cout"], cin)
    ref = tc._ref64(SEED, c["B"], c["H"], c["W"], c["ca"], c["cb"], c["cout"])
    if not c["bias"]:
        ref = ref - bias.astype(F64)[None, :, None, None]
        bias = np.zeros_like(bias)
    got = res["out"].numpy()
    assert got.shape == ref.shape and np.isfinite(got).all()
    if c["cout"] != c["oc"]:
        assert float(res["words_changed_outside"]) == 0
    if c["relu"]:
        assert (ref > 0).any() and (ref < 0).any()
    act = (lambda v: np.maximum(v, 0.0)) if c["relu"] else (lambda v: v)
    if precision is None:
        e = norm_rel(got, act(ref))
        print(f"conv {shape}: norm_rel {e:.2e}")
        assert e <= REL_TOL
        return
    lin, t = fam.Lin("conv", cin, c["cout"]), lambda v: torch.from_numpy(v).double()
    x = tc._input(SEED, c["B"], cin, c["H"], c["W"])
    mag = F.conv2d(t(np.abs(x)), t(np.abs(w)), None, 1, 1).numpy()
    scale = mag + np.abs(bias.astype(F64))[None, :, None, None]
    bound = pm.COEF[MODE[precision]] * mag + (lin.c + 6 * lin.S) * 2.0 ** -24 * scale
    err = np.abs(got.astype(F64) - act(ref))
    print(f"conv {shape} {MODE[precision]}: max |err| / bound = {(err / bound).max():.4f}")
    assert (err <= bound).all()


# ----------------------------------------------------------------------------------------------
# corr_enc_conv_forward, corr_enc_norm_finalize, corr_enc_join, corr_enc_join_affine
# ----------------------------------------------------------------------------------------------
ENC = {"2x7x9": dict(B=2, cin=64, H=7, W=9, cout=96, norm=True, stats=True),
       "1x1x1": dict(B=1, cin=32, H=1, W=1, cout=1, norm=False, stats=False)}


@functools.lru_cache(maxsize=None)
def _enc_inputs(shape):
    c = ENC[shape]
    x = _gpu(te._input(SEED, c["B"], c["cin"], c["H"], c["W"]))
    sc, sh = (_gpu(v) for v in te._norm(SEED, c["B"], c["cin"], True)) if c["norm"] else (None, None)
    return x, sc, sh


def case_enc_conv(A, shape, stride):
    """2x7x9: 64 -> 96, the per-batch norm on load, statistics (a buffer of exactly
    corr_enc_stats_bytes, every word written).  1x1x1: 32 -> 1, no norm, stats NULL."""
    lib, c = _lib(), ENC[shape]
    B, cin, H, W, cout = (c[k] for k in ("B", "cin", "H", "W", "cout"))
    Ho, Wo = _out_hw(H, W, stride)
    _, bias, pack = _weights("enc_conv", cout, cin)
    x, sc, sh = _enc_inputs(shape)
    x, pack, bias = A.inp("in", x), A.inp("packed", pack, align16=True), A.inp("bias", bias)
    if c["norm"]:
        sc, sh = A.inp("in_scale", sc), A.inp("in_shift", sh)
    out = A.out("out", (B, cout, Ho, Wo))
    sp, sn, st = None, 0, None
    if c["stats"]:
        sp, sn = A.ws("stats", lib.corr_enc_stats_bytes(B, cout, Ho, Wo), full=True)
        st = A.last_ws

    def call():
        _ok(lib.corr_enc_conv_forward(x.data_ptr(), cin, B, H, W, stride, None if sc is None else sc.data_ptr(),
                                      None if sh is None else sh.data_ptr(), 1, pack.data_ptr(), bias.data_ptr(), cout,
                                      out.data_ptr(), sp, sn, _stream()))
    return call, _clones(out=out, **({} if st is None else {"stats": st}))


def _check_statistics(y, stats, B, C):
    """tests/test_encoder.py::test_statistics' bar: the statistics, merged by enc_norm_finalize,
    give the instance norm of the launch's own output."""
    from eraft_amd import _lib as L
    scale, shift = L.enc_norm_finalize(stats.to(DEV), B, C, y.shape[2], y.shape[3], EPS)
    e = norm_rel(*te._normalised(y, scale.cpu().numpy(), shift.cpu().numpy()))
    assert e <= REL_TOL, e


def anchor_enc_conv(res, shape, stride):
    c = ENC[shape]
    ref = te._ref64(SEED, c["B"], c["H"], c["W"], c["cin"], c["cout"], stride, "batch" if c["norm"] else "off")
    got = res["out"].numpy()
    e = norm_rel(got, ref)
    print(f"enc_conv {shape} stride {stride}: norm_rel {e:.2e}")
    assert got.shape == ref.shape and e <= REL_TOL
    if c["stats"]:
        _check_statistics(got, res["stats"], c["B"], c["cout"])


@functools.lru_cache(maxsize=None)
def _enc_stats(which):
    """(y, stats, B, C, Ho, Wo): "stride2", the statistics of the stride-2 case above; "one-pixel",
    Ho * Wo = 1 (tests/test_encoder.py::test_statistics_of_a_single_pixel's case)."""
    from eraft_amd import _lib as L
    if which == "stride2":
        c = ENC["2x7x9"]
        x, sc, sh = _enc_inputs("2x7x9")
        _, bias, pack = _weights("enc_conv", c["cout"], c["cin"])
        y, st = L.enc_conv_forward(x, pack, bias, c["cout"], 2, sc, sh, stats=True)
    else:
        _, bias, pack = _weights("enc_conv", 96, 64)
        y, st = L.enc_conv_forward(_gpu(te._input(95, 2, 64, 2, 2)), pack, torch.zeros_like(bias), 96, 2, stats=True)
    torch.cuda.synchronize()
    return (y, st) + tuple(y.shape)


def case_norm_finalize(A, which):
    lib = _lib()
    _, stats, B, C, Ho, Wo = _enc_stats(which)
    st = A.inp("stats", stats)
    scale, shift = A.out("scale", (B, C)), A.out("shift", (B, C))

    def call():
        _ok(lib.corr_enc_norm_finalize(st.data_ptr(), B, C, Ho, Wo, EPS, scale.data_ptr(), shift.data_ptr(), _stream()))
    return call, _clones(scale=scale, shift=shift)


def anchor_norm_finalize(res, which):
    """The instance norm of the map the statistics came from, in fp64 (tests/test_encoder.py's
    _normalised); with one pixel scale = 1 / sqrt(eps) and the normalised value is 0 up to rounding
    (test_statistics_of_a_single_pixel's bars)."""
    y = _enc_stats(which)[0].cpu().numpy()
    scale, shift = res["scale"].numpy(), res["shift"].numpy()
    a, b = te._normalised(y, scale, shift)
    if which == "one-pixel":
        assert np.allclose(scale, 1.0 / np.sqrt(F64(np.float32(EPS))), rtol=1e-6)
        assert np.abs(a).max() <= 1e-3
    else:
        assert norm_rel(a, b) <= REL_TOL


@functools.lru_cache(maxsize=None)
def _join_inputs(affine, per_batch):
    """y, skip, (scale, shift), (skip_scale, skip_shift) as numpy: tests/test_encoder.py::test_join's
    data for corr_enc_join, tests/test_encoder_front.py::test_join_affine's for the affine form."""
    B, C, H, W = 2, 96, 7, 9
    if affine is None:
        return te._input(97, B, C, H, W), te._input(98, B, C, H, W), te._norm(97, B, C, per_batch), None
    return (tfr._input(121, B, C, H, W), tfr._input(122, B, C, H, W), tfr._affine_pair(121, B, C, per_batch),
            tfr._affine_pair(125, B, C, per_batch) if affine == "relu" else None)


@functools.lru_cache(maxsize=None)
def _join_inputs_gpu(affine, per_batch):
    y, skip, norm, knorm = _join_inputs(affine, per_batch)
    return _gpu(y), _gpu(skip), tuple(_gpu(v) for v in norm), None if knorm is None else tuple(_gpu(v) for v in knorm)


def case_join(A, per_batch, alias, affine=None):
    """affine None: corr_enc_join; "relu": corr_enc_join_affine with a skip affine and its ReLU;
    "null": corr_enc_join_affine with both skip pointers NULL.  alias: out = y, an in/out buffer."""
    lib = _lib()
    B, C, H, W = 2, 96, 7, 9
    y, skip, (sc, sh), knorm = _join_inputs_gpu(affine, per_batch)
    y = A.inout("y", y) if alias else A.inp("y", y)
    skip, sc, sh = A.inp("skip", skip), A.inp("scale", sc), A.inp("shift", sh)
    ksc, ksh = (None, None) if knorm is None else (A.inp("skip_scale", knorm[0]), A.inp("skip_shift", knorm[1]))
    out = y if alias else A.out("out", (B, C, H, W))

    def call():
        if affine is None:
            _ok(lib.corr_enc_join(y.data_ptr(), sc.data_ptr(), sh.data_ptr(), int(per_batch), skip.data_ptr(), B, C, H, W,
                                  out.data_ptr(), _stream()))
        else:
            _ok(lib.corr_enc_join_affine(y.data_ptr(), sc.data_ptr(), sh.data_ptr(), int(per_batch), skip.data_ptr(),
                                         None if ksc is None else ksc.data_ptr(), None if ksh is None else ksh.data_ptr(),
                                         int(per_batch), int(affine == "relu"), B, C, H, W, out.data_ptr(), _stream()))
    return call, _clones(out=out)


def anchor_join(res, per_batch, alias, affine=None):
    """The header's formula in fp64 within REL_TOL, as test_join and test_join_affine."""
    y, skip, (sc, sh), knorm = _join_inputs(affine, per_batch)
    s = skip.astype(F64)
    if knorm is not None:
        s = np.maximum(s * tfr._bcast(knorm[0].astype(F64), 2, 96) + tfr._bcast(knorm[1].astype(F64), 2, 96), 0.0)
    ref = np.maximum(s + te._apply64(y, sc, sh), 0.0)
    assert (ref > 0).any() and (ref == 0).any()
    assert norm_rel(res["out"].numpy(), ref) <= REL_TOL


# ----------------------------------------------------------------------------------------------
# corr_enc_stem_forward, corr_enc_pw_forward
# ----------------------------------------------------------------------------------------------
def case_stem(A, cin, shape):
    """The 7x7 stem reads exactly cin planes; 2 x cin x 13 x 17 gives the ragged 7 x 9 output, 1 x cin
    x 3 x 4 is smaller than the window.  Statistics on."""
    lib = _lib()
    B, H, W = shape
    cout = 64
    Ho, Wo = _out_hw(H, W, 2)
    _, bias, pack = _weights("stem", cout, cin)
    x = A.inp("in", _front_input("stem", B, cin, H, W))
    pack, bias = A.inp("packed", pack, align16=True), A.inp("bias", bias)
    out = A.out("out", (B, cout, Ho, Wo))
    sp, sn = A.ws("stats", lib.corr_enc_stats_bytes(B, cout, Ho, Wo), full=True)
    st = A.last_ws

    def call():
        _ok(lib.corr_enc_stem_forward(x.data_ptr(), cin, B, H, W, pack.data_ptr(), bias.data_ptr(), cout, out.data_ptr(),
                                      sp, sn, _stream()))
    return call, _clones(out=out, stats=st)


@functools.lru_cache(maxsize=None)
def _front_input(kind, B, cin, H, W):
    return _gpu(tfr._input(SEED, B, cin, H, W, 0.5 if kind == "stem" else 0.0))


def anchor_stem(res, cin, shape):
    B, H, W = shape
    got = res["out"].numpy()
    e = norm_rel(got, tfr._ref64("stem", SEED, B, H, W, cin, 64, 2, 0.5))
    print(f"stem cin {cin} {shape}: norm_rel {e:.2e}")
    assert e <= REL_TOL
    _check_statistics(got, res["stats"], B, 64)


def case_pw(A, cin, cout, shape, stride):
    lib = _lib()
    B, H, W = shape
    Ho, Wo = _out_hw(H, W, stride)
    _, bias, pack = _weights("pw", cout, cin)
    x = A.inp("in", _front_input("pw", B, cin, H, W))
    pack, bias = A.inp("packed", pack, align16=True), A.inp("bias", bias)
    out = A.out("out", (B, cout, Ho, Wo))
    sp, sn = A.ws("stats", lib.corr_enc_stats_bytes(B, cout, Ho, Wo), full=True)
    st = A.last_ws

    def call():
        _ok(lib.corr_enc_pw_forward(x.data_ptr(), cin, B, H, W, stride, pack.data_ptr(), bias.data_ptr(), cout,
                                    out.data_ptr(), sp, sn, _stream()))
    return call, _clones(out=out, stats=st)


def anchor_pw(res, cin, cout, shape, stride):
    B, H, W = shape
    got = res["out"].numpy()
    e = norm_rel(got, tfr._ref64("pw", SEED, B, H, W, cin, cout, stride, 0.0))
    print(f"pw {cin} -> {cout} {shape} stride {stride}: norm_rel {e:.2e}")
    assert e <= REL_TOL
    if got.shape[2] * got.shape[3] > 1:
        _check_statistics(got, res["stats"], B, cout)


# ----------------------------------------------------------------------------------------------
# corr_mask_upsample_forward
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mask_inputs(B, H, W, channels, offset):
    hidden, flow = tm._inputs(B, H, W)
    return _windowed(_gpu(hidden), channels, offset), _gpu(flow)


def case_mask_upsample(A, shape, channels, offset):
    lib = _lib()
    B, H, W = shape
    _, bias, pack = _weights("mask", 576, 256)
    hidden, flow = _mask_inputs(B, H, W, channels, offset)
    hidden, flow = A.inp("hidden", hidden), A.inp("flow", flow)
    pack, bias = A.inp("packed", pack, align16=True), A.inp("bias", bias)
    out = A.out("out", (B, 2, 8 * H, 8 * W))

    def call():
        _ok(lib.corr_mask_upsample_forward(hidden.data_ptr(), channels, offset, flow.data_ptr(), pack.data_ptr(),
                                           bias.data_ptr(), tm.SCALE, B, H, W, out.data_ptr(), _stream()))
    return call, _clones(out=out)


def anchor_mask_upsample(res, shape, channels, offset):
    e = norm_rel(res["out"].numpy(), tm._ref64(*shape, 1))
    print(f"mask_upsample {shape}: norm_rel {e:.2e}")
    assert e <= REL_TOL


# ----------------------------------------------------------------------------------------------
# corr_flow_enc_forward, corr_flow_head_forward
# ----------------------------------------------------------------------------------------------
def case_flow_enc(A, shape):
    """2x7x9: out (channels 64 .. 191) and flow_copy (192, 193) are one 256-channel tensor.  1x3x4:
    flow_copy is a tensor of its own.  1x1x1: flow_copy NULL."""
    lib = _lib()
    B, H, W = shape
    cout = 128
    _, bias, pack = _weights("flow_enc", cout, 2)
    flow = A.inp("flow", _flow_gpu(shape))
    pack, bias = A.inp("packed", pack, align16=True), A.inp("bias", bias)
    if shape == (2, 7, 9):
        out = copy_ = A.out("x", (B, 256, H, W), full=False)
        oc, off, cc, coff = 256, 64, 256, 192
        collect = _window_results(out, out=(off, cout), flow_copy=(coff, 2))
    else:
        out = A.out("out", (B, cout, H, W))
        copy_ = A.out("flow_copy", (B, 2, H, W)) if shape == (1, 3, 4) else None
        oc, off, cc, coff = cout, 0, 2 if copy_ is not None else 0, 0
        collect = _clones(out=out, **({} if copy_ is None else {"flow_copy": copy_}))

    def call():
        _ok(lib.corr_flow_enc_forward(flow.data_ptr(), B, H, W, pack.data_ptr(), bias.data_ptr(), cout, 1, out.data_ptr(),
                                      oc, off, None if copy_ is None else copy_.data_ptr(), cc, coff, _stream()))
    return call, collect


@functools.lru_cache(maxsize=None)
def _flow_gpu(shape):
    return _gpu(tf._flow(*shape))


def anchor_flow_enc(res, shape):
    e = norm_rel(res["out"].numpy(), np.maximum(tf._enc_ref64(*shape, 128), 0.0))
    print(f"flow_enc {shape}: norm_rel {e:.2e}")
    assert e <= REL_TOL
    if shape != (1, 1, 1):
        assert bit_equal(res["flow_copy"].numpy(), tf._flow(*shape))
    if shape == (2, 7, 9):
        assert float(res["words_changed_outside"]) == 0


@functools.lru_cache(maxsize=None)
def _head_inputs(shape):
    cin, c0 = tf._coords(*shape)
    return _windowed(_gpu(tf._hidden(*shape)), 512, 0), _gpu(cin), _gpu(c0)


def case_flow_head(A, shape, form):
    """hidden is channels 0 .. 255 of 512.  form "delta": coords_in NULL; "coords": with coords_in;
    "flow": with coords_in and coords0."""
    lib = _lib()
    B, H, W = shape
    _, bias, pack = _weights("flow_head", 2, 256)
    hidden, cin, c0 = _head_inputs(shape)
    hidden, pack, bias = A.inp("hidden", hidden), A.inp("packed", pack, align16=True), A.inp("bias", bias)
    cin = A.inp("coords_in", cin) if form != "delta" else None
    c0 = A.inp("coords0", c0) if form == "flow" else None
    outs = {"delta": A.out("delta", (B, 2, H, W))}
    if cin is not None:
        outs["coords_out"] = A.out("coords_out", (B, 2, H, W))
    if c0 is not None:
        outs["flow_out"] = A.out("flow_out", (B, 2, H, W))
    ptr = lambda t: None if t is None else t.data_ptr()

    def call():
        _ok(lib.corr_flow_head_forward(hidden.data_ptr(), 512, 0, B, H, W, pack.data_ptr(), bias.data_ptr(), ptr(cin),
                                       ptr(c0), outs["delta"].data_ptr(), ptr(outs.get("coords_out")),
                                       ptr(outs.get("flow_out")), _stream()))
    return call, _clones(**outs)


def anchor_flow_head(res, shape, form):
    """delta: the fp64 convolution within REL_TOL; the two updates are one fp32 operation each on
    the delta this launch stores, so they are checked bit for bit."""
    delta = res["delta"].numpy()
    e = norm_rel(delta, tf._head_ref64(*shape))
    print(f"flow_head {shape} {form}: norm_rel {e:.2e}")
    assert e <= REL_TOL
    cin, c0 = tf._coords(*shape)
    if form != "delta":
        assert bit_equal(res["coords_out"].numpy(), cin + delta)
    if form == "flow":
        assert bit_equal(res["flow_out"].numpy(), res["coords_out"].numpy() - c0)


# ----------------------------------------------------------------------------------------------
# corr_ondemand_lookup_conv, corr_pyramid_export, corr_pyramid_import
# ----------------------------------------------------------------------------------------------
def case_ondemand_lookup_conv(A, geo):
    B, D, H, W, L, r = GEO[geo]
    lib = _lib()
    ws = A.inp("workspace", core._prepared(geo), align16=True)
    cs = [A.inp(f"coords{t}", c) for t, c in enumerate(core._lookups(geo)[0])]
    _, pack, bias, _, _ = core._convc1("A")  # geometries A and G both have 3 levels: one [256, 243] weight
    pack, bias = A.inp("packed", pack, align16=True), A.inp("bias", bias)
    outs = [A.out(f"out{t}", (B, 256, H, W)) for t in range(T)]

    def call():
        for c, o in zip(cs, outs):
            _ok(lib.corr_ondemand_lookup_conv(ws.data_ptr(), c.data_ptr(), B, D, H, W, L, r, 0, pack.data_ptr(),
                                              bias.data_ptr(), 1, o.data_ptr(), _stream()))
    return call, _clones(**{f"out{t}": o for t, o in enumerate(outs)})


def anchor_ondemand_lookup_conv(res, geo):
    """tests/test_ondemand_conv.py::test_special_coordinates' check: against relu(conv2d(.)) in fp64 of
    corr_ondemand_lookup's own output for the same workspace and coordinates, the same non-finite
    pattern (the query with NaN coordinates is NaN in all 256 outputs) and 1e-5 of the largest."""
    B, D, H, W, L, r = GEO[geo]
    lib = _lib()
    assert L == GEO["A"][4]
    w, _, bias, _, _ = core._convc1("A")
    for t, c in enumerate(core._lookups(geo)[0]):
        look = torch.empty(B, L * (2 * r + 1) ** 2, H, W, device=DEV)
        _ok(lib.corr_ondemand_lookup(core._prepared(geo).data_ptr(), c.data_ptr(), B, D, H, W, L, r, 0, look.data_ptr(),
                                     _stream()))
        torch.cuda.synchronize()
        ref = torch.relu(toc._ref64_from(look, w.view(256, -1, 1, 1), bias)).numpy()
        assert np.isnan(ref).any() and np.isfinite(ref).any() and (ref[np.isfinite(ref)] > 0).any()
        e = norm_rel(res[f"out{t}"].numpy(), ref)
        print(f"ondemand_lookup_conv {geo} lookup {t}: {e:.2e} of the largest output")
        assert e <= 1e-5


def case_pyramid_export(A, geo):
    """The tiled levels come from a build into sentinel-prefilled buffers: padding cells are poison."""
    B, _, H, W, L, _ = GEO[geo]
    lib = _lib()
    lv = core._pyr_in(A, geo)
    outs = [A.out(f"out{l}", s) for l, s in enumerate(core._level_shapes(geo, False))]

    def call():
        _ok(lib.corr_pyramid_export(_ptrs(lv), B * H * W, H, W, L, _ptrs(outs), _stream()))
    return call, _clones(**{f"out{l}": o for l, o in enumerate(outs)})


def anchor_pyramid_export(res, geo):
    """The fp64 chain of oracle/torch_ops.py (the all-pairs product and its average pools), REL_TOL."""
    from oracle.torch_ops import cpu_build
    _, _, H, W, L, _ = GEO[geo]
    f1, f2 = (t.cpu().double() for t in core._fmaps(geo))
    for l, ref in enumerate(cpu_build(f1, f2, L)):
        got = res[f"out{l}"].numpy().reshape(ref.shape)
        assert norm_rel(got, ref.numpy()) <= REL_TOL, l


def case_pyramid_import(A, geo):
    """Every word of every tiled level is written (padding cells are zeroed); the export of the
    result is among the results."""
    B, _, H, W, L, _ = GEO[geo]
    lib = _lib()
    src = [A.inp(f"src{l}", v) for l, v in enumerate(core._grad_pyramid(geo))]
    lv = [A.out(f"pyr{l}", s) for l, s in enumerate(core._level_shapes(geo, True))]

    def call():
        _ok(lib.corr_pyramid_import(_ptrs(src), B * H * W, H, W, L, _ptrs(lv), _stream()))

    def collect():
        res = {f"tiled{l}": v.clone() for l, v in enumerate(lv)}
        res.update(core._export(lv, geo))
        return res
    return call, collect


def anchor_pyramid_import(res, geo):
    """The export of the import is the source, bit for bit, and every other word is a zero."""
    for l, src in enumerate(core._grad_pyramid(geo)):
        src = src.cpu()
        assert torch.equal(res[f"pyr{l}"].view(torch.int32), src.view(torch.int32)), l
        assert int((res[f"tiled{l}"].view(torch.int32) != 0).sum()) == int((src.view(torch.int32) != 0).sum()), l


# ----------------------------------------------------------------------------------------------
# the table: id -> (entry point, case, anchor, whether it has a statistics buffer)
# ----------------------------------------------------------------------------------------------
def _table():
    t = {}

    def add(entry, label, fn, anchor, stats=False, **kw):
        name = f"{entry}[{label}]"
        assert name not in t, name
        t[name] = (entry, functools.partial(fn, **kw), functools.partial(anchor, **kw), stats)

    for entry, sizes in (("corr_conv_pack_weights", ((126, 256), (1, 32))),
                         ("corr_enc_stem_pack_weights", ((64, 15), (64, 1))),
                         ("corr_enc_pw_pack_weights", ((96, 64), (1, 32))),
                         ("corr_mask_upsample_pack_weights", ((576, 256),)),
                         ("corr_flow_enc_pack_weights", ((128, 2),)),
                         ("corr_flow_head_pack_weights", ((2, 256),))):
        for cout, cin in sizes:
            add(entry, f"{cout}x{cin}", case_pack, anchor_pack, pack_fn=entry, cout=cout, cin=cin)
    for shape in CONV:
        add("corr_conv_forward", shape, case_conv_forward, anchor_conv_forward, shape=shape)
        for pn, p in PRECS.items():
            add("corr_conv_forward_prec", f"{shape}-{pn}", case_conv_forward, anchor_conv_forward, shape=shape, precision=p)
    for stride in (1, 2):
        add("corr_enc_conv_forward", f"2x7x9-s{stride}", case_enc_conv, anchor_enc_conv, stats=True, shape="2x7x9",
            stride=stride)
    add("corr_enc_conv_forward", "1x1x1", case_enc_conv, anchor_enc_conv, shape="1x1x1", stride=1)
    for which in ("stride2", "one-pixel"):
        add("corr_enc_norm_finalize", which, case_norm_finalize, anchor_norm_finalize, which=which)
    for per_batch in (True, False):
        for alias in (False, True):
            tag = f"{'batch' if per_batch else 'channel'}-{'inplace' if alias else 'separate'}"
            add("corr_enc_join", tag, case_join, anchor_join, per_batch=per_batch, alias=alias)
            for affine in ("relu", "null"):
                add("corr_enc_join_affine", f"{tag}-skip_{affine}", case_join, anchor_join, per_batch=per_batch,
                    alias=alias, affine=affine)
    for cin in (15, 1):
        for shape in ((2, 13, 17), (1, 3, 4)):
            add("corr_enc_stem_forward", f"cin{cin}-{'x'.join(map(str, shape))}", case_stem, anchor_stem, stats=True,
                cin=cin, shape=shape)
    for stride in (1, 2):
        add("corr_enc_pw_forward", f"2x7x9-s{stride}", case_pw, anchor_pw, stats=True, cin=64, cout=96, shape=(2, 7, 9),
            stride=stride)
    add("corr_enc_pw_forward", "1x1x1", case_pw, anchor_pw, stats=True, cin=32, cout=1, shape=(1, 1, 1), stride=1)
    add("corr_mask_upsample_forward", "2x7x9-off256", case_mask_upsample, anchor_mask_upsample, shape=(2, 7, 9),
        channels=512, offset=256)
    add("corr_mask_upsample_forward", "1x1x1-off0", case_mask_upsample, anchor_mask_upsample, shape=(1, 1, 1),
        channels=256, offset=0)
    for shape in ((2, 7, 9), (1, 3, 4), (1, 1, 1)):
        add("corr_flow_enc_forward", "x".join(map(str, shape)), case_flow_enc, anchor_flow_enc, shape=shape)
    for shape in ((2, 7, 9), (1, 1, 1)):
        for form in ("delta", "coords", "flow"):
            add("corr_flow_head_forward", f"{'x'.join(map(str, shape))}-{form}", case_flow_head, anchor_flow_head,
                shape=shape, form=form)
    for geo in "AG":
        add("corr_ondemand_lookup_conv", geo, case_ondemand_lookup_conv, anchor_ondemand_lookup_conv, geo=geo)
    add("corr_pyramid_export", "A", case_pyramid_export, anchor_pyramid_export, geo="A")
    add("corr_pyramid_import", "A", case_pyramid_import, anchor_pyramid_import, geo="A")
    return t


CASES = _table()
IDS = list(CASES)
_PLAIN = {}


def _plain(name):
    """The same call made the ordinary way (plain tensors, the default stream); made once."""
    if name not in _PLAIN:
        _PLAIN[name] = {k: v.cpu() for k, v in _run_case(CASES[name][1], Arena()).items()}
    return _PLAIN[name]


# ----------------------------------------------------------------------------------------------
# the four properties
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_writes_stay_inside(gpu, name):
    """Property 1: every output, in/out buffer and statistics buffer in a guarded window."""
    arena = Arena(guard_out=True, guard_ws=True)
    got = _run_case(CASES[name][1], arena)
    arena.check()
    _same(_plain(name), got, name, clean=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in IDS if CASES[n][3]])
def test_workspace_is_as_large_as_claimed_and_needs_no_initialisation(gpu, name):
    """Property 2 for the statistics: a buffer of exactly corr_enc_stats_bytes, in a guarded window,
    holding the sentinel, is fully written and nothing past it is touched."""
    arena = Arena(guard_ws=True)
    got = _run_case(CASES[name][1], arena)
    assert arena.n_ws == 1
    arena.check()
    _same(_plain(name), got, name, clean=True)


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("name", IDS)
def test_results_do_not_depend_on_memory_outside_the_inputs(gpu, name, misalign):
    """Property 3: NaN before and after every input and in the channels outside a channel window;
    again with the 4-byte-aligned inputs one float off their 16-byte boundary."""
    arena = Arena(guard_in=True, misalign=misalign)
    got = _run_case(CASES[name][1], arena)
    arena.check()
    _same(_plain(name), got, name, clean=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_work_is_ordered_on_the_callers_stream(gpu, side, name):
    """Property 4 (test_core_discipline._ordered_on_the_callers_stream)."""
    ref = _plain(name)  # also loads every kernel of the case, so that the enqueue only enqueues
    _ordered_on_the_callers_stream(CASES[name][1], ref, side, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_the_plain_call_is_anchored(gpu, name):
    """What the four properties compare with is itself right (see each anchor)."""
    res = _plain(name)
    for k, v in res.items():
        _guard.check_clean(v, f"{name}: {k}")
    CASES[name][2](res)


def _fake_window_case(A, astray):
    """A torch-only "entry point" that sums channels 4 .. 11 of a 16-channel tensor in place; with
    `astray` it also reads channel 12, multiplied by zero."""
    x = A.inp("x", _windowed(torch.arange(8 * 8 * 4, dtype=torch.float32, device=DEV).view(1, 8, 8, 4), 16, 4))
    y = A.out("y", (1, 8, 4))

    def call():
        torch.sum(x[:, 4:12], 1, out=y)
        if astray:
            y.add_(x[:, 12] * 0.0)
    return call, _clones(y=y)


@pytest.mark.gpu
@pytest.mark.parametrize("astray", [False, True])
def test_the_input_test_notices_a_read_outside_the_channel_window(gpu, astray):
    """Property 3's own check for the channel-window role: it passes a fake entry point that keeps
    to its window and fails one that reads a channel outside it, although that read is multiplied
    by zero and the plain call makes it too."""
    case = functools.partial(_fake_window_case, astray=astray)
    ref = {k: v.cpu() for k, v in _run_case(case, Arena()).items()}
    arena = Arena(guard_in=True)
    got = _run_case(case, arena)
    arena.check()
    if not astray:
        _same(ref, got, "fake", clean=True)
        assert torch.isfinite(ref["y"]).all()
    else:
        with pytest.raises(AssertionError, match="the sentinel reached the result"):
            _same(ref, got, "fake", clean=True)


# ----------------------------------------------------------------------------------------------
# the ratchet (no GPU)
# ----------------------------------------------------------------------------------------------
def test_the_table_is_what_the_core_ratchet_sends_here():
    """The table's entry points are exactly those that test_core_discipline.COVERED_ELSEWHERE maps
    to this file, each owner is one of the four property tests, and every case the suite promises
    is there."""
    here = {n: o for n, o in core.COVERED_ELSEWHERE.items() if o.startswith("test_family_discipline.py::")}
    assert {entry for entry, *_ in CASES.values()} == set(here)
    assert len(here) == 20 and len(here) == len(core.COVERED_ELSEWHERE)
    four = {"test_writes_stay_inside", "test_workspace_is_as_large_as_claimed_and_needs_no_initialisation",
            "test_results_do_not_depend_on_memory_outside_the_inputs", "test_work_is_ordered_on_the_callers_stream"}
    assert {o.split("::")[1] for o in here.values()} <= four
    for name in four:
        assert callable(globals()[name])
    want = {"corr_conv_pack_weights": 2, "corr_conv_forward": 2, "corr_conv_forward_prec": 4, "corr_enc_conv_forward": 3,
            "corr_enc_norm_finalize": 2, "corr_enc_join": 4, "corr_enc_join_affine": 8, "corr_enc_stem_pack_weights": 2,
            "corr_enc_stem_forward": 4, "corr_enc_pw_pack_weights": 2, "corr_enc_pw_forward": 3,
            "corr_mask_upsample_pack_weights": 1, "corr_mask_upsample_forward": 2, "corr_flow_enc_pack_weights": 1,
            "corr_flow_enc_forward": 3, "corr_flow_head_pack_weights": 1, "corr_flow_head_forward": 6,
            "corr_ondemand_lookup_conv": 2, "corr_pyramid_export": 1, "corr_pyramid_import": 1}
    have = {}
    for entry, *_ in CASES.values():
        have[entry] = have.get(entry, 0) + 1
    assert have == want
    # the entry points with a statistics buffer are those whose prototype takes stats_bytes
    with_stats = {entry for entry, _, _, stats in CASES.values() if stats}
    assert with_stats == {"corr_enc_conv_forward", "corr_enc_stem_forward", "corr_enc_pw_forward"}
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "corr_mi355x.h")) as f:
        text = f.read()
    assert set(re.findall(r"\b(corr_\w+)\s*\([^;{]*?size_t stats_bytes[^;{]*?\)\s*;", text)) == with_stats


# ----------------------------------------------------------------------------------------------
# a cached pack used from a second stream (eraft_amd/_cache.py)
# ----------------------------------------------------------------------------------------------
def _two_stream_gru():
    from eraft_amd.gru import sepconv_gru
    net, inp, _, _ = tc._block_inputs(SEED, 2, 7, 9, fused=True)
    h, x = _gpu(net), _gpu(np.concatenate([inp, prng.gauss(SEED + 9, (2, 128, 7, 9))], 1))
    return tc._block(DEV).gru, lambda m: (sepconv_gru(m, h, x),)


def _two_stream_update_block():
    from eraft_amd.update import update_block
    arrs = tuple(_gpu(a) for a in tc._block_inputs(SEED, 2, 7, 9, fused=True))
    return tc._block(DEV), lambda m: tuple(t.clone() for t in update_block(m, *arrs, fused=True, defer_mask=True))


def _two_stream_encoder():
    from eraft_amd.encoder import encoder_forward
    x = _gpu(prng.gauss(SEED, (2, 3, 32, 40)))
    return te._encoder("batch", 3, DEV), lambda m: (encoder_forward(m, x),)


def _two_stream_mask_upsample():
    from eraft_amd.upsample import mask_upsample
    hidden, flow = (_gpu(a) for a in tm._inputs(2, 7, 9))
    return tc._block(DEV).mask[2], lambda m: (mask_upsample(m, hidden, 0, flow),)


def _two_stream_lookup_conv():
    """CorrBlock.lookup_conv: the "module" is convc1, the block is built once and shared."""
    from eraft_amd import CorrBlock
    f1, f2 = _gpu(prng.gauss(SEED + 1, (1, 32, 16, 24))), _gpu(prng.gauss(SEED + 2, (1, 32, 16, 24)))
    blk, coords = CorrBlock(f1, f2, num_levels=4, radius=4), _gpu(prng.lookup_coords(SEED + 3, 1, 16, 24, 3.0))
    return tc._block(DEV).encoder.convc1, lambda m: (blk.lookup_conv(coords, m.weight, m.bias),)


TWO_STREAM = {"sepconv_gru": _two_stream_gru, "update_block": _two_stream_update_block,
              "encoder": _two_stream_encoder, "mask_upsample": _two_stream_mask_upsample,
              "lookup_conv": _two_stream_lookup_conv}


@pytest.mark.gpu
@pytest.mark.parametrize("which", list(TWO_STREAM))
def test_a_cached_pack_is_ordered_for_a_second_stream(gpu, side, monkeypatch, which):
    """The module's first call, which makes its packs, is enqueued on the side stream behind the
    producer; the same call follows at once on the default stream, a cache hit.  Without an
    ordering between the make and the hit the second call reads packs that are not written yet.
    Both results must be the bits of a deep copy of the module (its own tensors, so its own cache
    entries) run alone on the default stream.

    The control has two legs, since a correct cache makes the default stream wait for the side
    stream from the hit onwards.  Before the second call the default stream clones a probe that
    receives its values behind the producer: it must still see the sentinel (the default stream
    does overtake the side stream).  After the second call is enqueued the host asks whether an
    event recorded behind the producer has completed: it must not have (the hit was enqueued while
    the packs were still unwritten).  If either leg does not hold the run proved nothing.
    Everything read is allocated memory: a failure is a wrong value, not a fault."""
    from eraft_amd.model import SepConvGRU
    monkeypatch.setattr(SepConvGRU, "fused", True)  # the update block's GRU on its kernels, not on MIOpen
    with torch.no_grad():
        module, run = TWO_STREAM[which]()
        keep = copy.deepcopy(module)      # kept alive: its packs' memory is not handed out again
        ref = [t.cpu() for t in run(keep)]
        probe, values = _poison(torch.empty(1024, device=DEV)), torch.zeros(1024, device=DEV)
        produced = torch.cuda.Event()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            core._produce()
            probe.copy_(values)
            produced.record()
            first = run(module)
        early = probe.clone()
        second = run(module)
        still_producing = not produced.query()
        side.synchronize()
        torch.cuda.synchronize()
    assert bool((_guard._bits(early) == _guard.SENTINEL).all()) and still_producing, \
        "the producer ended before the second call was enqueued: it is too short to prove anything"
    assert not bool(probe.any())
    for tag, got in (("on the making stream", first), ("on the second stream", second)):
        assert len(got) == len(ref)
        for k, (a, b) in enumerate(zip(got, ref)):
            assert bit_equal(a.cpu().numpy(), b.numpy()), f"{which}: result {k} {tag} differs from the reference"
