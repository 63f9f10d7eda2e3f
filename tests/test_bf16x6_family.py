"""The bf16x6 convolution family's six products, pinned bit for bit (csrc/corr_bf16x6.h: split3, six(),
store_pieces; corr_common.h: split_sum).

The split is exact, so with inputs on which every output has exactly one non-zero product, and that
product is exactly representable in fp32, a kernel's answer is known to the last bit and every lost
piece shows (tests/_bf16x6.py has the model, the operand classes A-D and the planners).

CPU: the model and the generators, and that the chosen inputs tell a kernel that loses a product from
one that does not.  GPU: for the kernels with a linear epilogue the weight pieces of every (cout, cin,
tap), the activation pieces of every pixel, the cross terms and the bias alone, all by bit equality;
an element-wise a-priori error bound; for the GRU half step, the mask head and the fused lookups, whose
product cannot be read back, the forms described at their tests; and the non-finite rule against the
fp32 op chain.  DESIGN.md §22 has the measured bound ratios and the mutation table.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _bf16x6 as bx
import prng
from _util import REL_TOL, bit_equal

DEV = "cuda:0"
F32, F64 = np.float32, np.float64
HID = 128


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


# ----------------------------------------------------------------------------------------------
# the kernels with a linear epilogue
# ----------------------------------------------------------------------------------------------
class Lin:
    """One configuration of a linear kernel: out = conv(x, w, stride, pad) + bias."""

    def __init__(self, kind, cin, cout, stride=1, ca=None, off=0):
        self.kind, self.cin, self.cout, self.stride, self.ca, self.off = kind, cin, cout, stride, ca or cin, off
        self.k = {"conv": 3, "enc_conv": 3, "stem": 7, "pw": 1, "flow_enc": 7, "flow_head": 3}[kind]
        self.pad = self.k // 2
        self.relu = kind in ("conv", "flow_enc")  # the kernels with a ReLU switch
        # S: six() calls that feed one output (the K steps of 32; read from each kernel's main loop)
        self.S = {"conv": 9 * cin // 32,        # corr_conv.hip: chunk outer, tap inner, one step each
                  "enc_conv": 9 * cin // 32,    # the same kernel's <STRIDE, NORM_IN, STATS> forms
                  "stem": 25,                   # corr_enc_front.hip: kStemSteps, two taps of <= 16 channels a step
                  "pw": cin // 32,              # one tap
                  "flow_enc": 4,                # corr_flow.hip: kFeSteps, 16 taps of 2 channels a step
                  "flow_head": 9 * 8}[kind]     # kFhKS = 8 steps for each of the 9 per-tap products
        # c: the roundings that are no MFMA's (see test_error_bound)
        self.c = 5 + (16 if kind == "flow_head" else 0)

    def __repr__(self):
        ch = f"{self.ca}+{self.cin - self.ca}" if self.ca != self.cin else f"{self.cin}"
        return f"{self.kind}-s{self.stride}-{ch}-{self.cout}" + (f"-off{self.off}" if self.off else "")

    def bind(self, w):
        """Packs w [cout, cin, k, k] once; returns run(x, bias=None, relu=False) -> numpy out."""
        from eraft_amd import _lib
        k, cout = self.kind, self.cout
        wg = _gpu(w)
        if k in ("conv", "enc_conv"):  # cout = 512: the pack stacked from two weights
            packed = _lib.conv_pack_weights([wg[:256].contiguous(), wg[256:].contiguous()] if cout == 512 else wg)
        else:
            packed = {"stem": _lib.enc_stem_pack_weights, "pw": _lib.enc_pw_pack_weights,
                      "flow_enc": _lib.flow_enc_pack_weights, "flow_head": _lib.flow_head_pack_weights}[k](wg)

        def run(x, bias=None, relu=False):
            bg = _gpu(np.zeros(cout, F32) if bias is None else bias)
            xg = _gpu(x)
            if k == "conv":
                a = xg[:, :self.ca].contiguous()
                b = xg[:, self.ca:].contiguous() if self.ca < self.cin else None
                out = _lib.conv_forward(a, b, packed, bg, cout, relu)
            elif k == "flow_enc":
                out = _lib.flow_enc_forward(xg, packed, bg, cout, relu)
            else:
                assert not relu
                if k == "enc_conv":
                    out = _lib.enc_conv_forward(xg, packed, bg, cout, self.stride)
                elif k == "stem":
                    out = _lib.enc_stem_forward(xg, packed, bg, cout)
                elif k == "pw":
                    out = _lib.enc_pw_forward(xg, packed, bg, cout, self.stride)
                else:
                    buf = torch.full((x.shape[0], 256 + self.off) + x.shape[2:], 1e6, dtype=torch.float32, device=DEV)
                    buf[:, self.off:] = xg
                    out = _lib.flow_head_forward(buf, self.off, packed, bg)[0]
            return out.cpu().numpy()
        return run


# the suites' edge shapes (partial tiles, B > 1, more than two tiles along W, along H); at stride 2 the
# inputs whose outputs have these shapes
EDGE = [(2, 7, 9), (1, 5, 35), (1, 13, 5)]
EDGE2 = [(2, 13, 17), (1, 9, 69), (1, 25, 9)]


def _cases():
    out = []
    for lin, shapes in ((Lin("conv", 256, 126, ca=192), EDGE),       # both input pointers, padded output rows
                        (Lin("conv", 128, 512), EDGE[:1]),           # the pack stacked from two weights
                        (Lin("conv", 64, 1, ca=32), EDGE[:1]),       # the smallest channel counts
                        (Lin("enc_conv", 64, 96), EDGE),
                        (Lin("enc_conv", 64, 96, stride=2), EDGE2),
                        (Lin("enc_conv", 32, 1), EDGE[:1]),
                        (Lin("stem", 15, 64, stride=2), EDGE2),
                        (Lin("stem", 16, 1, stride=2), EDGE2[:1]),
                        (Lin("pw", 64, 96), EDGE),
                        (Lin("pw", 64, 96, stride=2), EDGE2),
                        (Lin("pw", 32, 1), EDGE[:1]),
                        (Lin("flow_enc", 2, 128), EDGE),
                        (Lin("flow_enc", 2, 100), EDGE[:1]),
                        (Lin("flow_enc", 2, 1), EDGE[:1]),
                        (Lin("flow_head", 256, 2), EDGE),
                        (Lin("flow_head", 256, 2, off=256), EDGE[:1])):
        out += [pytest.param(lin, s, id=f"{lin!r}-{'x'.join(map(str, s))}") for s in shapes]
    return out


CASES = _cases()
FIRST = [c for c in CASES if c.values[1] in (EDGE[0], EDGE2[0])]  # every configuration once


def _seed(lin, shape):
    return 31 * sum(map(ord, repr(lin))) + sum(shape)


def impulse_launches(cls, seed, shape, wshape, stride, padding, scale=0, spread=(20, 12), max_launches=400,
                     full=True):
    """(w, plan, [(x, sites, expected)]): a dense class `cls` weight and impulse launches against it,
    until every (cin, tap) has been reached (full) or for max_launches."""
    cout, cin, kh, kw = wshape
    B, _, H, W = shape
    wv, pv = bx.operands(cls, seed, cout * cin * kh * kw, 4096, scale, *spread)
    w = wv.reshape(wshape)
    plan = bx.ImpulsePlan(B, cin, H, W, (kh, kw), stride, padding)
    out, used = [], 0
    while not plan.done() and len(out) < max_launches:
        sites = plan.next_sites()
        if not sites:
            continue
        x = bx.impulses(shape, sites, pv[(used + np.arange(len(sites))) % pv.size])
        used += len(sites)
        out.append((x, sites, bx.expected_conv(x, w, stride, padding)))
    assert plan.done() or not full, "the launches do not reach every (cin, tap)"
    return w, plan, out


def onehot_launches(seed, shape, wshape, stride, padding, scale=0, spread=(20, 12)):
    """(x, [(w, expected)]): a dense class B activation and one-hot weight launches against it, until
    every tap has occurred."""
    cout, cin, kh, kw = wshape
    xv, pv = bx.operands("B", seed, int(np.prod(shape)), 1024, scale, *spread)
    x = xv.reshape(shape)
    out = []
    for n in range(max(2, -(-kh * kw // cout))):
        w = bx.onehot_weights(cout, cin, (kh, kw), n, pv[(n * cout + np.arange(cout)) % pv.size])
        out.append((w, bx.expected_conv(x, w, stride, padding)))
    return x, out


def _assert_onehot_coverage(launches, wshape):
    taps = np.zeros(wshape[2:], bool)
    pix = None
    for w, exp in launches:
        taps |= (w != 0).any(axis=(0, 1))
        hit = (exp != 0).any(axis=1)
        pix = hit if pix is None else pix | hit
    assert taps.all(), "a tap never occurred"
    assert pix.all(), "an output pixel never held a product"


# ----------------------------------------------------------------------------------------------
# CPU: the model, the generators, and that the inputs can tell
# ----------------------------------------------------------------------------------------------
def test_model_split_is_exact():
    """hi + mid + lo == x in fp64 for 10^5 values over +-20 decades; every piece is a bf16."""
    rng = np.random.default_rng(7)
    x = (rng.standard_normal(100000) * 10.0 ** rng.uniform(-20, 20, 100000)).astype(F32)
    h, m, l = bx.split3(x)
    assert (h.astype(F64) + m.astype(F64) + l.astype(F64) == x.astype(F64)).all()
    for p in (h, m, l):
        assert (p.view(np.uint32) & 0xFFFF == 0).all()
    assert (np.abs(m) <= np.abs(h) * 2.0 ** -8).all() and (np.abs(l) <= np.abs(h) * 2.0 ** -16).all()


def test_model_guards():
    """The truncated hi next to FLT_MAX, (inf, 0, 0) for the infinities, NaN through hi."""
    fmax = np.array([bx.FLT_MAX, -bx.FLT_MAX, np.float32(3.4e38)], F32)
    h, m, l = bx.split3(fmax)
    assert np.isfinite(h).all() and (h.astype(F64) + m.astype(F64) + l.astype(F64) == fmax.astype(F64)).all()
    assert h.view(np.uint32)[0] == 0x7F7F0000
    h, m, l = bx.split3(np.array([np.inf, -np.inf], F32))
    assert np.array_equal(h, [np.inf, -np.inf]) and not m.any() and not l.any()
    assert np.isnan(bx.split3(np.array([np.nan], F32))[0]).all()
    # rne: ties to even, in both directions
    t = np.array([0x3F808000, 0x3F818000, 0x3F808001], np.uint32).view(F32)
    assert np.array_equal(bx.rne_bf16(t).view(np.uint32), [0x3F800000, 0x3F820000, 0x3F810000])
    # the model's infinity rule is split_sum's
    assert bx.six_model(np.array([np.inf], F32), np.array([2.0], F32))[0] == np.inf
    assert bx.six_model(np.array([-3.0], F32), np.array([np.inf], F32))[0] == -np.inf


@pytest.mark.parametrize("cls", "ABCD")
def test_generators_hold_their_preconditions(cls):
    """operands() checks them itself (check_pairs raises); here also which products each class needs:
    the model without a product differs from the exact product exactly for those."""
    needs = {"A": {"wl_xh", "wm_xh", "wh_xh"}, "B": {"wl_xh", "wm_xh", "wh_xh"},
             "C": {"wm_xm", "wm_xh", "wh_xm", "wh_xh"}, "D": {"wl_xh", "wm_xh", "wh_xh"}}[cls]
    if cls == "B":
        needs = {"wh_xl", "wh_xm", "wh_xh"}
    for seed in (1, 2, 3):
        full, point = bx.operands(cls, seed, 3000, 48)
        w, x = (point[:, None], full[None, :]) if cls == "B" else (full[:, None], point[None, :])
        exact = (w.astype(F64) * x.astype(F64)).astype(F32)
        assert bx.bits_equal(bx.six_model(w, x, mfma=True), exact)   # exact sums: the rounding has no say
        for drop in bx.PRODUCTS:
            same = bx.six_model(w, x, drop=drop).view(np.uint32) == exact.view(np.uint32)
            assert same.all() if drop not in needs else not same.any(), (cls, drop)


def test_check_pairs_refuses_broken_classes():
    one = np.array([1.0], F32)
    for w, x, need in ((np.array([1.0 + 2.0 ** -23], F32), np.array([1.0 + 2.0 ** -23], F32), {"wh", "wl", "xh", "xl"}),
                       (np.array([1.5], F32), one, {"wh", "wm", "xh"}),          # a piece that should not be zero
                       (np.array([1.0 + 2.0 ** -9], F32), one, {"wh", "xh"}),    # a piece that should be zero
                       (np.array([2.0 ** -50], F32), one, {"wh", "xh"})):        # out of the magnitude range
        with pytest.raises(ValueError):
            bx.check_pairs(w, x, need)
    bx.check_pairs(np.array([1.0 + 2.0 ** -9], F32), np.array([1.0 + 2.0 ** -10], F32), {"wh", "wm", "xh", "xm"})


def _model_conv(x, w, stride, padding, drop=None):
    """The model of six() and split_sum on inputs with one product per output: each piece product's
    convolution in fp64 is that product itself, and the sums are taken in the kernels' order in fp32."""
    wp, xp = dict(zip("hml", bx.split3(w))), dict(zip("hml", bx.split3(x)))
    conv = lambda a, b: F.conv2d(torch.from_numpy(a).double(), torch.from_numpy(b).double(), None, stride,
                                 padding).numpy().astype(F32)
    acs = None
    for name in bx.PRODUCTS[:-1]:
        if name != drop:
            p = conv(xp[name[4]], wp[name[1]])
            acs = p if acs is None else (acs + p).astype(F32)
    acc = conv(xp["h"], wp["h"]) if drop != "wh_xh" else np.zeros_like(acs)
    return (acc + acs).astype(F32)


# small stand-ins for the kernels' geometries: 3x3, the strided 7x7, 1x1 at stride 2, the GRU's 1x5
CPU_GEO = [((2, 32, 7, 9), (6, 32, 3, 3), 1, 1), ((1, 5, 13, 17), (4, 5, 7, 7), 2, 3),
           ((2, 32, 13, 17), (5, 32, 1, 1), 2, 0), ((1, 64, 5, 12), (3, 64, 1, 5), 1, (0, 2))]


@pytest.mark.parametrize("geo", CPU_GEO, ids=["3x3", "7x7s2", "1x1s2", "1x5"])
@pytest.mark.parametrize("cls", "ACD")
def test_impulse_inputs_tell_a_lost_product(cls, geo):
    """On the impulse launches the model reproduces the expected output bit for bit, the launches
    observe every (cout, cin, tap), and the model without a product the class needs does not."""
    shape, wshape, stride, pad = geo
    w, plan, launches = impulse_launches(cls, 5, shape, wshape, stride, pad)
    seen = np.zeros(wshape, bool)
    needed = ("wm_xm", "wm_xh", "wh_xm") if cls == "C" else ("wl_xh", "wm_xh")
    for x, sites, exp in launches:
        bx.observe(plan, sites, exp, seen)
        assert bx.bits_equal(_model_conv(x, w, stride, pad), exp)
        for drop in needed:
            assert not bx.bits_equal(_model_conv(x, w, stride, pad, drop), exp), drop
    assert seen.all()


@pytest.mark.parametrize("geo", CPU_GEO, ids=["3x3", "7x7s2", "1x1s2", "1x5"])
def test_onehot_inputs_tell_a_lost_product(geo):
    shape, wshape, stride, pad = geo
    x, launches = onehot_launches(6, shape, wshape, stride, pad)
    _assert_onehot_coverage(launches, wshape)
    for w, exp in launches:
        assert bx.bits_equal(_model_conv(x, w, stride, pad), exp)
        for drop in ("wh_xl", "wh_xm"):
            assert not bx.bits_equal(_model_conv(x, w, stride, pad, drop), exp), drop


@pytest.mark.parametrize("lin,shape", CASES)
def test_gpu_inputs_hold_their_preconditions(lin, shape):
    """The inputs of the GPU tests of the linear kernels, with their seeds, built here on the CPU: the
    generators' own checks pass, every expected output is exact with one product per output, and the
    coverage the GPU tests assert can be reached."""
    xs, ws = _lin_shapes(lin, shape)
    w, plan, launches = impulse_launches("A", _seed(lin, shape), xs, ws, lin.stride, lin.pad)
    seen = np.zeros(ws, bool)
    for x, sites, exp in launches:
        bx.observe(plan, sites, exp, seen)
    assert seen.all()
    _assert_onehot_coverage(onehot_launches(_seed(lin, shape) + 1, xs, ws, lin.stride, lin.pad)[1], ws)
    if shape in (EDGE[0], EDGE2[0]):
        for cls in "CD":
            assert impulse_launches(cls, _seed(lin, shape) + 2, xs, ws, lin.stride, lin.pad,
                                    max_launches=min(lin.k * lin.k, 9), full=False)[2]


@pytest.mark.parametrize("d,shape", [(0, (2, 7, 9)), (1, (1, 13, 5))])
def test_gru_inputs_hold_their_preconditions(d, shape):
    """The q path's inputs with the GPU tests' seeds: |s| <= 2^-13 and tanh(s) within half an ulp."""
    k, pad = _gru_geo(d)
    B, H, W = shape
    for cls in "ACD":
        _, _, launches = impulse_launches(cls, 31 + d, (B, GRU_C, H, W), (HID, GRU_C) + k, 1, pad, **GRU_SCALE,
                                          max_launches=3, full=False)
        for _, _, exp in launches:
            _assert_tanh_is_identity(exp)
    bx.operands("B", 41 + d, B * GRU_C * H * W, 1024, GRU_SCALE["scale"], *GRU_SCALE["spread"])


def test_plans_of_the_gpu_cases_reach_every_weight():
    """The planner alone (no values) on every GPU case's geometry, the GRU's and a clipped one."""
    geos = [(s, lin.cin, lin.k, lin.stride, lin.pad) for lin, s in (c.values for c in CASES)]
    geos += [((2, 7, 9), 448, (1, 5), 1, (0, 2)), ((1, 13, 5), 448, (5, 1), 1, (2, 0)), ((1, 1, 1), 32, 3, 1, 1)]
    for (B, H, W), cin, k, stride, pad in geos:
        plan, n = bx.ImpulsePlan(B, cin, H, W, k, stride, pad), 0
        if (H, W) == (1, 1):  # only the centre tap can be reached
            plan.need[:, ::2] = False
            plan.need[:, :, ::2] = False
        while not plan.done():
            plan.next_sites()
            n += 1
            assert n < 400, ((B, H, W), cin, k)


# ----------------------------------------------------------------------------------------------
# GPU: the linear kernels
# ----------------------------------------------------------------------------------------------
def _lin_shapes(lin, shape):
    B, H, W = shape
    return (B, lin.cin, H, W), (lin.cout, lin.cin, lin.k, lin.k)


@pytest.mark.gpu
@pytest.mark.parametrize("lin,shape", CASES)
def test_weight_pieces(lin, shape):
    """Class A: impulse activations +-2^e against full-mantissa weights.  Every output is one weight
    times a power of two, so all three pieces of that weight (wh xh, wm xh, wl xh) must arrive; the
    counter asserts that every (cout, cin, tap) was such a product."""
    xs, ws = _lin_shapes(lin, shape)
    w, plan, launches = impulse_launches("A", _seed(lin, shape), xs, ws, lin.stride, lin.pad)
    run, seen = lin.bind(w), np.zeros(ws, bool)
    for x, sites, exp in launches:
        bx.observe(plan, sites, exp, seen)
        assert bit_equal(run(x), exp)
    assert seen.all()
    print(f"{lin!r} {shape}: {len(launches)} launches")


@pytest.mark.gpu
@pytest.mark.parametrize("lin,shape", CASES)
def test_activation_pieces(lin, shape):
    """Class B: one-hot weights +-2^e (one (cin, tap) per output channel) against full-mantissa
    activations with a per-pixel exponent spread: every output plane is a shifted, zero-padded,
    scaled copy of an input plane (wh xh, wh xm, wh xl).  Every tap occurs and every output pixel
    holds a product."""
    xs, ws = _lin_shapes(lin, shape)
    x, launches = onehot_launches(_seed(lin, shape) + 1, xs, ws, lin.stride, lin.pad)
    _assert_onehot_coverage(launches, ws)
    for w, exp in launches:
        assert bit_equal(lin.bind(w)(x), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("cls", "CD")
@pytest.mark.parametrize("lin,shape", FIRST)
def test_cross_terms(lin, shape, cls):
    """Classes C (wm xm beside wh xm and wm xh) and D (every piece of the weight against a partner
    that is no power of two) in the impulse form: one pass over the grid offsets."""
    xs, ws = _lin_shapes(lin, shape)
    w, plan, launches = impulse_launches(cls, _seed(lin, shape) + 2, xs, ws, lin.stride, lin.pad,
                                         max_launches=min(lin.k * lin.k, 9), full=False)
    run = lin.bind(w)
    for x, sites, exp in launches:
        assert np.count_nonzero(exp) >= lin.cout
        assert bit_equal(run(x), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("lin,shape", FIRST)
def test_bias_alone(lin, shape):
    """Zero weights and a full-mantissa bias: the output is the bias (or relu(bias)), bit for bit."""
    xs, ws = _lin_shapes(lin, shape)
    bias = bx.operands("A", 11, lin.cout, 1)[0]
    x = prng.gauss(13, xs)
    run = lin.bind(np.zeros(ws, F32))
    for relu in ((False, True) if lin.relu else (False,)):
        got = run(x, bias, relu)
        exp = np.broadcast_to((np.maximum(bias, 0) if relu else bias)[None, :, None, None], got.shape)
        assert bit_equal(got, exp), relu


def _bound_inputs(case, lin, shape):
    """(x, w, bias) of an error-bound case."""
    xs, ws = _lin_shapes(lin, shape)
    x, w = prng.gauss(21, xs).astype(F64), prng.gauss(22, ws, 0.1).astype(F64)
    bias = prng.gauss(23, (lin.cout,), 0.1).astype(F64)
    if case == "in_scales":      # per-input-channel scales, the weights scaled the opposite way
        s = 10.0 ** np.linspace(-3, 3, lin.cin)
        x, w = x * s[None, :, None, None], w / s[None, :, None, None]
    elif case == "out_scales":   # a small output channel is judged on its own magnitude
        s = 10.0 ** np.linspace(-6, 6, lin.cout) if lin.cout > 1 else np.array([1e-6])
        w, bias = w * s[:, None, None, None], bias * s
    elif case == "cancelling":   # pairs of channels that cancel to 1e-4 of their terms
        x[:, 1::2] = x[:, 0::2][:, :x[:, 1::2].shape[1]] * (1 + 1e-4 * prng.gauss(24, x[:, 1::2].shape))
        w[:, 1::2] = -w[:, 0::2][:, :w[:, 1::2].shape[1]]
        bias = bias * 1e-4
    return x.astype(F32), w.astype(F32), bias.astype(F32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["gauss", "in_scales", "out_scales", "cancelling"])
@pytest.mark.parametrize("lin,shape", FIRST)
def test_error_bound(lin, shape, case):
    """Element-wise a-priori bound, as test_build_bf16x6_error_bound's:

        |out - out64| <= (c + 6 S) u (sum |w| |x| + |bias|),   u = 2^-24.

    S is the number of six() calls that feed one output (Lin.S), each MFMA rounding its accumulator
    once: 6 S roundings, each of a partial sum no larger than sum |w| |x|.  c = 5: the piece products
    that six() drops (wm xl and wl xm, each at most 2^-8 2^-16 |w x|: 2 u; wl xl is 2^-32 |w x|), one
    rounding in split_sum's join, one in the bias add, and one u for the second-order terms of all of
    these (the sums are bounded by (1 + u)^(6 S + 4) times the exact ones; (6 S + 4)^2 u < 1 for every
    S here).  The output is stored as the bias add leaves it.  The flow head forms nine per-tap
    products of 8 steps each (S = 72), joins each (9 roundings, 8 more than c counts) and adds them in
    fp32 (8 roundings): c = 5 + 16.  The bound is derived, not measured; DESIGN.md §22 records the
    printed ratios."""
    x, w, bias = _bound_inputs(case, lin, shape)
    got = lin.bind(w)(x, bias).astype(F64)
    t = lambda a: torch.from_numpy(a).double()
    ref = F.conv2d(t(x), t(w), t(bias), lin.stride, lin.pad).numpy()
    mag = F.conv2d(t(np.abs(x)), t(np.abs(w)), t(np.abs(bias)), lin.stride, lin.pad).numpy()
    bound = (lin.c + 6 * lin.S) * 2.0 ** -24 * mag
    ratio = (np.abs(got - ref) / np.maximum(bound, 1e-300)).max()
    print(f"bound {lin!r} {shape} {case}: max |err| / bound = {ratio:.4f} (S = {lin.S}, c = {lin.c})")
    assert np.isfinite(got).all()
    assert (np.abs(got - ref) <= bound).all()


# ----------------------------------------------------------------------------------------------
# GPU: the GRU half step
# ----------------------------------------------------------------------------------------------
GRU_IN = 320            # with the 128 hidden channels: all 448 input channels
GRU_C = HID + GRU_IN
GRU_SHAPES = [(0, (2, 7, 9)), (1, (1, 13, 5)), (0, (1, 5, 35))]
GRU_SCALE = dict(scale=-26, spread=(6, 4))  # |w x| < 2^-19 * 2^4 * 3: the preactivation stays below 2^-13


def _gru_geo(d):
    return ((1, 5), (0, 2)) if d == 0 else ((5, 1), (2, 0))


def _gru(h, x, d, ws, bs):
    """gru_half_step of numpy inputs; ws = (wz, wr, wq) [128, 448, kh, kw] (None: zero), bs the biases."""
    from eraft_amd import _lib
    k, _ = _gru_geo(d)
    zero = torch.zeros((HID, h.shape[1] + x.shape[1]) + k, device=DEV)
    packed = _lib.gru_pack_weights(*(zero if w is None else _gpu(w) for w in ws))
    return _lib.gru_half_step(_gpu(h), _gpu(x), d, packed, *(_gpu(np.broadcast_to(F32(b), (HID,))) for b in bs)).cpu().numpy()


def _assert_tanh_is_identity(s):
    """In fp64: tanh(s) is closer to s than half an ulp of s, so tanhf(s) correctly rounded is s or
    its neighbour."""
    s64 = s.astype(F64)
    assert (np.abs(s64) <= 2.0 ** -13).all()
    assert (np.abs(np.tanh(s64) - s64) <= 0.5 * np.spacing(np.abs(s)).astype(F64)).all()


def _assert_within_one_ulp(got, s):
    assert np.isfinite(got).all()
    assert (got[s == 0] == 0).all()
    assert (np.abs(got.astype(F64) - s.astype(F64)) <= np.spacing(np.abs(s)).astype(F64)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("cls", "ACD")
@pytest.mark.parametrize("d,shape", GRU_SHAPES[:2])
def test_gru_q_weight_pieces(d, shape, cls):
    """The q path, impulse form.  convz = convr = 0 and bz = br = +100 make z = r = 1 exactly, so
    h' = tanhf(s) with s the candidate's preactivation: one product of a class A (C, D) weight and an
    impulse, scaled to |s| <= 2^-13 where tanh(s) rounds to s or its neighbour.  |h' - s| <= 1 ulp(s);
    a lost 2^-16-class piece moves s by up to 128 ulp.  Class A observes every (128, 448, 5) weight."""
    k, pad = _gru_geo(d)
    B, H, W = shape
    ws = (HID, GRU_C) + k
    w, plan, launches = impulse_launches(cls, 31 + d, (B, GRU_C, H, W), ws, 1, pad, **GRU_SCALE,
                                         max_launches=400 if cls == "A" else 5, full=cls == "A")
    seen = np.zeros(ws, bool)
    for x, sites, exp in launches:
        bx.observe(plan, sites, exp, seen)
        _assert_tanh_is_identity(exp)
        _assert_within_one_ulp(_gru(x[:, :HID], x[:, HID:], d, (None, None, w), (100.0, 100.0, 0.0)), exp)
    assert seen.all() or cls != "A"


@pytest.mark.gpu
@pytest.mark.parametrize("d,shape", GRU_SHAPES)
def test_gru_q_activation_pieces(d, shape):
    """The q path, one-hot form: one-hot weights +-2^e against full-mantissa h and x (class B), until
    every one of the 448 x 5 (channel, tap) pairs has been some output channel's."""
    k, pad = _gru_geo(d)
    B, H, W = shape
    ws = (HID, GRU_C) + k
    xv, pv = bx.operands("B", 41 + d, B * GRU_C * H * W, 1024, GRU_SCALE["scale"], *GRU_SCALE["spread"])
    x = xv.reshape(B, GRU_C, H, W)
    seen, pix = np.zeros((GRU_C, 5), bool), np.zeros((B, H, W), bool)
    for n in range(-(-GRU_C * 5 // HID)):
        o = np.arange(HID)
        j = (n * HID + o) % (GRU_C * 5)        # the (channel, tap) pair of output channel o
        w = np.zeros((HID, GRU_C, 5), F32)
        w[o, j // 5, j % 5] = pv[(n * HID + o) % pv.size]
        seen[j // 5, j % 5] = True
        w = w.reshape(ws)
        exp = bx.expected_conv(x, w, 1, pad)
        pix |= (exp != 0).any(axis=1)
        _assert_tanh_is_identity(exp)
        _assert_within_one_ulp(_gru(x[:, :HID], x[:, HID:], d, (None, None, w), (100.0, 100.0, 0.0)), exp)
    assert seen.all() and pix.all()


def _gate_runs(gate, d, shape, seed):
    """The z (r) path: the kernel's own epilogue on an exactly known preactivation is the comparator.
    Returns (bias run, [(weight run, touched)]): in the bias run the gate's weights are zero and its
    bias is s_o; in a weight run the bias is zero and w[o, ci, tap] = s_o 2^-e meets 2^e impulses in
    x, so the preactivation is s_o exactly at the touched outputs and 0 elsewhere.  h = 1 with zero
    weights on the h channels.  z is observed as h' = (1 - z) h + z tanh(0) = 1 - z (convq = 0); r
    through q's r h input: z = 1 (bz = +100) and convq = 2^-13 at the centre tap of channel o's own
    r h, so h' = tanhf(2^-13 r)."""
    k, pad = _gru_geo(d)
    B, H, W = shape
    rng = np.random.default_rng(seed)
    s = bx.operands("A", seed, HID, 1, 0, 1, 0)[0]                 # full mantissas in 0.5 .. 4
    e = rng.integers(-6, 7, GRU_IN)
    h = np.ones((B, HID, H, W), F32)
    wq = None
    if gate == "r":
        wq = np.zeros((HID, GRU_C) + k, F32)
        wq[np.arange(HID), np.arange(HID), k[0] // 2, k[1] // 2] = 2.0 ** -13
    w = np.zeros((HID, GRU_C) + k, F32)
    w[:, HID:] = (s[:, None].astype(F64) * np.ldexp(1.0, -e)[None, :]).astype(F32)[:, :, None, None]
    ws = (None, w, wq) if gate == "r" else (w, None, None)
    b_run = ((100.0, s, 0.0) if gate == "r" else (s, 0.0, 0.0))
    w_run = ((100.0, 0.0, 0.0) if gate == "r" else (0.0, 0.0, 0.0))
    by_bias = _gru(h, np.zeros((B, GRU_IN, H, W), F32), d, (None, None, wq), b_run)
    plan, runs = bx.ImpulsePlan(B, GRU_IN, H, W, k, 1, pad), []
    while not plan.done():
        sites = plan.next_sites()
        x = bx.impulses((B, GRU_IN, H, W), sites, [2.0 ** e[c] for _, c, _, _ in sites])
        pre = bx.expected_conv(x, w[:, HID:], 1, pad)
        assert ((pre == 0) | (pre == s[None, :, None, None])).all()
        runs.append((_gru(h, x, d, ws, w_run), pre != 0))
    return by_bias, runs


@pytest.mark.gpu
@pytest.mark.parametrize("gate", "zr")
@pytest.mark.parametrize("d,shape", GRU_SHAPES[:2])
def test_gru_gate_weight_pieces(d, shape, gate):
    by_bias, runs = _gate_runs(gate, d, shape, 51 + d)
    zero = F32(0.5) if gate == "z" else np.tanh(F64(2.0 ** -14)).astype(F32)   # the gate at preactivation 0
    touched = np.zeros(by_bias.shape, bool)
    for got, hit in runs:
        touched |= hit
        assert bit_equal(got[hit], by_bias[hit])
        assert np.abs(got[~hit].astype(F64) - zero).max(initial=0) <= np.spacing(zero)
    assert touched.all()   # every output pixel of every channel held the product once
    assert len(np.unique(by_bias)) >= HID // 2   # the comparator does depend on s_o


# ----------------------------------------------------------------------------------------------
# GPU: the mask head fused with the convex upsampling
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("embed", [False, True], ids=["standalone", "offset256"])
@pytest.mark.parametrize("shape", [(1, 8, 32), (2, 7, 9)])
def test_mask_upsample_weight_pieces(shape, embed):
    """The logits cannot be read back, so the kernel's own softmax and combination on an exactly
    known logit is the comparator: hidden is one-hot per pixel (value 2^e_c in channel c, c cycling
    over all 256) and W[o, c] = s_o 2^-e_c, so every logit is s_o exactly, as in a second run with
    W = 0 and bias = s_o.  The two outputs are bit-equal."""
    from eraft_amd import _lib
    B, H, W = shape
    rng = np.random.default_rng(61)
    s = bx.operands("A", 61, 576, 1, 0, 1, 0)[0]
    e = rng.integers(-8, 9, 256)
    w = (s[:, None].astype(F64) * np.ldexp(1.0, -e)[None, :]).astype(F32)
    flow = _gpu(prng.gauss(62, (B, 2, H, W), 3.0))
    off = 256 if embed else 0

    def run(hidden, w, bias):
        buf = torch.full((B, 256 + off, H, W), 1e30, dtype=torch.float32, device=DEV)
        buf[:, off:] = _gpu(hidden)
        return _lib.mask_upsample_forward(buf, off, flow, _lib.mask_upsample_pack_weights(_gpu(w)), _gpu(bias),
                                          0.25).cpu().numpy()

    by_bias = run(np.zeros((B, 256, H, W), F32), np.zeros_like(w), s)
    seen = np.zeros(256, bool)
    n = 0
    while not seen.all():
        c = (np.arange(B * H * W) + n * B * H * W) % 256
        hidden = np.zeros((B, H, W, 256), F32)
        hidden.reshape(-1, 256)[np.arange(c.size), c] = np.ldexp(1.0, e[c])
        seen[c] = True
        n += 1
        assert bit_equal(run(hidden.transpose(0, 3, 1, 2), w, np.zeros(576, F32)), by_bias)
    assert len(np.unique(by_bias)) > by_bias.size // 4


# ----------------------------------------------------------------------------------------------
# GPU: the lookups fused with convc1
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("block", ["CorrBlock", "OnDemandConvCorrBlock"])
def test_lookup_conv_weight_pieces(block):
    """The activations are the block's own lookup, so only the weight side is free: with one non-zero
    full-mantissa weight per output row (the column moving through all 324 from launch to launch) and
    the lookup read back from the unfused call, out[o] = w[o, k] lookup[k] is a single product, and
    the model's six-product value of it is the kernel's, bit for bit.  The lookup values are arbitrary,
    so the partial sums are not exact here and the model rounds them as the MFMA does (bx.mfma_acc).
    Every (o, k) is observed."""
    import eraft_amd
    B, D, H, W, L, R = 2, 32, 16, 24, 4, 4   # the coarsest level is 2 x 3
    C = L * 81
    f1, f2 = prng.gauss(71, (B, D, H, W)), prng.gauss(72, (B, D, H, W))
    coords = _gpu(prng.lookup_coords(73, B, H, W, 24.0))   # wide: every window tap of every level meets the map
    wv = bx.operands("A", 74, 256 * C, 1, 0, 6, 0)[0].reshape(256, C)
    zero = torch.zeros(256, device=DEV)
    seen = np.zeros((256, C), bool)
    with torch.no_grad():
        blk = getattr(eraft_amd, block)(_gpu(f1), _gpu(f2), num_levels=L, radius=R)
        look = blk(coords).cpu().numpy()                      # [B, C, H, W]
        assert np.isfinite(look).all() and (look != 0).any(axis=(0, 2, 3)).all()   # every channel holds products
        small = np.abs(look[look != 0]).min()
        assert small > 2.0 ** -60                             # no subnormal piece or product
        for n in range(C):
            k = (np.arange(256) + n) % C
            w = np.zeros((256, C), F32)
            w[np.arange(256), k] = wv[np.arange(256), k]
            seen[np.arange(256), k] = True
            out = blk.lookup_conv(coords, _gpu(w).view(256, C, 1, 1), zero, relu=False).cpu().numpy()
            x = look[:, k]
            hit = x != 0                                      # elsewhere the output is bias + 0
            exp = np.zeros_like(x)
            exp[hit] = bx.six_model(np.broadcast_to(w[np.arange(256), k][None, :, None, None], x.shape)[hit], x[hit],
                                    mfma=True)
            assert bit_equal(out, exp), n
    assert seen.all()


# ----------------------------------------------------------------------------------------------
# GPU: the non-finite rule
# ----------------------------------------------------------------------------------------------
SPECIAL = [((0, 1, 1), np.inf), ((0, 5, 7), -np.inf), ((1, 1, 7), np.nan), ((1, 5, 1), bx.FLT_MAX),
           ((1, 3, 4), -bx.FLT_MAX)]   # at 2 x 7 x 9: no two of them within one 3x3, 1x5 or 5x1 window


def _plant(x, channels):
    for ((b, y, xx), v), c in zip(SPECIAL, channels):
        x[b, c, y, xx] = v
    return x


def _same_pattern_and_close(got, ref):
    """The non-finite pattern is identical (NaN where NaN, each infinity with its sign) and the finite
    values are within REL_TOL of the largest, the values an FLT_MAX reaches and the others each on
    their own scale."""
    assert got.shape == ref.shape
    assert np.array_equal(np.isnan(got), np.isnan(ref))
    assert np.array_equal(np.isinf(got), np.isinf(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)])
    fin = np.isfinite(ref)
    big = fin & (np.abs(ref) > 1e20)
    for sel in (big, fin & ~big):
        if sel.any():
            assert np.abs(got[sel].astype(F64) - ref[sel]).max() <= REL_TOL * np.abs(ref[sel]).max()


NF_LIN = [Lin("conv", 256, 126, ca=192), Lin("pw", 64, 96), Lin("flow_head", 256, 2, off=256)]


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["activations", "weight"])
@pytest.mark.parametrize("lin", NF_LIN, ids=repr)
def test_non_finite_linear(lin, what):
    """+inf, -inf, NaN and +-FLT_MAX activations at distinct pixels, or an infinite weight (at the
    centre tap, which no border clips): the fp32 convolution on the CPU has the same non-finite
    pattern and the finite values agree within REL_TOL.  The weights are 2^-10-scale so that every
    finite sum stays far from overflow."""
    xs, ws = _lin_shapes(lin, (2, 7, 9))
    x, w, bias = prng.gauss(81, xs), prng.gauss(82, ws, 2.0 ** -10), prng.gauss(83, (lin.cout,), 0.1)
    _plant(x, (3, lin.cin - 1, 17, 30, 8))
    if what == "weight":
        x[~np.isfinite(x)] = 1.0
        w[lin.cout // 2, 5, lin.k // 2, lin.k // 2] = np.inf
        w[0, 9, lin.k // 2, lin.k // 2] = -np.inf
    got = lin.bind(w)(x, bias)
    t = torch.from_numpy
    ref = F.conv2d(t(x), t(w), t(bias), lin.stride, lin.pad).numpy()
    assert not np.isfinite(ref).all()
    _same_pattern_and_close(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("lin", NF_LIN, ids=repr)
def test_flt_max_passes_unchanged(lin):
    """The truncated-hi guard: +-FLT_MAX (and the values just inside the guard's range) under a
    one-hot weight 1.0 come out bit for bit."""
    xs, ws = _lin_shapes(lin, (2, 7, 9))
    x = bx.operands("B", 91, int(np.prod(xs)), 1, 0, 12, 0)[0].reshape(xs).copy()
    near = np.array([0x7F7FFFFF, 0x7F7F8000, 0x7F7F7FFF, 0xFF7FFFFF, 0xFF7FC000], np.uint32).view(F32)
    for i, v in enumerate(near):
        x[i % 2, :, (2 * i) % 7, (3 * i) % 9] = v
    for n in range(-(-lin.k * lin.k // lin.cout)):
        w = bx.onehot_weights(lin.cout, lin.cin, lin.k, n, np.ones(lin.cout, F32))
        exp = bx.expected_conv(x, w, lin.stride, lin.pad)
        assert (np.abs(exp) == bx.FLT_MAX).any()
        assert bit_equal(lin.bind(w)(x), exp)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["activations", "weight"])
@pytest.mark.parametrize("d", [0, 1])
def test_non_finite_gru(d, what):
    """The half step against the fp32 op chain on the CPU (test_gru._chain): specials in x and in h,
    or infinite gate and candidate weights at the centre tap."""
    from test_gru import _chain
    k, _ = _gru_geo(d)
    B, H, W = 2, 7, 9
    h = np.tanh(prng.gauss(84, (B, HID, H, W)).astype(F64)).astype(F32)
    x = prng.gauss(85, (B, GRU_IN, H, W))
    ws = [prng.gauss(86 + i, (HID, GRU_C) + k, 2.0 ** -10) for i in range(3)]
    bs = [prng.gauss(89 + i, (HID,), 0.1) for i in range(3)]
    if what == "activations":
        for ((b, y, xx), v), c, in_h in zip(SPECIAL, (3, 100, 17, 30, 8), (False, True, False, True, False)):
            (h if in_h else x)[b, c, y, xx] = v
    else:
        ws[0][3, 200, k[0] // 2, k[1] // 2] = np.inf
        ws[1][5, 300, k[0] // 2, k[1] // 2] = -np.inf
        ws[2][7, 5, k[0] // 2, k[1] // 2] = -np.inf
    got = _gru(h, x, d, ws, bs)
    t = torch.from_numpy
    ref = _chain(t(h), t(x), [t(w).reshape(HID, GRU_C, 5) for w in ws], [t(b) for b in bs], d).numpy()
    assert what == "weight" or not np.isfinite(ref).all()
    _same_pattern_and_close(got, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["activations", "weight"])
def test_non_finite_mask_upsample(what):
    """The mask head and the convex upsampling against the fp32 chain on the CPU (0.25 (W hidden + b),
    softmax over the nine taps, the combination of the 3x3 flow window)."""
    from eraft_amd import _lib
    from eraft_amd.model import ERAFT
    B, H, W = 2, 7, 9
    hidden = np.maximum(prng.gauss(94, (B, 256, H, W)), 0.0).astype(F32)
    w, bias = prng.gauss(95, (576, 256), 2.0 ** -10), prng.gauss(96, (576,), 0.5)
    flow = prng.gauss(97, (B, 2, H, W), 3.0)
    if what == "activations":
        _plant(hidden, (3, 255, 17, 30, 8))
    else:
        w[100, 7], w[300, 200] = np.inf, -np.inf
    got = _lib.mask_upsample_forward(_gpu(hidden), 0, _gpu(flow), _lib.mask_upsample_pack_weights(_gpu(w)),
                                     _gpu(bias), 0.25).cpu().numpy()
    t = torch.from_numpy
    mask = 0.25 * F.conv2d(t(hidden), t(w).view(576, 256, 1, 1), t(bias))
    ref = ERAFT.upsample_flow(t(flow), mask).numpy()
    assert not np.isfinite(ref).all()
    _same_pattern_and_close(got, ref)
