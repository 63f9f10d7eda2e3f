"""The training tail with the mask head inside it (csrc/corr_mask_loss.hip,
include/corr_mi355x_train_head.h, SequenceLoss.add_hidden, ERAFT.fuse_mask_loss) against the fp64
truth of tests/_mask_head_ref.py, which also states the cases' input conditions.

Bars.  P = max|pred64| of the case, G = sum_i gamma^(n-1-i):
  loss          |d| <= 1e-5 P G                  (test_sequence_loss.py's bar)
  epe           |d| <= sqrt(2) 1e-5 P
  counts        exact
  fused vs corr_sequence_loss over the prediction corr_mask_upsample_forward stores: counts exact;
                loss and EPE sums within 2 * 16 * 2^-24 relative (their terms are all >= 0, so the
                sum is the sum of absolute terms): each side groups at most 16 fp32 terms per thread
  dz, dflow     within 1e-4 of max|ref| per tensor
  hidden.grad, weight.grad, bias.grad   within 1e-3 of max|ref| per tensor (MIOpen's part)
The tests print their measured figures; DESIGN.md §32 records them.
"""
import ctypes
import gc
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _loss_ref as R
import _mask_head_ref as M
from _util import DEV, norm_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "corr_mi355x_train_head.h")
G = sum(M.weights())

# (shape, sigma of the ground truth, max_flow, no_valid)
CASES = [("nopad", 2.0, 400.0, False), ("cut", 2.0, 400.0, False), ("rows", 2.0, 400.0, False),
         ("lane", 2.0, 400.0, False), ("odd", 2.0, 400.0, False), ("cut", 30.0, 400.0, False),
         ("cut", 2.0, 5.0, False), ("nopad", 2.0, 400.0, True)]
IDS = [f"{s}-sigma{g:g}-maxflow{m:g}" + ("-novalid" if nv else "") for s, g, m, nv in CASES]
WINDOWS = ("own", "slice")


@pytest.fixture(scope="module")
def lib():
    from eraft_amd.build import build_library
    from eraft_amd import _lib
    build_library()
    return _lib.load()


# ----------------------------------------------------------------------------------------------
# no GPU
# ----------------------------------------------------------------------------------------------
def _declared():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(corr_[a-z_]+)\s*\(", src)))


def test_head_header_declares_the_train_head_exports(lib):
    from eraft_amd import _lib
    assert sorted(_lib.TRAIN_HEAD_EXPORTS) == _declared() and len(_lib.TRAIN_HEAD_EXPORTS) == 3
    for other in (_lib.EXPORTS, _lib.TRAIN_EXPORTS, _lib.ENC_PREC_EXPORTS):
        assert not set(_lib.TRAIN_HEAD_EXPORTS) & set(other)
    for name in _lib.TRAIN_HEAD_EXPORTS:
        assert hasattr(lib, name), name
        want = ctypes.c_size_t if name.endswith("_workspace") else ctypes.c_int
        assert getattr(lib, name).restype is want, name
    assert lib.corr_version() == 202


def test_build_lists_the_header_and_the_source():
    from eraft_amd import build
    assert "corr_mask_loss.hip" in build.SOURCES
    assert any(h.endswith("corr_mi355x_train_head.h") for h in build.HEADERS)


def test_workspace_size(lib):
    for bad in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (-1, 4, 8)):
        assert lib.corr_mask_upsample_loss_workspace(*bad) == 0, bad
    # the backward's 18 S planes; the forward's 48-byte partials (one per 2 blocks of 16 pixels) fit
    assert lib.corr_mask_upsample_loss_workspace(2, 9, 70) == 2 * 18 * 9 * 70 * 4
    assert lib.corr_mask_upsample_loss_workspace(1, 1, 1) == 72 >= 48


_P = 256   # a well-aligned non-null pointer that is never dereferenced
_BIG = 1 << 40


def _refused(lib, rc, msg):
    err = lib.corr_last_error().decode()
    return rc == -1 and msg in err and len(err) > len(msg)


def test_refusals(lib):
    """One refusal per rule, each CORR_EINVAL with a message: any HIP call would fail differently
    on a machine without a GPU."""
    def fwd(hidden=_P, hc=256, off=0, flow=_P, packed=_P, bias=_P, ms=0.25, gt=_P, valid=_P, N=2, h=9, w=70, H=50,
            W=545, mf=400.0, out=_P, ws=_P, wsb=_BIG):
        return lib.corr_mask_upsample_loss(hidden, hc, off, flow, packed, bias, ms, gt, valid, N, h, w, H, W, mf, 1,
                                           out, ws, wsb, None)

    def bwd(hidden=_P, hc=256, off=0, flow=_P, packed=_P, bias=_P, ms=0.25, gt=_P, valid=_P, scale=_P, N=2, h=9,
            w=70, H=50, W=545, mf=400.0, dflow=_P, dz=_P, ws=_P, wsb=_BIG):
        return lib.corr_mask_upsample_loss_bwd(hidden, hc, off, flow, packed, bias, ms, gt, valid, scale, N, h, w, H,
                                               W, mf, dflow, dz, ws, wsb, None)

    need = lib.corr_mask_upsample_loss_workspace(2, 9, 70)
    common = ("hidden", "flow", "packed", "bias", "gt", "valid")
    for call, ptrs in ((fwd, common), (bwd, common + ("scale", "dflow", "dz"))):
        for name in ptrs:
            assert _refused(lib, call(**{name: None}), f"{name} is NULL"), name
            assert _refused(lib, call(**{name: _P + 2}), f"{name} is not 4-byte aligned"), name
        assert _refused(lib, call(packed=_P + 8), "packed is not 16-byte aligned")
        assert _refused(lib, call(hc=511, off=256), "must lie in [0, hidden_channels)")
        assert _refused(lib, call(off=-1), "must lie in [0, hidden_channels)")
        assert not _refused(lib, call(hc=512, off=256, ws=None), "must lie in")
        for dim in ("N", "h", "w"):
            assert _refused(lib, call(**{dim: 0}), "N, h, w must be >= 1"), dim
        assert _refused(lib, call(H=73), "H, W must be <= 8h, 8w")
        assert _refused(lib, call(W=561), "H, W must be <= 8h, 8w")
        assert _refused(lib, call(H=0), "H, W must be >= 1")
        assert _refused(lib, call(W=-3), "H, W must be >= 1")
        assert _refused(lib, call(wsb=need - 1), "workspace of")
        assert not _refused(lib, call(wsb=need, ws=None), "workspace of")
        assert _refused(lib, call(ws=None), "workspace is NULL")
        assert _refused(lib, call(ws=_P + 4), "workspace is not 8-byte aligned")
        for mf in (0.0, -1.0, float("inf"), float("nan")):
            assert _refused(lib, call(mf=mf), "max_flow must be finite and positive"), mf
        assert _refused(lib, call(ms=float("nan")), "mask_scale must be finite")
        # 576 * 1821 * 2048 >= 2^31 dz elements; one coarse row fewer passes on to the next check
        assert _refused(lib, call(N=1, h=1821, w=2048, H=8, W=8), "too large")
        assert _refused(lib, call(N=1, h=1820, w=2048, H=8, W=8, wsb=16), "workspace of")
        # 2 * 4096 * 512 * 512 = 2^31 elements of hidden
        assert _refused(lib, call(N=2, hc=4096, h=512, w=512, H=8, W=8), "N*hidden_channels*h*w too large")
        assert _refused(lib, call(N=2, hc=4095, h=512, w=512, H=8, W=8, wsb=16), "workspace of")
    assert _refused(lib, fwd(out=None), "out is NULL")
    assert _refused(lib, fwd(out=_P + 4), "out is not 8-byte aligned")


def _check_forward(what, case, loss, metrics, t):
    """The forward bars of the module docstring; prints the figures."""
    bar = 1e-5 * case.scale * G
    loss = loss.detach()
    err = abs(float(loss) - t.loss)
    print(f"{what} {case.name}: loss {float(loss):.9g}, error {err:.2e} (bar {bar:.2e})")
    assert err <= bar
    if t.n_valid == 0:
        assert float(loss) == 0.0 and all(math.isnan(float(metrics[k])) for k in ("epe", "1px", "3px", "5px"))
        return
    e = abs(float(metrics["epe"]) - t.epe)
    print(f"{what} {case.name}: epe error {e:.2e} (bar {math.sqrt(2) * 1e-5 * case.scale:.2e})")
    assert e <= math.sqrt(2) * 1e-5 * case.scale
    for k, c in zip(("1px", "3px", "5px"), t.counts):
        assert round(float(metrics[k]) * t.n_valid) == c and abs(float(metrics[k]) - c / t.n_valid) < 1e-6, k


def _conv(case, device="cpu", dtype=torch.float32):
    conv = torch.nn.Conv2d(256, 576, 1)
    with torch.no_grad():
        conv.weight.copy_(case.weight)
        conv.bias.copy_(case.bias)
    return conv.to(device=device, dtype=dtype)


def test_the_input_conditions_hold_on_the_cpu():
    """Every case's kink and threshold bands remove at most 1 % of the sub-pixels (build() asserts
    it; here the fractions are printed), before any GPU call."""
    for args in CASES:
        case = M.build(*args)
        print(f"{case.name}: {case.removed:.3%} of the sub-pixels removed, max|pred64| {case.scale:.3f}")
        assert case.removed <= 0.01


@pytest.mark.parametrize("args", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_cpu_add_hidden_against_fp64(args, dtype):
    """add_hidden on CPU tensors (the torch composition in loss.py)."""
    from eraft_amd import SequenceLoss
    case = M.build(*args)
    t = M.truth(case)
    conv = _conv(case, dtype=dtype)
    crit = SequenceLoss(case.gt.to(dtype), case.valid.to(dtype), M.GAMMA, case.max_flow)
    hiddens = [x.clone().to(dtype).requires_grad_(True) for x in case.hiddens]
    flows = [f.clone().to(dtype).requires_grad_(True) for f in case.flows]
    for i in reversed(range(M.ITERS)):
        crit.add_hidden(conv, hiddens[i], flows[i], i, M.ITERS, M.pads(case.geo))
    loss, m = crit.result()
    _check_forward("cpu add_hidden", case, loss, m, t)
    if dtype == torch.float64 and t.n_valid:
        loss.backward()
        for i in range(M.ITERS):
            assert norm_rel(flows[i].grad.numpy(), t.dflows[i]) < 1e-9
            assert norm_rel(hiddens[i].grad.numpy(), t.dhiddens[i]) < 1e-9
        assert norm_rel(conv.weight.grad.numpy(), t.dweight) < 1e-9 and norm_rel(conv.bias.grad.numpy(), t.dbias) < 1e-9


def test_add_hidden_refuses_bad_geometry():
    from eraft_amd import SequenceLoss
    case = M.build(*CASES[0])
    conv = _conv(case)
    crit = SequenceLoss(case.gt, case.valid)
    with pytest.raises(ValueError, match="do not upsample"):
        crit.add_hidden(conv, case.hiddens[0], case.flows[0], 0, 1, (8, 0))
    with pytest.raises(ValueError, match="do not upsample"):
        crit.add_hidden(conv, case.hiddens[0][..., :-1], case.flows[0], 0, 1)
    with pytest.raises(ValueError, match="index"):
        crit.add_hidden(conv, case.hiddens[0], case.flows[0], 1, 1)
    crit.add_hidden(conv, case.hiddens[0], case.flows[0], 0, 1)
    with pytest.raises(ValueError, match="twice"):
        crit.add_hidden(conv, case.hiddens[0], case.flows[0], 0, 1)


def test_switch_follows_the_environment_and_defaults_to_off():
    from eraft_amd.model import ERAFT
    assert ERAFT.fuse_mask_loss is (os.environ.get("ERAFT_AMD_FUSE_MASK_LOSS", "0") == "1")


def test_model_on_the_cpu_with_the_attribute_set():
    """ERAFT.forward(..., sequence_loss=crit) on CPU tensors with fuse_mask_loss set on the instance:
    add_hidden's torch composition, i.e. the unswitched step's loss, metrics and gradients."""
    from eraft_amd import SequenceLoss
    from _train_ref import Config, inputs, make_model, substituted
    cfg = Config(H=120, W=150, B=1, iters=2)  # the padder pads to 128x160
    im1, im2, gt, _, _ = (None if a is None else torch.from_numpy(a) if isinstance(a, np.ndarray) else a
                          for a in inputs(cfg))
    valid = torch.from_numpy(np.asarray(R.VALID_VALUES, np.float32)[
        (R.prng.uniform(5, (cfg.B, cfg.H, cfg.W)) * 4).astype(np.int64).clip(0, 3)])
    with substituted(torch.float32, torch_upsample=False):
        model = make_model(cfg)
        crit = SequenceLoss(gt, valid)
        low, none = model(im1, im2, iters=cfg.iters, sequence_loss=crit)
        ref, ref_m = crit.result()
        ref.backward()
        g_ref = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        model.fuse_mask_loss = True
        seen = []
        crit = SequenceLoss(gt, valid)
        crit.add_hidden = lambda *a, _f=crit.add_hidden, **k: (seen.append(a[0]), _f(*a, **k))[1]
        low2, none2 = model(im1, im2, iters=cfg.iters, sequence_loss=crit)
        loss, m = crit.result()
        loss.backward()
    assert none == none2 == [] and torch.equal(low, low2)
    assert len(seen) == cfg.iters and all(c is model.update_block.mask[2] for c in seen)
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
    assert all(abs(float(m[k]) - float(ref_m[k])) <= 1e-6 for k in ref_m)
    got = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert got.keys() == g_ref.keys() and len(got) > 50
    scale = max(float(g.abs().max()) for g in g_ref.values())
    assert max(float((got[n] - g_ref[n]).abs().max()) for n in got) <= 1e-3 * scale


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu_lib(lib):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return lib


def _hidden(x, window, grad=False):
    """(the leaf, hidden, the buffer the kernel reads, offset): hidden as its own tensor, or as
    channels 256 .. 511 of a 512-channel buffer whose other channels hold NaN."""
    x = x.to(DEV)
    if window == "own":
        x = x.clone().requires_grad_(grad)
        return x, x, x, 0
    buf = torch.full((x.shape[0], 512, *x.shape[2:]), float("nan"), device=DEV)
    buf[:, 256:] = x
    buf.requires_grad_(grad)
    return buf, buf[:, 256:], buf, 256


def _leaf_grad(leaf, window):
    return leaf.grad if window == "own" else leaf.grad[:, 256:]


def _frame(case):
    return case.gt.to(DEV), case.valid.to(DEV)


def _criterion(case, conv, hiddens, flows, gt, valid, total=M.ITERS, only=None):
    from eraft_amd import SequenceLoss
    crit = SequenceLoss(gt, valid, M.GAMMA, case.max_flow)
    for i in (range(total) if only is None else [only]):
        crit.add_hidden(conv, hiddens[i], flows[i], i, total, M.pads(case.geo))
    return crit.result()


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("args", CASES, ids=IDS)
def test_forward_parity_against_fp64(gpu_lib, args, window):
    from eraft_amd import _lib
    from eraft_amd.upsample import _mask_pack
    case = M.build(*args)
    t = M.truth(case)
    conv, (gt, valid) = _conv(case, DEV), _frame(case)
    hid = [_hidden(x, window) for x in case.hiddens]
    flows = [f.to(DEV) for f in case.flows]
    ph, pw = M.pads(case.geo)
    with torch.no_grad():
        loss, m = _criterion(case, conv, [x[1] for x in hid], flows, gt, valid)
        packed, bias = _mask_pack(conv)
        per = []
        for (_, _, buf, off), flow in zip(hid, flows):
            stats = _lib.mask_upsample_loss(buf, off, flow, packed, bias, M.SCALE, gt, valid, case.max_flow, True)
            pred = _lib.mask_upsample_forward(buf, off, flow, packed, bias, M.SCALE)[..., ph:, pw:].contiguous()
            per.append((stats.cpu().numpy(), _lib.sequence_loss(pred, gt, valid, case.max_flow, True).cpu().numpy(),
                        pred.cpu().numpy()))
    assert loss.is_cuda and loss.dim() == 0 and all(v.is_cuda and v.dim() == 0 for v in m.values())
    _check_forward(f"add_hidden[{window}]", case, loss, m, t)
    for i, (s, s_ref, pred) in enumerate(per):
        assert norm_rel(pred, t.preds[i]) <= 1e-5
        assert all(float(x) == int(x) for x in s[[1, 3, 4, 5]])
        assert int(s[1]) == t.n_valid and [int(x) for x in s[[1, 3, 4, 5]]] == [int(x) for x in s_ref[[1, 3, 4, 5]]]
        if i == M.ITERS - 1:
            assert (int(s[3]), int(s[4]), int(s[5])) == t.counts
        for k, what in ((0, "loss sum"), (2, "EPE sum")):
            rel = abs(s[k] - s_ref[k]) / s_ref[k] if s_ref[k] else abs(s[k])
            print(f"{case.name}[{window}] iteration {i}: {what} vs the stored prediction's {rel:.2e} "
                  f"(bar {2 * 16 * 2.0 ** -24:.2e})")
            assert rel <= 2 * 16 * 2.0 ** -24


def _raw_bwd(lib, case, buf, off, flow, conv, gt, valid, coef):
    """corr_mask_upsample_loss_bwd over NaN-prefilled outputs -> (dflow, dz)."""
    from eraft_amd.upsample import _mask_pack
    N, h, w, H, W = case.geo
    packed, bias = _mask_pack(conv)
    scale = torch.full((1,), coef, dtype=torch.float32, device=DEV)
    dflow = torch.full((N, 2, h, w), float("nan"), device=DEV)
    dz = torch.full((N, 576, h, w), float("nan"), device=DEV)
    nbytes = lib.corr_mask_upsample_loss_workspace(N, h, w)
    ws = torch.full(((nbytes + 7) // 8,), float("nan"), dtype=torch.float64, device=DEV)
    rc = lib.corr_mask_upsample_loss_bwd(buf.data_ptr(), buf.shape[1], off, flow.data_ptr(), packed.data_ptr(),
                                         bias.data_ptr(), M.SCALE, gt.data_ptr(), valid.data_ptr(), scale.data_ptr(),
                                         N, h, w, H, W, case.max_flow, dflow.data_ptr(), dz.data_ptr(), ws.data_ptr(),
                                         nbytes, torch.cuda.current_stream().cuda_stream)
    assert rc == 0, lib.corr_last_error().decode(errors="replace")
    return dflow, dz


@pytest.mark.gpu
@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("args", CASES[:7], ids=IDS[:7])
def test_backward_parity_against_fp64_autograd(gpu_lib, args, window):
    case = M.build(*args)
    t = M.truth(case)
    conv, (gt, valid) = _conv(case, DEV), _frame(case)
    hid = [_hidden(x, window, grad=True) for x in case.hiddens]
    flows = [f.to(DEV).requires_grad_(True) for f in case.flows]
    loss, _ = _criterion(case, conv, [x[1] for x in hid], flows, gt, valid)
    loss.backward()
    gone = torch.from_numpy(M.cropped(case.geo)).to(DEV)
    for i, wt in enumerate(M.weights()):
        with torch.no_grad():
            dflow, dz = _raw_bwd(gpu_lib, case, hid[i][2].detach(), hid[i][3], flows[i].detach(), conv, gt, valid,
                                 np.float32(wt / case.gt.numel()))
        assert torch.equal(dz[:, gone], torch.zeros_like(dz[:, gone])), "dz is not 0 where the crop removes the sub-pixel"
        assert torch.equal(dflow, flows[i].grad)
        for what, got, ref, bar in (("dz", dz, t.dzs[i], 1e-4), ("dflow", flows[i].grad, t.dflows[i], 1e-4),
                                    ("dhidden", _leaf_grad(hid[i][0], window), t.dhiddens[i], 1e-3)):
            e = norm_rel(got.cpu().numpy(), ref)
            print(f"{case.name}[{window}] iteration {i}: {what} {e:.2e} of max|ref| (bar {bar:.0e})")
            assert e <= bar, (what, i)
        if window == "slice":
            rest = hid[i][0].grad[:, :256]
            assert torch.equal(rest, torch.zeros_like(rest))
    for what, got, ref in (("dweight", conv.weight.grad, t.dweight), ("dbias", conv.bias.grad, t.dbias)):
        e = norm_rel(got.cpu().numpy(), ref)
        print(f"{case.name}[{window}]: {what} {e:.2e} of max|ref| (bar 1e-03)")
        assert e <= 1e-3, what


@pytest.mark.gpu
def test_upstream_scalar_and_iteration_weights(gpu_lib):
    """(3 loss).backward() over n = 3 terms = 3 x the weighted sum of the single terms' gradients."""
    case = M.build(*CASES[1])
    gt, valid = _frame(case)
    single, dw, db = [], 0.0, 0.0
    for i, wt in enumerate(M.weights()):
        conv = _conv(case, DEV)
        x = case.hiddens[i].to(DEV).requires_grad_(True)
        f = case.flows[i].to(DEV).requires_grad_(True)
        loss, _ = _criterion(case, conv, {i: x}, {i: f}, gt, valid, total=M.ITERS, only=i)  # weight gamma^(n-1-i)
        one, _ = _criterion(case, conv, [x], [f], gt, valid, total=1)                        # weight 1
        assert abs(float(loss.detach()) - wt * float(one.detach())) <= 1e-6 * abs(float(one.detach()))
        one.backward()
        single.append((x.grad.double(), f.grad.double()))
        dw, db = dw + wt * conv.weight.grad.double(), db + wt * conv.bias.grad.double()
    conv = _conv(case, DEV)
    xs = [x.to(DEV).requires_grad_(True) for x in case.hiddens]
    fs = [f.to(DEV).requires_grad_(True) for f in case.flows]
    loss, _ = _criterion(case, conv, xs, fs, gt, valid)
    (3 * loss).backward()
    pairs = [(f"dhidden {i}", xs[i].grad, 3 * wt * single[i][0]) for i, wt in enumerate(M.weights())]
    pairs += [(f"dflow {i}", fs[i].grad, 3 * wt * single[i][1]) for i, wt in enumerate(M.weights())]
    pairs += [("dweight", conv.weight.grad, 3 * dw), ("dbias", conv.bias.grad, 3 * db)]
    for what, got, ref in pairs:
        e = norm_rel(got.cpu().numpy(), ref.cpu().numpy())
        print(f"{what}: {e:.2e}")
        assert e <= 1e-4, what


@pytest.mark.gpu
def test_second_order_is_refused(gpu_lib):
    case = M.build(*CASES[0])
    conv, (gt, valid) = _conv(case, DEV), _frame(case)
    f = case.flows[0].to(DEV).requires_grad_(True)
    loss, _ = _criterion(case, conv, [case.hiddens[0].to(DEV)], [f], gt, valid, total=1)
    (g,) = torch.autograd.grad(loss, f, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


def _bits(a):
    return a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int64)


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu_lib):
    case = M.build(*CASES[1])
    runs = []
    for _ in range(2):
        conv, (gt, valid) = _conv(case, DEV), _frame(case)
        xs = [x.to(DEV).requires_grad_(True) for x in case.hiddens]
        fs = [f.to(DEV).requires_grad_(True) for f in case.flows]
        loss, m = _criterion(case, conv, xs, fs, gt, valid)
        loss.backward()
        with torch.no_grad():
            raw = _raw_bwd(gpu_lib, case, xs[0].detach(), 0, fs[0].detach(), conv, gt, valid, np.float32(1e-4))
        runs.append([loss.detach().double(), *(m[k] for k in sorted(m)), *(f.grad for f in fs), *raw])
    for a, b in zip(*runs):
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["gt-under-valid-0", "hidden-kept", "hidden-cropped"])
def test_non_finite_inputs_poison_as_the_torch_chain(gpu_lib, where):
    """A NaN in gt under valid = 0 poisons the sum (v is multiplied in); one in hidden poisons it
    where the crop keeps the coarse pixel and not where it removes it: NaN-ness equals the fp32
    torch chain's."""
    case = M.build("rows")  # pads 24 and 24: coarse rows and columns 0..2 are removed
    hiddens, gt, valid = [x.clone() for x in case.hiddens], case.gt.clone(), case.valid.clone()
    if where == "gt-under-valid-0":
        valid[0, 5, 7] = 0.0
        gt[0, 1, 5, 7] = float("nan")
    elif where == "hidden-kept":
        hiddens[1][0, 100, 4, 5] = float("nan")
    else:
        hiddens[1][0, 100, 1, 5] = float("nan")
        hiddens[2][0, 7, 5, 2] = float("nan")
    chain = R.torch_loss([M.pred64(x, f, case.weight, case.bias, case.geo) for x, f in zip(hiddens, case.flows)],
                         gt, valid)
    assert bool(torch.isnan(chain)) == (where != "hidden-cropped")
    conv = _conv(case, DEV)
    with torch.no_grad():
        fused, _ = _criterion(case, conv, [x.to(DEV) for x in hiddens], [f.to(DEV) for f in case.flows], gt.to(DEV),
                              valid.to(DEV))
    assert bool(torch.isnan(fused)) == bool(torch.isnan(chain))
    if where == "hidden-cropped":
        assert abs(float(fused) - float(chain)) <= 1e-5 * case.scale * G


@pytest.mark.gpu
def test_pack_follows_an_in_place_parameter_update(gpu_lib):
    """An optimizer step updates the parameters in place: the next call packs the new weights, and
    its loss is that of a fresh module holding them, bit for bit."""
    case = M.build(*CASES[1])
    conv, (gt, valid) = _conv(case, DEV), _frame(case)
    xs, fs = [x.to(DEV) for x in case.hiddens], [f.to(DEV) for f in case.flows]
    with torch.no_grad():
        before, _ = _criterion(case, conv, xs, fs, gt, valid)
        conv.weight.mul_(0.5)
        conv.bias.add_(0.25)
        after, _ = _criterion(case, conv, xs, fs, gt, valid)
        fresh = torch.nn.Conv2d(256, 576, 1).to(DEV)
        fresh.weight.copy_(conv.weight)
        fresh.bias.copy_(conv.bias)
        want, _ = _criterion(case, fresh, xs, fs, gt, valid)
    assert float(after) != float(before) and torch.equal(_bits(after), _bits(want))


@pytest.mark.gpu
def test_other_heads_take_the_torch_composition(gpu_lib):
    """A head without a bias is not the kernel's: add_hidden runs scale * conv(hidden) and add_upsampled."""
    case = M.build(*CASES[0])
    gt, valid = _frame(case)
    conv = torch.nn.Conv2d(256, 576, 1, bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(case.weight)
        xs, fs = [x.to(DEV) for x in case.hiddens], [f.to(DEV) for f in case.flows]
        got, _ = _criterion(case, conv, xs, fs, gt, valid)
        from eraft_amd import SequenceLoss
        crit = SequenceLoss(gt, valid, M.GAMMA, case.max_flow)
        for i in range(M.ITERS):
            crit.add_upsampled(fs[i], M.SCALE * conv(xs[i]), i, M.ITERS, M.pads(case.geo))
        want, _ = crit.result()
    assert torch.equal(_bits(got), _bits(want))


# ---- buffer and stream discipline of the two launching entry points (test_core_discipline.py) ----
from test_core_discipline import Arena, _clones, _ordered_on_the_callers_stream, _run_case, _same, gpu, side  # noqa: E402,F401

DISCIPLINE_SHAPES = ("cut", "rows")
_DATA = {}


def _shared(shape):
    if shape not in _DATA:
        from eraft_amd import _lib
        case = M.build(shape)
        _DATA[shape] = (case.geo, case.hiddens[0].to(DEV), case.flows[0].to(DEV),
                        _lib.mask_upsample_pack_weights(case.weight.to(DEV)), case.bias.to(DEV), case.gt.to(DEV),
                        case.valid.to(DEV), torch.full((1,), 0.37, device=DEV))
    return _DATA[shape]


def _ok(lib, rc):
    assert rc == 0, f"rc {rc}: {lib.corr_last_error().decode(errors='replace')}"


def _s():
    return torch.cuda.current_stream().cuda_stream


def _head_inputs(A, shape):
    geo, hidden, flow, packed, bias, gt, valid, scale = _shared(shape)
    ins = [A.inp(n, v) for n, v in zip(("hidden", "flow"), (hidden, flow))]
    ins.append(A.inp("packed", packed, align16=True))
    ins += [A.inp(n, v) for n, v in zip(("bias", "gt", "valid", "scale"), (bias, gt, valid, scale))]
    return (geo, *ins)


def case_mask_upsample_loss(A, shape):
    from eraft_amd import _lib
    lib = _lib.load()
    (N, h, w, H, W), hidden, flow, packed, bias, gt, valid, _ = _head_inputs(A, shape)
    out = A.out("out", (12,))  # six fp64 words
    wp, wn = A.ws("workspace", lib.corr_mask_upsample_loss_workspace(N, h, w))

    def call():
        _ok(lib, lib.corr_mask_upsample_loss(hidden.data_ptr(), 256, 0, flow.data_ptr(), packed.data_ptr(),
                                             bias.data_ptr(), M.SCALE, gt.data_ptr(), valid.data_ptr(), N, h, w, H, W,
                                             400.0, 1, out.data_ptr(), wp, wn, _s()))
    return call, _clones(out=out)


def case_mask_upsample_loss_bwd(A, shape):
    from eraft_amd import _lib
    lib = _lib.load()
    (N, h, w, H, W), hidden, flow, packed, bias, gt, valid, scale = _head_inputs(A, shape)
    dflow, dz = A.out("dflow", (N, 2, h, w)), A.out("dz", (N, 576, h, w))
    wp, wn = A.ws("workspace", lib.corr_mask_upsample_loss_workspace(N, h, w))

    def call():
        _ok(lib, lib.corr_mask_upsample_loss_bwd(hidden.data_ptr(), 256, 0, flow.data_ptr(), packed.data_ptr(),
                                                 bias.data_ptr(), M.SCALE, gt.data_ptr(), valid.data_ptr(),
                                                 scale.data_ptr(), N, h, w, H, W, 400.0, dflow.data_ptr(),
                                                 dz.data_ptr(), wp, wn, _s()))
    return call, _clones(dflow=dflow, dz=dz)


ENTRIES = {"corr_mask_upsample_loss": case_mask_upsample_loss, "corr_mask_upsample_loss_bwd": case_mask_upsample_loss_bwd}
DISCIPLINE = {f"{e}[{s}]": (lambda A, f=f, s=s: f(A, s)) for e, f in ENTRIES.items() for s in DISCIPLINE_SHAPES}
_PLAIN = {}


def _plain(name):
    if name not in _PLAIN:
        _PLAIN[name] = {k: v.cpu() for k, v in _run_case(DISCIPLINE[name], Arena()).items()}
    return _PLAIN[name]


def test_discipline_covers_every_launching_entry_point():
    from eraft_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    with_stream = {n for n, a in re.findall(r"\b(corr_[a-z_]+)\s*\(([^;]*)\)\s*;", src) if re.search(r"void\s*\*\s*stream\b", a)}
    assert with_stream == set(ENTRIES) == {n for n in _lib.TRAIN_HEAD_EXPORTS if not n.endswith("_workspace")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISCIPLINE))
def test_writes_stay_inside(gpu, name):
    """Outputs and workspace in guarded windows over a NaN prefill: guards intact, every output (all
    of dz, 0 exactly where the crop removes the sub-pixel) written, results those of the plain call."""
    arena = Arena(guard_out=True, guard_ws=True)
    got = _run_case(DISCIPLINE[name], arena)
    arena.check()
    _same(_plain(name), got, name)
    if "dz" in got:
        gone = torch.from_numpy(M.cropped(M.SHAPES[name[name.index("[") + 1:-1]])).to(DEV)
        assert gone.any() and torch.equal(got["dz"][:, gone], torch.zeros_like(got["dz"][:, gone]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISCIPLINE))
def test_workspace_is_as_large_as_claimed_and_needs_no_initialisation(gpu, name):
    arena = Arena(guard_ws=True)
    got = _run_case(DISCIPLINE[name], arena)
    assert arena.n_ws == 1
    arena.check()
    _same(_plain(name), got, name)


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("name", list(DISCIPLINE))
def test_results_do_not_depend_on_memory_outside_the_inputs(gpu, name, misalign):
    arena = Arena(guard_in=True, misalign=misalign)
    got = _run_case(DISCIPLINE[name], arena)
    arena.check()
    _same(_plain(name), got, name, clean=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISCIPLINE))
def test_work_is_ordered_on_the_callers_stream(gpu, side, name):
    _ordered_on_the_callers_stream(DISCIPLINE[name], _plain(name), side, name)


# ---- peak memory of the tail ----
@pytest.mark.gpu
def test_tail_peak_memory_is_lower_by_the_saved_masks(gpu_lib):
    """(2, 24, 32 -> 192, 256), 6 iterations, forward + backward to every (hidden_i, flow_i) and to
    one shared head: today's path saves six masks for backward, add_hidden none, and both hold one
    transient mask-sized gradient; two masks of margin cover the allocator's rounding.

    A leaf's gradient is dropped as it arrives (a post-accumulate hook, which counts it), as the
    update block consumes dhidden and dflow in a step: six accumulated dhidden are 2.67 masks that
    no step holds, and they sit in the new path's peak (the end of its backward) and not in today's
    (the start of its backward, all six masks still saved).  Measured on an MI355X with the
    gradients kept instead: 24902656 bytes today, 14654976 with add_hidden, 2.90 masks apart."""
    from eraft_amd import SequenceLoss
    N, h, w, H, W = M.PEAK_GEO
    iters, one_mask = 6, N * 576 * h * w * 4
    hiddens, flows, weight, bias = M.inputs(M.PEAK_GEO, 950)
    hiddens, flows = (hiddens * 2)[:iters], (flows * 2)[:iters]
    gt = torch.from_numpy(R.prng.gauss(990, (N, 2, H, W), 2.0)).to(DEV)
    valid = torch.ones((N, H, W), device=DEV)
    conv = torch.nn.Conv2d(256, 576, 1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(weight)
        conv.bias.copy_(bias)

    def step(fused):
        xs = [x.to(DEV).requires_grad_(True) for x in hiddens]
        fs = [f.to(DEV).requires_grad_(True) for f in flows]
        arrived = []

        def consume(leaf):
            arrived.append(leaf.grad.shape)
            leaf.grad = None

        for leaf in (*xs, *fs):
            leaf.register_post_accumulate_grad_hook(consume)
        conv.zero_grad(set_to_none=True)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        crit = SequenceLoss(gt, valid)
        for i in range(iters):
            if fused:
                crit.add_hidden(conv, xs[i], fs[i], i, iters)
            else:
                crit.add_upsampled(fs[i], M.SCALE * conv(xs[i]), i, iters)
        loss, _ = crit.result()
        loss.backward()
        torch.cuda.synchronize()
        assert sorted(arrived) == sorted(t.shape for t in (*xs, *fs))
        assert conv.weight.grad is not None and conv.bias.grad is not None
        return torch.cuda.max_memory_allocated() - base, float(loss.detach())

    step(True), step(False)  # the pack, MIOpen's choices and workspaces: made before the measurement
    (peak_a, loss_a), (peak_b, loss_b) = step(False), step(True)
    print(f"tail peak above the inputs: {peak_a} bytes today, {peak_b} with add_hidden: {(peak_a - peak_b) / one_mask:.2f} "
          f"masks of {one_mask} bytes fewer (bar 4)")
    assert abs(loss_a - loss_b) <= 1e-5 * abs(loss_a)
    assert peak_a - peak_b >= 4 * one_mask


# ---- the whole model ----
@pytest.mark.gpu
def test_whole_model_step_with_the_switch(gpu_lib, monkeypatch):
    """TRAIN of test_train_parity with fuse_mask_loss set on the instance: the step calls no
    576-output convolution, every parameter receives a finite gradient, and the loss and metrics are
    the unswitched step's at the bars test_sequence_loss.py applies to two separate steps.  With
    the attribute unset the step calls neither new entry point.  (Gradients are not compared across
    two forwards, DESIGN §29: the tail-level tests above share their inputs and carry that.)"""
    from eraft_amd import SequenceLoss, _lib
    from _train_ref import inputs, make_model
    from test_train_parity import TRAIN as cfg
    model = make_model(cfg).to(DEV)
    im1, im2, gt, finit, _ = (None if a is None else torch.from_numpy(a).to(DEV) if isinstance(a, np.ndarray) else a
                              for a in inputs(cfg))
    valid = torch.from_numpy(np.asarray(R.VALID_VALUES, np.float32)[
        (R.prng.uniform(5, (cfg.B, cfg.H, cfg.W)) * 4).astype(np.int64).clip(0, 3)]).to(DEV)
    kw = {"iters": cfg.iters, "flow_init": finit}
    calls = []
    for name in ("mask_upsample_loss", "mask_upsample_loss_bwd"):
        monkeypatch.setattr(_lib, name, lambda *a, _f=getattr(_lib, name), _n=name, **k: (calls.append(_n), _f(*a, **k))[1])
    conv2d = F.conv2d

    def no_mask_head(x, weight, *a, **k):
        assert tuple(weight.shape) != (576, 256, 1, 1), "the step ran the mask head's convolution"
        return conv2d(x, weight, *a, **k)

    def step():
        model.zero_grad(set_to_none=True)
        crit = SequenceLoss(gt, valid)
        _, preds = model(im1, im2, sequence_loss=crit, **kw)
        assert preds == []
        loss, metrics = crit.result()
        loss.backward()
        return float(loss.detach()), {k: float(v) for k, v in metrics.items()}

    assert model.fuse_mask_loss is False
    l_ref, m_ref = step()
    assert calls == []
    with torch.no_grad():
        _, preds = model(im1, im2, **kw)
        P = max(float(p.abs().max()) for p in preds)
        epe = torch.sum((preds[-1] - gt) ** 2, dim=1).sqrt()[R.valid_mask(gt, valid, 400.0)].double().cpu()
    model.fuse_mask_loss = True
    monkeypatch.setattr(F, "conv2d", no_mask_head)
    l_fus, m_fus = step()
    monkeypatch.setattr(F, "conv2d", conv2d)
    assert calls == ["mask_upsample_loss"] * cfg.iters + ["mask_upsample_loss_bwd"] * cfg.iters
    for n, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), n
    bar, ebar = 1e-5 * P * sum(R.GAMMA ** k for k in range(cfg.iters)), math.sqrt(2) * 1e-5 * P
    print(f"loss {l_fus:.9g} with the switch, {l_ref:.9g} without: {abs(l_fus - l_ref):.2e} (bar {bar:.2e}); epe "
          f"{abs(m_fus['epe'] - m_ref['epe']):.2e} (bar {ebar:.2e})")
    assert abs(l_fus - l_ref) <= bar and abs(m_fus["epe"] - m_ref["epe"]) <= ebar
    for k, th in (("1px", 1.0), ("3px", 3.0), ("5px", 5.0)):
        near = int(((epe - th).abs() <= ebar).sum())
        assert abs(round(m_fus[k] * epe.numel()) - round(m_ref[k] * epe.numel())) <= 2 * near, k
    with torch.no_grad():  # validation
        calls.clear()
        crit = SequenceLoss(gt, valid)
        model(im1, im2, sequence_loss=crit, **kw)
        loss, m = crit.result()
    assert calls == ["mask_upsample_loss"] * cfg.iters and not loss.requires_grad
    assert abs(float(loss) - l_ref) <= bar and abs(float(m["epe"]) - m_ref["epe"]) <= ebar
