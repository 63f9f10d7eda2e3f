"""The sequence loss in HIP (csrc/corr_loss.hip, include/corr_mi355x_train.h, eraft_amd/loss.py):
alone over stored predictions and fused with the convex upsampling, against the fp64 truth of
tests/_loss_ref.py (which also states the cases' input conditions).

Bars.  P = max|pred64| of the case, G = sum_i gamma^(n-1-i):
  loss          |d| <= 1e-5 P G       the project's bar for corr_convex_upsample, 1e-5 of max|out|,
                                      carried through a mean and the weighted sum
  counts        exact
  epe           |d| <= sqrt(2) 1e-5 P
  dflow, dmask, dpred   within 1e-4 of max|ref| per tensor (test_convex_upsample_backward_vs_autograd)
  dpred         also bit-equal to scale * v * sign(pred - gt) formed in fp32 by torch
  whole model   GPU_TOL = 1e-3 norm_rel per parameter, whole gradient's absolute error <= 1e-3 of
                its largest entry (test_train_parity.py's bars for two paths that differ only in
                this project's kernels)
The tests print their measured errors; DESIGN.md §29 records them.
"""
import ctypes
import gc
import math
import os
import re

import numpy as np
import pytest
import torch

import _loss_ref as R
from _util import DEV, bit_equal, norm_rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "corr_mi355x_train.h")
G = sum(R.weights())

# (shape, sigma, max_flow, no_valid)
CASES = [("nopad", 2.0, 400.0, False), ("cut", 2.0, 400.0, False), ("rows", 2.0, 400.0, False),
         ("lane", 2.0, 400.0, False), ("cut", 30.0, 400.0, False), ("cut", 2.0, 5.0, False),
         ("nopad", 2.0, 400.0, True)]
IDS = [f"{s}-sigma{g:g}-maxflow{m:g}" + ("-novalid" if nv else "") for s, g, m, nv in CASES]


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


def test_train_header_declares_the_train_exports(lib):
    from eraft_amd import _lib
    assert sorted(_lib.TRAIN_EXPORTS) == _declared() and len(_lib.TRAIN_EXPORTS) == 6
    assert not set(_lib.TRAIN_EXPORTS) & set(_lib.EXPORTS)
    for name in _declared():
        assert hasattr(lib, name), name
    for name in _lib.TRAIN_EXPORTS:
        want = ctypes.c_size_t if name.endswith("_workspace") else ctypes.c_int
        assert getattr(lib, name).restype is want, name


def test_abi_version_is_unchanged(lib):
    assert lib.corr_version() == 202


def test_package_exports_the_loss():
    import eraft_amd
    assert "sequence_loss" in eraft_amd.__all__ and "SequenceLoss" in eraft_amd.__all__
    assert callable(eraft_amd.sequence_loss) and callable(eraft_amd.SequenceLoss)


def test_workspace_sizes(lib):
    for bad in ((0, 4, 8), (1, 0, 8), (1, 4, 0), (-1, 4, 8)):
        assert lib.corr_upsample_loss_workspace(*bad) == 0 and lib.corr_sequence_loss_workspace(*bad) == 0, bad
    # the 18 S planes of the backward; the forward's 48-byte partials per 64-lane workgroup fit in them
    assert lib.corr_upsample_loss_workspace(2, 9, 70) == 2 * 18 * 9 * 70 * 4
    assert lib.corr_upsample_loss_workspace(2, 9, 70) >= 2 * 9 * 2 * 48
    assert lib.corr_sequence_loss_workspace(1, 64, 64) == 48
    assert lib.corr_sequence_loss_workspace(1, 64, 65) == 96


_P = 256   # a well-aligned non-null pointer that is never dereferenced
_BIG = 1 << 40


def _refused(lib, rc, msg):
    err = lib.corr_last_error().decode()
    return rc == -1 and msg in err and len(err) > len(msg)


def test_upsample_loss_refusals(lib):
    """One refusal per rule, each CORR_EINVAL with a message: any HIP call would fail differently
    on a machine without a GPU."""
    def fwd(flow=_P, mask=_P, gt=_P, valid=_P, N=2, h=9, w=70, H=50, W=545, mf=400.0, out=_P, ws=_P, wsb=_BIG):
        return lib.corr_upsample_loss(flow, mask, gt, valid, N, h, w, H, W, mf, 1, out, ws, wsb, None)

    def bwd(flow=_P, mask=_P, gt=_P, valid=_P, scale=_P, N=2, h=9, w=70, H=50, W=545, mf=400.0, dflow=_P, dmask=_P,
            ws=_P, wsb=_BIG):
        return lib.corr_upsample_loss_bwd(flow, mask, gt, valid, scale, N, h, w, H, W, mf, dflow, dmask, ws, wsb, None)

    need = lib.corr_upsample_loss_workspace(2, 9, 70)
    for call, ptrs in ((fwd, ("flow", "mask", "gt", "valid")),
                       (bwd, ("flow", "mask", "gt", "valid", "scale", "dflow", "dmask"))):
        for name in ptrs:
            assert _refused(lib, call(**{name: None}), f"{name} is NULL"), name
            assert _refused(lib, call(**{name: _P + 2}), f"{name} is not 4-byte aligned"), name
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
        # 576 * 1821 * 2048 >= 2^31 mask elements; one coarse row fewer passes on to the next check
        assert _refused(lib, call(N=1, h=1821, w=2048, H=8, W=8), "too large")
        assert _refused(lib, call(N=1, h=1820, w=2048, H=8, W=8, wsb=16), "workspace of")
    assert _refused(lib, fwd(out=None), "out is NULL")
    assert _refused(lib, fwd(out=_P + 4), "out is not 8-byte aligned")


def test_sequence_loss_refusals(lib):
    def fwd(pred=_P, gt=_P, valid=_P, N=2, H=50, W=545, mf=400.0, out=_P, ws=_P, wsb=_BIG):
        return lib.corr_sequence_loss(pred, gt, valid, N, H, W, mf, 1, out, ws, wsb, None)

    def bwd(pred=_P, gt=_P, valid=_P, scale=_P, N=2, H=50, W=545, mf=400.0, dpred=_P):
        return lib.corr_sequence_loss_bwd(pred, gt, valid, scale, N, H, W, mf, dpred, None)

    for call, ptrs in ((fwd, ("pred", "gt", "valid")), (bwd, ("pred", "gt", "valid", "scale", "dpred"))):
        for name in ptrs:
            assert _refused(lib, call(**{name: None}), f"{name} is NULL"), name
            assert _refused(lib, call(**{name: _P + 2}), f"{name} is not 4-byte aligned"), name
        assert _refused(lib, call(N=0), "N must be >= 1")
        assert _refused(lib, call(H=0), "H, W must be >= 1")
        assert _refused(lib, call(W=0), "H, W must be >= 1")
        for mf in (0.0, -1.0, float("inf"), float("nan")):
            assert _refused(lib, call(mf=mf), "max_flow must be finite and positive"), mf
        assert _refused(lib, call(N=1, H=1 << 15, W=1 << 15), "too large")      # 2 * 2^30 elements
    need = lib.corr_sequence_loss_workspace(2, 50, 545)
    assert _refused(lib, fwd(wsb=need - 1), "workspace of")
    assert _refused(lib, fwd(ws=None), "workspace is NULL")
    assert _refused(lib, fwd(ws=_P + 4), "workspace is not 8-byte aligned")
    assert _refused(lib, fwd(out=None), "out is NULL")
    assert _refused(lib, fwd(out=_P + 4), "out is not 8-byte aligned")
    assert _refused(lib, fwd(N=1, H=(1 << 15) - 1, W=1 << 15, wsb=16), "workspace of")  # one row fewer: the next check


def _preds_cpu(case, dtype):
    return [R.upsample64(f, m, case.geo).to(dtype) for f, m in zip(case.flows, case.masks)]


def _check_forward(what, case, loss, metrics, t):
    """Every forward bar of the module docstring; prints the figures."""
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


@pytest.mark.parametrize("args", CASES, ids=IDS)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
def test_cpu_fallback_against_fp64(args, dtype):
    """sequence_loss and SequenceLoss on CPU tensors (the torch composition in loss.py)."""
    from eraft_amd import SequenceLoss, sequence_loss
    case = R.build(*args)
    t = R.truth(case)
    gt, valid = case.gt.to(dtype), case.valid.to(dtype)
    loss, m = sequence_loss(_preds_cpu(case, dtype), gt, valid[:, None], R.GAMMA, case.max_flow)
    assert loss.dim() == 0 and all(isinstance(v, torch.Tensor) and v.dim() == 0 for v in m.values())
    _check_forward("cpu sequence_loss", case, loss, m, t)
    crit = SequenceLoss(gt, valid, R.GAMMA, case.max_flow)
    flows = [f.clone().to(dtype).requires_grad_(True) for f in case.flows]
    for i in reversed(range(R.ITERS)):  # any order of arrival: result() sums in iteration order
        crit.add_upsampled(flows[i], case.masks[i].to(dtype), i, R.ITERS, R.pads(case.geo))
    loss, m = crit.result()
    _check_forward("cpu SequenceLoss", case, loss, m, t)
    if dtype == torch.float64 and t.n_valid:
        loss.backward()
        for i in range(R.ITERS):
            assert norm_rel(flows[i].grad.numpy(), t.dflows[i]) < 1e-9


def test_criterion_refuses_bad_geometry():
    from eraft_amd import SequenceLoss
    case = R.build(*CASES[0])
    crit = SequenceLoss(case.gt, case.valid)
    with pytest.raises(ValueError, match="does not upsample"):
        crit.add_upsampled(case.flows[0], case.masks[0], 0, 1, (8, 0))
    with pytest.raises(ValueError, match="index"):
        crit.add_upsampled(case.flows[0], case.masks[0], 1, 1)
    with pytest.raises(ValueError, match="valid"):
        SequenceLoss(case.gt, case.valid[:, :-1])
    with pytest.raises(RuntimeError, match="no prediction"):
        crit.result()


def test_model_forward_with_a_criterion_on_the_cpu():
    """ERAFT.forward(..., sequence_loss=crit) on CPU tensors: the loss of the unfused model's
    predictions put through sequence_loss, an empty prediction list, and the same gradients."""
    from eraft_amd import SequenceLoss, sequence_loss
    from _train_ref import Config, inputs, make_model, substituted
    cfg = Config(H=120, W=150, B=1, iters=2)  # the padder pads to 128x160
    im1, im2, gt, _, _ = (None if a is None else torch.from_numpy(a) if isinstance(a, np.ndarray) else a
                          for a in inputs(cfg))
    valid = torch.from_numpy(np.asarray(R.VALID_VALUES, np.float32)[
        (R.prng.uniform(5, (cfg.B, cfg.H, cfg.W)) * 4).astype(np.int64).clip(0, 3)])
    with substituted(torch.float32, torch_upsample=False):
        model = make_model(cfg)
        low, preds = model(im1, im2, iters=cfg.iters)
        ref, ref_m = sequence_loss(preds, gt, valid)
        ref.backward()
        g_ref = {n: p.grad.clone() for n, p in model.named_parameters() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        crit = SequenceLoss(gt, valid)
        low2, none = model(im1, im2, iters=cfg.iters, sequence_loss=crit)
        loss, m = crit.result()
        loss.backward()
    assert none == [] and len(preds) == cfg.iters and torch.equal(low, low2)
    assert abs(float(loss.detach()) - float(ref.detach())) <= 1e-6 * abs(float(ref.detach()))
    assert all(abs(float(m[k]) - float(ref_m[k])) <= 1e-6 for k in ref_m)
    got = {n: p.grad for n, p in model.named_parameters() if p.grad is not None}
    assert got.keys() == g_ref.keys() and len(got) > 50
    scale = max(float(g.abs().max()) for g in g_ref.values())
    assert max(float((got[n] - g_ref[n]).abs().max()) for n in got) <= 1e-3 * scale


# ----------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------
def _gpu_case(case):
    return ([f.to(DEV) for f in case.flows], [m.to(DEV) for m in case.masks], case.gt.to(DEV), case.valid.to(DEV))


def _fused(case, flows, masks, gt, valid, total=R.ITERS, only=None):
    from eraft_amd import SequenceLoss
    crit = SequenceLoss(gt, valid, R.GAMMA, case.max_flow)
    for i in (range(total) if only is None else [only]):
        crit.add_upsampled(flows[i], masks[i], i, total, R.pads(case.geo))
    return crit.result()


def _upsampled(case, flow, mask):
    """upsample_flow's own output on the GPU, cropped by the pad."""
    from eraft_amd.model import ERAFT
    ph, pw = R.pads(case.geo)
    return ERAFT.upsample_flow(flow, mask)[..., ph:, pw:]


@pytest.fixture(scope="module")
def gpu_lib(lib):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return lib


@pytest.mark.gpu
@pytest.mark.parametrize("args", CASES, ids=IDS)
def test_forward_parity_against_fp64(gpu_lib, args):
    from eraft_amd import _lib, sequence_loss
    case = R.build(*args)
    t = R.truth(case)
    flows, masks, gt, valid = _gpu_case(case)
    with torch.no_grad():
        loss_f, m_f = _fused(case, flows, masks, gt, valid)
        preds = [_upsampled(case, f, m) for f, m in zip(flows, masks)]
        for p, p64 in zip(preds, t.preds):
            assert norm_rel(p.cpu().numpy(), p64) <= 1e-5
        loss_s, m_s = sequence_loss(preds, gt, valid[:, None], R.GAMMA, case.max_flow)
        stats = _lib.upsample_loss(flows[-1], masks[-1], gt, valid, case.max_flow, True).cpu().numpy()
        stats_s = _lib.sequence_loss(preds[-1].contiguous(), gt, valid, case.max_flow, True).cpu().numpy()
    assert loss_f.is_cuda and loss_f.dim() == 0 and all(v.is_cuda and v.dim() == 0 for v in m_f.values())
    _check_forward("fused", case, loss_f, m_f, t)
    _check_forward("stand-alone", case, loss_s, m_s, t)
    d = abs(float(loss_f) - float(loss_s))
    print(f"fused vs stand-alone {case.name}: {d:.2e}")
    assert d <= 1e-5 * case.scale * G
    for s in (stats, stats_s):
        assert (int(s[1]), int(s[3]), int(s[4]), int(s[5])) == (t.n_valid, *t.counts)
        assert all(float(x) == int(x) for x in s[[1, 3, 4, 5]])
    # the fused prediction carries upsample_flow's bits, so the two sums see the same terms; they
    # group them differently into the threads' fp32 sums of 16 terms (16 * 2^-24 each at most)
    assert abs(stats[0] - stats_s[0]) <= 2 * 16 * 2.0 ** -24 * abs(stats_s[0])


def _torch_dpred(pred, gt, valid, max_flow, scale):
    """scale * v * sign(pred - gt), formed in fp32 by torch."""
    v = R.valid_mask(gt, valid, max_flow).float()[:, None]
    return torch.tensor(scale, dtype=torch.float32, device=pred.device) * v * torch.sign(pred - gt)


@pytest.mark.gpu
@pytest.mark.parametrize("args", CASES[:6], ids=IDS[:6])
def test_backward_parity_against_fp64_autograd(gpu_lib, args):
    from eraft_amd import sequence_loss
    case = R.build(*args)
    t = R.truth(case)
    flows, masks, gt, valid = _gpu_case(case)
    flows = [f.requires_grad_(True) for f in flows]
    masks = [m.requires_grad_(True) for m in masks]
    loss, _ = _fused(case, flows, masks, gt, valid)
    loss.backward()
    with torch.no_grad():
        preds = [_upsampled(case, f, m).contiguous() for f, m in zip(flows, masks)]
    preds = [p.requires_grad_(True) for p in preds]
    loss_s, _ = sequence_loss(preds, gt, valid, R.GAMMA, case.max_flow)
    loss_s.backward()
    for i, wt in enumerate(R.weights()):
        for what, got, ref in (("dflow", flows[i].grad, t.dflows[i]), ("dmask", masks[i].grad, t.dmasks[i]),
                               ("dpred", preds[i].grad, t.dpreds[i])):
            e = norm_rel(got.cpu().numpy(), ref)
            print(f"{case.name} iteration {i}: {what} {e:.2e} of max|ref|")
            assert e <= 1e-4, (what, i)
        want = _torch_dpred(preds[i].detach(), gt, valid, case.max_flow, np.float32(wt / preds[i].numel()))
        assert torch.equal(preds[i].grad.view(torch.int32), want.view(torch.int32)), i


@pytest.mark.gpu
def test_upstream_scalar_and_iteration_weights(gpu_lib):
    """(3 loss).backward() over n = 3 terms = 3 x the weighted sum of the single terms' gradients."""
    case = R.build(*CASES[1])
    flows, masks, gt, valid = _gpu_case(case)
    single = []
    for i in range(R.ITERS):
        f, m = flows[i].clone().requires_grad_(True), masks[i].clone().requires_grad_(True)
        loss, _ = _fused(case, {i: f}, {i: m}, gt, valid, total=R.ITERS, only=i)  # weight gamma^(n-1-i)
        one, _ = _fused(case, [f], [m], gt, valid, total=1)                        # weight 1
        assert abs(float(loss.detach()) - R.weights()[i] * float(one.detach())) <= 1e-6 * abs(float(one.detach()))
        one.backward()
        single.append((f.grad.double(), m.grad.double()))
    fs = [f.clone().requires_grad_(True) for f in flows]
    ms = [m.clone().requires_grad_(True) for m in masks]
    loss, _ = _fused(case, fs, ms, gt, valid)
    (3 * loss).backward()
    for i, wt in enumerate(R.weights()):
        for what, got, ref in (("dflow", fs[i].grad, single[i][0]), ("dmask", ms[i].grad, single[i][1])):
            e = norm_rel(got.cpu().numpy(), (3 * wt * ref).cpu().numpy())
            print(f"term {i}: {what} {e:.2e}")
            assert e <= 1e-4


@pytest.mark.gpu
def test_second_order_is_refused(gpu_lib):
    case = R.build(*CASES[0])
    flows, masks, gt, valid = _gpu_case(case)
    f = flows[0].requires_grad_(True)
    loss, _ = _fused(case, [f], masks[:1], gt, valid, total=1)
    (g,) = torch.autograd.grad(loss, f, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


@pytest.mark.gpu
def test_two_runs_are_bit_identical(gpu_lib):
    case = R.build(*CASES[1])
    runs = []
    for _ in range(2):
        flows, masks, gt, valid = _gpu_case(case)
        flows = [f.requires_grad_(True) for f in flows]
        masks = [m.requires_grad_(True) for m in masks]
        loss, m = _fused(case, flows, masks, gt, valid)
        loss.backward()
        runs.append([loss.detach().double(), *(m[k] for k in sorted(m)), *(f.grad for f in flows), *(x.grad for x in masks)])
    for a, b in zip(*runs):
        a, b = a.contiguous().view(torch.int32 if a.element_size() == 4 else torch.int64), b.contiguous().view(
            torch.int32 if b.element_size() == 4 else torch.int64)
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("where", ["gt-under-valid-0", "mask-kept", "mask-cropped"])
def test_non_finite_inputs_poison_as_the_torch_chain(gpu_lib, where):
    """A NaN in gt under valid = 0 poisons the sum (v is multiplied in); one in the mask poisons it
    where the crop keeps the coarse pixel and not where it removes it: NaN-ness equals the fp32
    torch chain's."""
    from eraft_amd import sequence_loss
    case = R.build("rows")  # pads 24 and 24: coarse rows and columns 0..2 are removed
    flows, masks, gt, valid = (list(case.flows), [m.clone() for m in case.masks], case.gt.clone(), case.valid.clone())
    if where == "gt-under-valid-0":
        valid[0, 5, 7] = 0.0
        gt[0, 1, 5, 7] = float("nan")
    elif where == "mask-kept":
        masks[1][0, 100, 4, 5] = float("nan")
    else:
        masks[1][0, 100, 1, 5] = float("nan")
        masks[2][0, 7, 5, 2] = float("nan")
    chain = R.torch_loss([R.torch_upsample_flow(f, m)[..., 24:, 24:] for f, m in zip(flows, masks)], gt, valid)
    assert bool(torch.isnan(chain)) == (where != "mask-cropped")
    d = lambda ts: [x.to(DEV) for x in ts]  # noqa: E731
    flows, masks, gt, valid = d(flows), d(masks), gt.to(DEV), valid.to(DEV)
    with torch.no_grad():
        fused, _ = _fused(case, flows, masks, gt, valid)
        alone, _ = sequence_loss([_upsampled(case, f, m) for f, m in zip(flows, masks)], gt, valid)
    assert bool(torch.isnan(fused)) == bool(torch.isnan(chain)) == bool(torch.isnan(alone))
    if where == "mask-cropped":
        assert abs(float(fused) - float(chain)) <= 1e-5 * case.scale * G


# ---- buffer and stream discipline of the four launching entry points (test_core_discipline.py) ----
from test_core_discipline import Arena, _clones, _ordered_on_the_callers_stream, _run_case, _same, gpu, side  # noqa: E402,F401

DISCIPLINE_SHAPES = ("cut", "rows")


def _data(shape):
    case = R.build(shape)
    flows, masks, gt, valid = _gpu_case(case)
    with torch.no_grad():
        pred = _upsampled(case, flows[0], masks[0]).contiguous()
    return case.geo, flows[0], masks[0], gt, valid, pred, torch.full((1,), 0.37, device=DEV)


_DATA = {}


def _shared(shape):
    if shape not in _DATA:
        _DATA[shape] = _data(shape)
    return _DATA[shape]


def _ok(lib, rc):
    assert rc == 0, f"rc {rc}: {lib.corr_last_error().decode(errors='replace')}"


def _s():
    return torch.cuda.current_stream().cuda_stream


def case_upsample_loss(A, shape):
    from eraft_amd import _lib
    lib = _lib.load()
    (N, h, w, H, W), flow, mask, gt, valid, _, _ = _shared(shape)
    flow, mask, gt, valid = (A.inp(n, v) for n, v in zip(("flow", "mask", "gt", "valid"), (flow, mask, gt, valid)))
    out = A.out("out", (12,))  # six fp64 words
    wp, wn = A.ws("workspace", lib.corr_upsample_loss_workspace(N, h, w))

    def call():
        _ok(lib, lib.corr_upsample_loss(flow.data_ptr(), mask.data_ptr(), gt.data_ptr(), valid.data_ptr(), N, h, w, H,
                                        W, 400.0, 1, out.data_ptr(), wp, wn, _s()))
    return call, _clones(out=out)


def case_upsample_loss_bwd(A, shape):
    from eraft_amd import _lib
    lib = _lib.load()
    (N, h, w, H, W), flow, mask, gt, valid, _, scale = _shared(shape)
    flow, mask, gt, valid, scale = (A.inp(n, v) for n, v in zip(("flow", "mask", "gt", "valid", "scale"),
                                                                (flow, mask, gt, valid, scale)))
    dflow, dmask = A.out("dflow", (N, 2, h, w)), A.out("dmask", (N, 576, h, w))
    wp, wn = A.ws("workspace", lib.corr_upsample_loss_workspace(N, h, w))

    def call():
        _ok(lib, lib.corr_upsample_loss_bwd(flow.data_ptr(), mask.data_ptr(), gt.data_ptr(), valid.data_ptr(),
                                            scale.data_ptr(), N, h, w, H, W, 400.0, dflow.data_ptr(), dmask.data_ptr(),
                                            wp, wn, _s()))
    return call, _clones(dflow=dflow, dmask=dmask)


def case_sequence_loss(A, shape):
    from eraft_amd import _lib
    lib = _lib.load()
    (N, h, w, H, W), _, _, gt, valid, pred, _ = _shared(shape)
    pred, gt, valid = (A.inp(n, v) for n, v in zip(("pred", "gt", "valid"), (pred, gt, valid)))
    out = A.out("out", (12,))
    wp, wn = A.ws("workspace", lib.corr_sequence_loss_workspace(N, H, W))

    def call():
        _ok(lib, lib.corr_sequence_loss(pred.data_ptr(), gt.data_ptr(), valid.data_ptr(), N, H, W, 400.0, 1,
                                        out.data_ptr(), wp, wn, _s()))
    return call, _clones(out=out)


def case_sequence_loss_bwd(A, shape):
    from eraft_amd import _lib
    lib = _lib.load()
    (N, h, w, H, W), _, _, gt, valid, pred, scale = _shared(shape)
    pred, gt, valid, scale = (A.inp(n, v) for n, v in zip(("pred", "gt", "valid", "scale"), (pred, gt, valid, scale)))
    dpred = A.out("dpred", (N, 2, H, W))

    def call():
        _ok(lib, lib.corr_sequence_loss_bwd(pred.data_ptr(), gt.data_ptr(), valid.data_ptr(), scale.data_ptr(), N, H, W,
                                            400.0, dpred.data_ptr(), _s()))
    return call, _clones(dpred=dpred)


ENTRIES = {"corr_upsample_loss": case_upsample_loss, "corr_upsample_loss_bwd": case_upsample_loss_bwd,
           "corr_sequence_loss": case_sequence_loss, "corr_sequence_loss_bwd": case_sequence_loss_bwd}
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
    assert with_stream == set(ENTRIES) == {n for n in _lib.TRAIN_EXPORTS if not n.endswith("_workspace")}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(DISCIPLINE))
def test_writes_stay_inside(gpu, name):
    """Outputs and workspace in guarded windows over a NaN prefill: guards intact, every output
    (all of dmask, the cropped coarse pixels included) written, results those of the plain call."""
    arena = Arena(guard_out=True, guard_ws=True)
    got = _run_case(DISCIPLINE[name], arena)
    arena.check()
    _same(_plain(name), got, name)
    if "dmask" in got:
        geo = R.SHAPES[name[name.index("[") + 1:-1]]
        ph, pw = R.pads(geo)
        gone = got["dmask"][:, :, :ph // 8, :]
        assert torch.equal(gone, torch.zeros_like(gone)) and torch.equal(got["dmask"][..., :pw // 8], torch.zeros_like(got["dmask"][..., :pw // 8]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in DISCIPLINE if not n.startswith("corr_sequence_loss_bwd")])
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


# ---- the whole model ----
@pytest.mark.gpu
def test_whole_model_step_matches_the_unfused_step(gpu_lib):
    """TRAIN of test_train_parity (120x150 padded to 128x160, B = 2, 4 iterations, train mode, warm
    start): a step with sequence_loss=crit against a step of the same model with the predictions
    put through the torch loss.

    The network's forward is not bit-reproducible from call to call on the GPU (the low-resolution
    flow of two identical calls differs by 4e-5 on an MI355X), and one ReLU unit of the update block
    that lands on the other side of its kink moves parameters' gradients by 2e-3 .. 6e-3
    (test_train_parity.py); two separate steps missed the 1e-3 bar in one run of two for that
    reason alone (worst parameter 1.7e-5 in one run, 2.3e-3 in the next).  So the gradients are compared over ONE
    forward: a criterion that hands each iteration's (flow, mask) to the fused term and, the same
    tensors, to upsample_flow and the torch loss, and one backward for each loss over the shared
    graph: no ReLU side can differ.  Two separate steps give the losses and the peak memory."""
    from eraft_amd import SequenceLoss
    from eraft_amd.model import ERAFT
    from _train_ref import inputs, make_model, zero_set
    from test_train_parity import GPU_TOL, TRAIN as cfg
    model = make_model(cfg).to(DEV)
    im1, im2, gt, finit, _ = (None if a is None else torch.from_numpy(a).to(DEV) if isinstance(a, np.ndarray) else a
                              for a in inputs(cfg))
    valid = torch.from_numpy(np.asarray(R.VALID_VALUES, np.float32)[
        (R.prng.uniform(5, (cfg.B, cfg.H, cfg.W)) * 4).astype(np.int64).clip(0, 3)]).to(DEV)
    kw = {"iters": cfg.iters, "flow_init": finit}

    def grads():
        return {n: None if p.grad is None else p.grad.double().cpu().numpy() for n, p in model.named_parameters()}

    def step(fused):
        """(loss, metrics, what the unfused step saw, peak memory) of one whole step."""
        model.zero_grad(set_to_none=True)
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        if fused:
            crit = SequenceLoss(gt, valid)
            _, preds = model(im1, im2, sequence_loss=crit, **kw)
            assert preds == []
            loss, metrics = crit.result()
        else:
            _, preds = model(im1, im2, **kw)
            loss, metrics = R.torch_loss(preds, gt, valid), None
        loss.backward()
        torch.cuda.synchronize()
        peak, seen = torch.cuda.max_memory_allocated(), None
        if not fused:  # max|pred| and the valid pixels' EPE, on the CPU: nothing of this step stays on the GPU
            epe = torch.sum((preds[-1].detach() - gt) ** 2, dim=1).sqrt()[R.valid_mask(gt, valid, 400.0)]
            seen = (max(float(p.detach().abs().max()) for p in preds), epe.double().cpu())
        return float(loss.detach()), metrics, seen, peak

    l_ref, _, (P, epe), peak_ref = step(False)
    l_fus, metrics, _, peak_fus = step(True)
    bar, ebar = 1e-5 * P * sum(R.GAMMA ** k for k in range(cfg.iters)), math.sqrt(2) * 1e-5 * P
    print(f"loss {l_fus:.9g} fused, {l_ref:.9g} unfused (bar {bar:.2e}); peak memory {peak_fus} fused, {peak_ref} unfused")
    assert abs(l_fus - l_ref) <= bar
    assert peak_fus < peak_ref

    class Both(SequenceLoss):
        """The fused term and, from the same tensors, the chain it replaces."""
        chain = []

        def add_upsampled(self, flow, mask, index, total, pad=(0, 0)):
            super().add_upsampled(flow, mask, index, total, pad)
            self.chain.append(ERAFT.upsample_flow(flow, mask)[..., pad[0]:, pad[1]:])

    model.zero_grad(set_to_none=True)
    crit = Both(gt, valid)
    model(im1, im2, sequence_loss=crit, **kw)
    loss, _ = crit.result()
    loss.backward(retain_graph=True)
    g_fus = grads()
    model.zero_grad(set_to_none=True)
    R.torch_loss(crit.chain, gt, valid).backward()
    g_ref = grads()
    assert {n for n, g in g_ref.items() if g is None} == {n for n, g in g_fus.items() if g is None}
    have = [n for n, g in g_ref.items() if g is not None]
    assert len(have) > 50
    zeros = zero_set(cfg)
    scale = max(np.abs(g_ref[n]).max() for n in have)
    whole = max(np.abs(g_fus[n] - g_ref[n]).max() for n in have) / scale
    worst = max((norm_rel(g_fus[n], g_ref[n]), n) for n in have if n not in zeros)
    print(f"worst parameter {worst[1]}: {worst[0]:.2e} norm_rel; whole gradient {whole:.2e} of its largest entry")
    assert worst[0] <= GPU_TOL and whole <= GPU_TOL

    # Validation under no_grad: the same loss and metrics as the training step's and as the torch
    # chain over the unfused step's predictions, "the same" being the forward bars of this file
    # since the network's forward is not reproducible; a count may differ by the number of valid
    # pixels whose EPE lies within the EPE bar of its threshold.
    with torch.no_grad():
        crit = SequenceLoss(gt, valid)
        model(im1, im2, sequence_loss=crit, **kw)
        loss, m = crit.result()
    assert not loss.requires_grad and set(m) == {"epe", "1px", "3px", "5px"} and epe.numel() > 1000
    print(f"no_grad: loss {float(loss):.9g} vs training step {abs(float(loss) - l_fus):.2e}, vs torch chain "
          f"{abs(float(loss) - l_ref):.2e} (bar {bar:.2e}); epe {float(m['epe']):.9g} vs training step "
          f"{abs(float(m['epe']) - float(metrics['epe'])):.2e}, vs torch chain {abs(float(m['epe']) - float(epe.mean())):.2e} "
          f"(bar {ebar:.2e})")
    assert abs(float(loss) - l_fus) <= bar and abs(float(loss) - l_ref) <= bar
    assert abs(float(m["epe"]) - float(metrics["epe"])) <= ebar and abs(float(m["epe"]) - float(epe.mean())) <= ebar
    for k, th in (("1px", 1.0), ("3px", 3.0), ("5px", 5.0)):
        near, want = int(((epe - th).abs() <= ebar).sum()), int((epe < th).sum())
        for what, got in (("no_grad", m[k]), ("training step", metrics[k])):
            assert abs(round(float(got) * epe.numel()) - want) <= near, (k, what)
