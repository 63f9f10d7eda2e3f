"""Harness of tests/test_sequence_loss.py: the cases and their fp64 truth (plain torch on the CPU).

A case is n = 3 iterations' (flow_i, mask_i) at the coarse size, one ground truth and one validity
map on the unpadded frame.  The truth is written out here: the torch upsampling composition
(_train_ref.torch_upsample_flow) in fp64, cropped by the pad at the top and left, then
    v      = (valid >= 0.5) & (sqrt(gx^2 + gy^2) < max_flow)
    loss   = sum_i gamma^(n-1-i) mean(v * |pred_i - gt|)
    epe    = sqrt(dx^2 + dy^2) of the last prediction over the valid pixels; its mean and the
             fractions below 1, 3 and 5
and the gradients are fp64 autograd of that.

Input conditions (asserted in build(), on the CPU): gt = pred64_last + d with a random sign and
|d| in [1e-2, 4]; no |pred64_i - gt| of any iteration lies within MARGIN = 1e-3 * max|pred64| of the
L1 kink; no fp64 EPE within 1e-3 of 1, 3 or 5; no |gt| within 1e-3 of max_flow.  Elements that
miss a condition get a new d until none does.  The flows are drawn at sigma 0.2 so that max|pred64|
<= 8 * 0.2 * 2 sqrt(3) = 5.6 and MARGIN stays below the smallest |d|.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

import prng
from _train_ref import torch_upsample_flow

GAMMA = 0.8
ITERS = 3
FLOW_SIGMA = 0.2
# (N, h, w, H, W): no pad; pads 22 and 15 (cut through coarse pixels, two 64-lane x-blocks, ragged
# second block); pads 24 and 24 (whole coarse rows and columns removed); pad 0, one lane in the
# second block
SHAPES = {"nopad": (1, 4, 8, 32, 64), "cut": (2, 9, 70, 50, 545), "rows": (1, 8, 12, 40, 72),
          "lane": (2, 3, 65, 24, 520)}
VALID_VALUES = (0.0, 0.49, 0.5, 1.0)


class Case(NamedTuple):
    name: str
    geo: tuple            # (N, h, w, H, W)
    flows: tuple          # fp32 torch [N, 2, h, w] per iteration
    masks: tuple          # fp32 torch [N, 576, h, w] per iteration
    gt: torch.Tensor      # fp32 [N, 2, H, W]
    valid: torch.Tensor   # fp32 [N, H, W]
    max_flow: float
    scale: float          # max |pred64| over the iterations


class Truth(NamedTuple):
    loss: float
    terms: tuple          # per iteration, unweighted: mean(v |pred_i - gt|)
    n_valid: int
    epe: float            # NaN with no valid pixel
    counts: tuple         # (#epe<1, #epe<3, #epe<5)
    preds: tuple          # fp64 numpy per iteration
    dflows: tuple         # d loss / d flow_i, fp64 numpy
    dmasks: tuple
    dpreds: tuple         # d loss / d pred_i


def weights(n=ITERS, gamma=GAMMA):
    return [gamma ** (n - 1 - i) for i in range(n)]


def pads(geo):
    N, h, w, H, W = geo
    return 8 * h - H, 8 * w - W


def upsample64(flow, mask, geo):
    ph, pw = pads(geo)
    return torch_upsample_flow(flow.double(), mask.double())[..., ph:, pw:]


def valid_mask(gt, valid, max_flow):
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    return (valid >= 0.5) & (mag < max_flow)


@functools.lru_cache(maxsize=None)
def build(shape, sigma=2.0, max_flow=400.0, no_valid=False, seed=700):
    geo = SHAPES[shape]
    N, h, w, H, W = geo
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    flows = tuple(t(prng.gauss(seed + i, (N, 2, h, w), FLOW_SIGMA)) for i in range(ITERS))
    masks = tuple(t(prng.gauss(seed + 10 + i, (N, 576, h, w), float(sigma))) for i in range(ITERS))
    preds = [upsample64(f, m, geo) for f, m in zip(flows, masks)]
    scale = max(float(p.abs().max()) for p in preds)
    margin = 1e-3 * scale
    assert 0 < margin < 1e-2, margin

    def draw(k):
        mag = 1e-2 + (4.0 - 1e-2) * t(prng.uniform(seed + 100 + k, (N, 2, H, W)).astype(np.float64))
        sign = torch.where(t(prng.uniform(seed + 200 + k, (N, 2, H, W)).astype(np.float64)) < 0.5, -1.0, 1.0)
        return mag * sign

    def misses(gt):
        """[N, H, W]: pixels that miss a condition."""
        g = gt.double()
        near_kink = torch.stack([(p - g).abs() < margin for p in preds]).any(0).any(1)
        epe = torch.sum((preds[-1] - g) ** 2, dim=1).sqrt()
        near_px = torch.stack([(epe - th).abs() < 1e-3 for th in (1.0, 3.0, 5.0)]).any(0)
        near_cut = (torch.sum(g ** 2, dim=1).sqrt() - max_flow).abs() < 1e-3
        return near_kink | near_px | near_cut

    d = draw(0)
    for k in range(1, 40):
        gt = (preds[-1] + d).float()
        bad = misses(gt)
        if not bad.any():
            break
        d = torch.where(bad[:, None], draw(k), d)
    gt = (preds[-1] + d).float()
    assert not misses(gt).any()
    dmin = float((gt.double() - preds[-1]).abs().min())
    assert dmin >= 1e-3 * scale and 1e-2 - 1e-5 <= dmin and float(d.abs().max()) <= 4.0, (dmin, scale)
    if no_valid:
        valid = t(np.where(prng.uniform(seed + 300, (N, H, W)) < 0.5, 0.0, 0.49).astype(np.float32))
    else:
        pick = (prng.uniform(seed + 300, (N, H, W)) * 4).astype(np.int64).clip(0, 3)
        valid = t(np.asarray(VALID_VALUES, np.float32)[pick])
        assert set(np.unique(valid.numpy()).tolist()) == set(np.float32(VALID_VALUES).tolist())
    v = valid_mask(gt, valid, max_flow)
    assert bool(v.any()) != no_valid
    if max_flow < 100 and not no_valid:
        cut = (valid >= 0.5) & ~v
        assert int(cut.sum()) > 0.05 * v.numel(), "max_flow cuts no real pixels"
    name = f"{shape}-s{sigma:g}-mf{max_flow:g}" + ("-novalid" if no_valid else "")
    return Case(name, geo, flows, masks, gt, valid, float(max_flow), scale)


@functools.lru_cache(maxsize=None)
def truth(case):
    gt, valid = case.gt.double(), case.valid.double()
    v = valid_mask(gt, valid, case.max_flow)
    flows = [f.double().requires_grad_(True) for f in case.flows]
    masks = [m.double().requires_grad_(True) for m in case.masks]
    preds = [upsample64(f, m, case.geo) for f, m in zip(flows, masks)]
    for p in preds:
        p.retain_grad()
    terms = [(v[:, None] * (p - gt).abs()).mean() for p in preds]
    loss = sum(wt * term for wt, term in zip(weights(), terms))
    loss.backward()
    epe = torch.sum((preds[-1].detach() - gt) ** 2, dim=1).sqrt().reshape(-1)[v.reshape(-1)]
    np64 = lambda ts: tuple(x.detach().numpy().copy() for x in ts)  # noqa: E731
    return Truth(float(loss.detach()), tuple(float(x.detach()) for x in terms), int(v.sum()),
                 float(epe.mean()) if epe.numel() else float("nan"),
                 tuple(int((epe < th).sum()) for th in (1.0, 3.0, 5.0)), np64(preds),
                 np64([f.grad for f in flows]), np64([m.grad for m in masks]), np64([p.grad for p in preds]))


def torch_loss(preds, gt, valid, gamma=GAMMA, max_flow=400.0):
    """The loss as the reference's trainers compose it in torch, in the tensors' own precision."""
    v = valid_mask(gt, valid, max_flow)
    n = len(preds)
    return sum(gamma ** (n - 1 - i) * (v[:, None] * (p - gt).abs()).mean() for i, p in enumerate(preds))
