"""Harness of tests/test_mask_head_loss.py: the cases and their fp64 truth (plain torch on the CPU).

A case is n = 3 iterations' (hidden_i, flow_i) at the coarse size, one mask head (weight [576, 256],
bias [576]) shared by the iterations, one ground truth and one validity map on the unpadded frame.
The truth is written out here as the reference composes it:
    mask_i = 0.25 * conv2d(hidden_i, weight, bias)
    pred_i = the torch upsampling composition (_train_ref.torch_upsample_flow), cropped by the pad
    v      = (valid >= 0.5) & (sqrt(gx^2 + gy^2) < max_flow)
    loss   = sum_i gamma^(n-1-i) mean(v * |pred_i - gt|); epe and its counts over the last prediction
all in fp64, and the gradients are fp64 autograd of that (dz is the gradient that arrives at the
convolution's output).

Inputs.  hidden = relu(gauss) as the head sees it; the weights are drawn so that the mask's sigma is
2 (the logits' 8); the flows at sigma 0.2 as _loss_ref's; the ground truth is gauss of the case's
sigma (2 or 30), independent of the predictions.  A sub-pixel with pred ~ gt has no comparable
gradient (the L1 kink), so valid is set to 0 wherever the fp64 truth has |pred64_i - gt| < 1e-3 in
any iteration and channel, and likewise where an fp32 implementation could not settle a count: the
fp64 EPE within 1e-3 of 1, 3 or 5, or |gt| within 1e-3 of max_flow.  build() asserts, on the CPU,
that this removes at most 1 % of the sub-pixels.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch
import torch.nn.functional as F

import _loss_ref as R
import prng
from _train_ref import torch_upsample_flow

GAMMA, ITERS, SCALE = R.GAMMA, R.ITERS, 0.25
KINK = 1e-3
# _loss_ref's four and (N, h, w, H, W) = (1, 5, 40, 36, 315): 15 tiles of 16 pixels, an odd count (the
# last workgroup's second block is dead), pads 4 and 5: neither a multiple of 4
SHAPES = {**R.SHAPES, "odd": (1, 5, 40, 36, 315)}
PEAK_GEO = (2, 24, 32, 192, 256)


class Case(NamedTuple):
    name: str
    geo: tuple            # (N, h, w, H, W)
    hiddens: tuple        # fp32 torch [N, 256, h, w] per iteration
    flows: tuple          # fp32 torch [N, 2, h, w] per iteration
    weight: torch.Tensor  # fp32 [576, 256, 1, 1]
    bias: torch.Tensor    # fp32 [576]
    gt: torch.Tensor      # fp32 [N, 2, H, W]
    valid: torch.Tensor   # fp32 [N, H, W]
    max_flow: float
    scale: float          # max |pred64| over the iterations
    removed: float        # fraction of the sub-pixels whose valid was set to 0


class Truth(NamedTuple):
    loss: float
    terms: tuple
    n_valid: int
    epe: float
    counts: tuple
    preds: tuple          # fp64 numpy per iteration
    dflows: tuple
    dhiddens: tuple
    dzs: tuple            # d loss / d conv2d's output, per iteration
    dweight: np.ndarray
    dbias: np.ndarray


def weights():
    return R.weights(ITERS, GAMMA)


def pads(geo):
    return R.pads(geo)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def pred64(hidden, flow, weight, bias, geo):
    ph, pw = pads(geo)
    mask = SCALE * F.conv2d(hidden, weight, bias)
    return torch_upsample_flow(flow, mask)[..., ph:, pw:]


def inputs(geo, seed):
    """(hiddens, flows, weight, bias) of a geometry."""
    N, h, w, _, _ = geo
    hiddens = tuple(torch.relu(_t(prng.gauss(seed + i, (N, 256, h, w), 1.0))) for i in range(ITERS))
    flows = tuple(_t(prng.gauss(seed + 10 + i, (N, 2, h, w), R.FLOW_SIGMA)) for i in range(ITERS))
    # E[hidden^2] = 1/2, so the logits' sigma is sqrt(128) sigma_w = 8 and the mask's is 2
    weight = _t(prng.gauss(seed + 20, (576, 256, 1, 1), 8.0 / np.sqrt(128.0)))
    bias = _t(prng.gauss(seed + 21, (576,), 1.0))
    return hiddens, flows, weight, bias


@functools.lru_cache(maxsize=None)
def build(shape, sigma=2.0, max_flow=400.0, no_valid=False, seed=900):
    geo = SHAPES[shape]
    N, h, w, H, W = geo
    hiddens, flows, weight, bias = inputs(geo, seed)
    preds = [pred64(x.double(), f.double(), weight.double(), bias.double(), geo) for x, f in zip(hiddens, flows)]
    scale = max(float(p.abs().max()) for p in preds)
    gt = _t(prng.gauss(seed + 30, (N, 2, H, W), float(sigma)))
    g = gt.double()
    kink = torch.stack([(p - g).abs() < KINK for p in preds]).any(0).any(1)
    epe = torch.sum((preds[-1] - g) ** 2, dim=1).sqrt()
    near_px = torch.stack([(epe - th).abs() < 1e-3 for th in (1.0, 3.0, 5.0)]).any(0)
    near_cut = (torch.sum(g ** 2, dim=1).sqrt() - max_flow).abs() < 1e-3
    gone = kink | near_px | near_cut
    removed = float(gone.double().mean())
    assert removed <= 0.01, f"{shape}: the kink and threshold bands remove {removed:.2%} of the sub-pixels"
    if no_valid:
        valid = _t(np.where(prng.uniform(seed + 40, (N, H, W)) < 0.5, 0.0, 0.49).astype(np.float32))
    else:
        pick = (prng.uniform(seed + 40, (N, H, W)) * 4).astype(np.int64).clip(0, 3)
        valid = _t(np.asarray(R.VALID_VALUES, np.float32)[pick])
    valid = torch.where(gone, torch.zeros_like(valid), valid)
    v = R.valid_mask(gt, valid, max_flow)
    assert bool(v.any()) != no_valid
    if max_flow < 100 and not no_valid:
        assert int(((valid >= 0.5) & ~v).sum()) > 0.01 * v.numel(), "max_flow cuts no real pixels"
    name = f"{shape}-s{sigma:g}-mf{max_flow:g}" + ("-novalid" if no_valid else "")
    return Case(name, geo, hiddens, flows, weight, bias, gt, valid, float(max_flow), scale, removed)


@functools.lru_cache(maxsize=None)
def truth(case):
    gt, valid = case.gt.double(), case.valid.double()
    v = R.valid_mask(gt, valid, case.max_flow)
    ph, pw = pads(case.geo)
    weight, bias = case.weight.double().requires_grad_(True), case.bias.double().requires_grad_(True)
    hiddens = [x.double().requires_grad_(True) for x in case.hiddens]
    flows = [f.double().requires_grad_(True) for f in case.flows]
    zs = [F.conv2d(x, weight, bias) for x in hiddens]
    for z in zs:
        z.retain_grad()
    preds = [torch_upsample_flow(f, SCALE * z)[..., ph:, pw:] for f, z in zip(flows, zs)]
    terms = [(v[:, None] * (p - gt).abs()).mean() for p in preds]
    loss = sum(wt * term for wt, term in zip(weights(), terms))
    loss.backward()
    epe = torch.sum((preds[-1].detach() - gt) ** 2, dim=1).sqrt().reshape(-1)[v.reshape(-1)]
    np64 = lambda ts: tuple(x.detach().numpy().copy() for x in ts)  # noqa: E731
    return Truth(float(loss.detach()), tuple(float(x.detach()) for x in terms), int(v.sum()),
                 float(epe.mean()) if epe.numel() else float("nan"),
                 tuple(int((epe < th).sum()) for th in (1.0, 3.0, 5.0)), np64(preds),
                 np64([f.grad for f in flows]), np64([x.grad for x in hiddens]), np64([z.grad for z in zs]),
                 weight.grad.numpy().copy(), bias.grad.numpy().copy())


def cropped(geo):
    """[576, h, w] bool: the sub-pixels (channel 64 k + 8 i + j of coarse pixel (y, x)) that the crop removes."""
    N, h, w, H, W = geo
    ph, pw = pads(geo)
    c = np.arange(576) % 64
    i, j = (c // 8)[:, None, None], (c % 8)[:, None, None]
    y, x = np.arange(h)[None, :, None], np.arange(w)[None, None, :]
    return (8 * y + i < ph) | (8 * x + j < pw)
