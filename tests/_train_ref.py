"""Harness of tests/test_train_parity.py: one training step of the project's own ERAFT module
(eraft_amd/model.py), run as three legs with the same weights, inputs and loss.

  fp64 CPU leg          the truth.  model.py in fp64 on the CPU with two names of eraft_amd.model
                        substituted for the run: CorrBlock by TorchCorrBlock (below, the op chain
                        of oracle/torch_ops.py) and coords_grid by a wrapper that returns the
                        leg's dtype.  model.py rounds the feature maps to fp32 at the CorrBlock
                        call (`.float()`); TorchCorrBlock casts them up again and that one
                        rounding is accepted (the GPU's maps are fp32 anyway).
  fp32 torch-only leg   the floor: the same substitutions in fp32, on the CPU and on the GPU.  On
                        the GPU ERAFT.upsample_flow is also replaced by the torch composition that
                        model.py runs for CPU tensors, so the leg holds no HIP kernel of this
                        project: it measures what fp32 and MIOpen alone cost.
  HIP leg               the model as shipped on cuda:0, with whatever switches the test has set.

A leg returns a Leg: the low-resolution flow, every prediction, every parameter's gradient, the
gradients that arrive at fnet's two outputs and at cnet's output (a forward hook calls
retain_grad() on them), the batch norms' running statistics after the step, and the inputs of the
update block's ReLUs (reference_legs says why).  The reference legs are cached per configuration
and never modified.
"""
from __future__ import annotations

import contextlib
import functools
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import prng

DEV = "cuda:0"
BINS = 5
BOUNDARY = ("fnet.out1", "fnet.out2", "cnet.out")
# every switch of model.py that selects one of this project's inference kernels; the reference
# legs run with all of them off, whatever the process's environment says
# the update block's convolutions whose output goes into a ReLU (reference_legs)
KINK_SITES = ("encoder.convc1", "encoder.convc2", "encoder.convf1", "encoder.convf2", "encoder.conv",
              "flow_head.conv1", "mask.0")
SWITCHES = (("BasicEncoder", "fused"), ("SepConvGRU", "fused"), ("BasicUpdateBlock", "fused"),
            ("ERAFT", "fuse_mask_upsample"), ("ERAFT", "fuse_ondemand_conv"))


@dataclass(frozen=True)
class Config:
    """What all three legs of a case share.  The HIP leg's switches are not part of it."""
    H: int = 128
    W: int = 160
    B: int = 1
    iters: int = 3
    train: bool = False      # train(): batch statistics in cnet's batch norms
    warm: bool = False       # flow_init = prng.gauss(sigma 1.5) at the feature maps' size
    freeze: str = ""         # "encoders" (fnet and cnet) or "update" (the update block)
    steps: int = 1           # 2: an in-place update with the fp64 leg's gradient, then a second step
    two_losses: bool = False  # the sequence loss plus a linear loss over one forward
    seed: int = 421          # of the images, the ground truth, flow_init and the linear loss


class Leg(NamedTuple):
    low: np.ndarray
    preds: tuple
    grads: dict      # parameter name -> gradient, None where the parameter has none
    boundary: dict   # BOUNDARY name -> gradient, None where the output carries none
    stats: dict      # batch norms' running_mean / running_var after the step
    acts: dict       # KINK_SITES name -> that convolution's output (a ReLU's input), per call


# ---------------------------------------------------------------------------------------------
# the reference CorrBlock, device-aware
# ---------------------------------------------------------------------------------------------
def torch_build(fmap1, fmap2, num_levels=4):
    """oracle/torch_ops.py cpu_build on fmap1's device (bit-identical on CPU tensors)."""
    B, D, H, W = fmap1.shape
    a = fmap1.reshape(B, D, H * W).transpose(1, 2)
    c = torch.matmul(a, fmap2.reshape(B, D, H * W))
    c = c / torch.sqrt(torch.tensor(D, device=fmap1.device).float())
    level = c.reshape(B * H * W, 1, H, W)
    levels = [level]
    for _ in range(num_levels - 1):
        level = F.avg_pool2d(level, 2, stride=2)
        levels.append(level)
    return levels


def torch_lookup(levels, coords, radius=4):
    """oracle/torch_ops.py cpu_lookup with its window offsets on coords' device."""
    B, _, H, W = coords.shape
    S = 2 * radius + 1
    off = torch.arange(-radius, radius + 1, dtype=torch.float32, device=coords.device)
    ox = off.view(S, 1).expand(S, S)
    oy = off.view(1, S).expand(S, S)
    delta = torch.stack([ox, oy], dim=-1).view(1, S, S, 2)
    centre = coords.permute(0, 2, 3, 1).reshape(B * H * W, 1, 1, 2)
    outs = []
    for l, lvl in enumerate(levels):
        h, w = lvl.shape[-2:]
        g = centre / 2 ** l + delta
        gx = 2 * g[..., 0:1] / (w - 1) - 1
        gy = 2 * g[..., 1:2] / (h - 1) - 1
        s = F.grid_sample(lvl, torch.cat([gx, gy], dim=-1), align_corners=True)
        outs.append(s.view(B, H, W, S * S))
    return torch.cat(outs, dim=-1).permute(0, 3, 1, 2).contiguous()


def torch_upsample_flow(flow, mask):
    """The torch composition ERAFT.upsample_flow runs for CPU tensors, on any device."""
    n, _, h, w = flow.shape
    mask = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(n, 2, 8 * h, 8 * w)


@contextlib.contextmanager
def substituted(dtype, torch_upsample):
    """eraft_amd.model with CorrBlock, coords_grid (and upsample_flow) substituted and every
    inference switch off, for a reference leg of `dtype`; undone on exit."""
    import eraft_amd.model as M

    class TorchCorrBlock:
        def __init__(self, f1, f2, num_levels=4, radius=4):
            self.levels, self.radius = torch_build(f1.to(dtype), f2.to(dtype), num_levels), radius

        def __call__(self, coords):
            return torch_lookup(self.levels, coords, self.radius)

    grid = M.coords_grid
    saved = [(M, "CorrBlock", M.CorrBlock), (M, "coords_grid", grid)]
    saved += [(getattr(M, c), a, getattr(M, c).__dict__[a]) for c, a in SWITCHES]
    if torch_upsample:
        saved.append((M.ERAFT, "upsample_flow", M.ERAFT.__dict__["upsample_flow"]))
    try:
        M.CorrBlock = TorchCorrBlock
        M.coords_grid = lambda *a, **k: grid(*a, **k).to(dtype)
        for c, a in SWITCHES:
            setattr(getattr(M, c), a, False)
        if torch_upsample:
            M.ERAFT.upsample_flow = staticmethod(torch_upsample_flow)
        yield
    finally:
        for obj, name, val in saved:
            setattr(obj, name, val)


# ---------------------------------------------------------------------------------------------
# one leg
# ---------------------------------------------------------------------------------------------
def make_model(cfg, alternate=False):
    from eraft_amd.model import ERAFT
    m = ERAFT({"subtype": "warm_start" if cfg.warm else "standard", "alternate_corr": alternate},
              n_first_channels=BINS)
    with torch.no_grad():
        for name, t in m.state_dict().items():
            v = prng.param_init(name, tuple(t.shape))
            if v is not None:
                t.copy_(torch.from_numpy(v))
    m.train(cfg.train)
    frozen = {"": (), "encoders": (m.fnet, m.cnet), "update": (m.update_block,)}[cfg.freeze]
    for part in frozen:
        part.requires_grad_(False)
    return m


def structural_zero(model):
    """Names of the parameters whose gradient is 0 in exact arithmetic: the bias of a convolution
    that feeds an instance norm, or a batch norm that normalises with batch statistics, shifts the
    norm's input, which changes nothing.  Derived from the encoders' modules (model.py)."""
    def shift_invariant(norm):
        return isinstance(norm, nn.InstanceNorm2d) or (isinstance(norm, nn.BatchNorm2d) and norm.training)

    names = {id(p): n for n, p in model.named_parameters()}
    out = set()
    for enc in (model.fnet, model.cnet):
        pairs = [(enc.conv1, enc.norm1)]
        for layer in (enc.layer1, enc.layer2, enc.layer3):
            for blk in layer:
                pairs += [(blk.conv1, blk.norm1), (blk.conv2, blk.norm2)]
                if blk.downsample is not None:
                    pairs.append((blk.downsample[0], blk.downsample[1]))
        out |= {names[id(conv.bias)] for conv, norm in pairs if shift_invariant(norm) and conv.bias.requires_grad}
    return out


def inputs(cfg):
    """(im1, im2, gt, flow_init or None, (G_i ...)) as fp32 numpy; the same for every leg."""
    B, H, W = cfg.B, cfg.H, cfg.W
    hp, wp = -(-H // 32) * 32, -(-W // 32) * 32  # ERAFT's padder: multiples of 32
    im1 = prng.voxel_grid(cfg.seed, (B, BINS, H, W))
    im2 = prng.voxel_grid(cfg.seed + 2, (B, BINS, H, W))
    gt = prng.gauss(cfg.seed + 4, (B, 2, H, W), 2.0)
    finit = prng.gauss(cfg.seed + 6, (B, 2, hp // 8, wp // 8), 1.5) if cfg.warm else None
    G = tuple(prng.gauss(cfg.seed + 10 + i, (B, 2, H, W)) for i in range(cfg.iters)) if cfg.two_losses else ()
    return im1, im2, gt, finit, G


def _np(t):
    return None if t is None else t.detach().double().cpu().numpy()


def _step(model, cfg, dtype, device, split_backward, sides=()):
    """One forward and backward -> Leg.  split_backward: the two losses are two backward calls
    over one forward (the HIP leg); otherwise one backward of their sum.  sides: (site, call, flat
    index, sign) of units that take the given side of their ReLU's kink (reference_legs)."""
    def put(a):
        return None if a is None else torch.from_numpy(a).to(device, dtype)

    im1, im2, gt, finit, G = inputs(cfg)
    im1, im2, gt, finit, G = put(im1), put(im2), put(gt), put(finit), [put(g) for g in G]
    model.zero_grad(set_to_none=True)
    kept = {}

    def keep(names):
        def hook(_mod, _inp, out):
            for n, o in zip(names, out if isinstance(out, (tuple, list)) else (out,)):
                kept[n] = o
                if o.requires_grad:
                    o.retain_grad()
        return hook

    acts = {name: [] for name in KINK_SITES}

    def site_hook(name):
        def hook(_mod, _inp, out):
            mine = [(i, sg) for site, call, i, sg in sides if site == name and call == len(acts[name])]
            if mine:
                # a unit on the other side moves to the smallest number on the given side (a change of
                # |x|, within the noise that made it ambiguous); the gradient passes unchanged
                idx = torch.tensor([i for i, _ in mine], device=out.device)
                sg = torch.tensor([sg for _, sg in mine], device=out.device, dtype=out.dtype)
                flat = out.detach().reshape(-1)
                move = (flat[idx] > 0) != (sg > 0)
                target, moved = torch.zeros_like(flat), torch.zeros_like(flat, dtype=torch.bool)
                target[idx[move]], moved[idx[move]] = sg[move] * torch.finfo(out.dtype).tiny, True
                out = torch.where(moved.view_as(out), target.view_as(out) + (out - out.detach()), out)
            acts[name].append(_np(out.clone()))  # a copy: some of the ReLUs work in place
            return out
        return hook

    handles = [model.fnet.register_forward_hook(keep(BOUNDARY[:2])),
               model.cnet.register_forward_hook(keep(BOUNDARY[2:])),
               *(model.update_block.get_submodule(n).register_forward_hook(site_hook(n)) for n in KINK_SITES)]
    try:
        low, preds = model(im1, im2, iters=cfg.iters, flow_init=finit)
    finally:
        for h in handles:
            h.remove()
    n = len(preds)
    seq = sum(0.8 ** (n - 1 - i) * (p - gt).abs().mean() for i, p in enumerate(preds))
    if cfg.two_losses:
        lin = sum((p * g).mean() for p, g in zip(preds, G))
        if split_backward:
            seq.backward(retain_graph=True)
            lin.backward()
        else:
            (seq + lin).backward()
    else:
        seq.backward()
    stats = {k: _np(v) for k, v in model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
    return Leg(_np(low), tuple(_np(p) for p in preds), {k: _np(p.grad) for k, p in model.named_parameters()},
               {k: _np(kept[k].grad) for k in BOUNDARY}, stats, {k: tuple(v) for k, v in acts.items()})


def _lr(g64):
    """Step size of the two-step case: the largest entry of the fp64 gradient moves its weight by
    0.05 (the convolution weights are of order 0.03 .. 0.3)."""
    return 0.05 / max(np.abs(g).max() for g in g64.values() if g is not None)


def _run(cfg, dtype, device, model, split_backward=False, sides=()):
    """cfg.steps steps of `model` -> the last step's Leg (`sides` act on the last step)."""
    model = model.to(device=device, dtype=dtype)
    leg = _step(model, cfg, dtype, device, split_backward, sides if cfg.steps == 1 else ())
    for k in range(cfg.steps - 1):
        # the same update in every leg: the fp64 leg's gradient of the first step, cast to fp32
        g64 = fp64_leg(_first_step(cfg)).grads
        lr = _lr(g64)
        with torch.no_grad():
            for name, p in model.named_parameters():
                if g64[name] is not None:
                    p.sub_((lr * torch.from_numpy(g64[name]).float()).to(device, dtype))
        leg = _step(model, cfg, dtype, device, split_backward, sides if k == cfg.steps - 2 else ())
    return leg


def _first_step(cfg):
    return Config(**{**cfg.__dict__, "steps": 1})


@functools.lru_cache(maxsize=None)
def fp64_leg(cfg, sides=()):
    with substituted(torch.float64, torch_upsample=False):
        return _run(cfg, torch.float64, "cpu", make_model(cfg), sides=sides)


@functools.lru_cache(maxsize=None)
def fp32_cpu_leg(cfg, sides=()):
    with substituted(torch.float32, torch_upsample=False):
        return _run(cfg, torch.float32, "cpu", make_model(cfg), sides=sides)


@functools.lru_cache(maxsize=None)
def fp32_gpu_leg(cfg, sides=()):
    with substituted(torch.float32, torch_upsample=True):
        return _run(cfg, torch.float32, DEV, make_model(cfg), sides=sides)


def hip_leg(cfg, alternate=False):
    """The code under test: the model as shipped on the GPU, with the switches the caller has set."""
    model = make_model(cfg, alternate)
    assert model.alternate_corr is alternate
    return _run(cfg, torch.float32, DEV, model, split_backward=True)


@functools.lru_cache(maxsize=None)
def zero_set(cfg):
    return frozenset(structural_zero(make_model(cfg)))


def reference_legs(cfg, hip, factor):
    """(fp64, fp32 CPU, fp32 torch-only GPU) legs to hold `hip` against, and a note for the log.

    A ReLU unit whose pre-activation lies within fp32 rounding noise of 0 is on or off by chance in
    every fp32 run, and the gradient jumps with it: at such a unit the truth has two values.  For
    the encoders' units the jump is far below any bar of the module.  In the update block it is
    not: one unit of flow_head.conv1 flipping (245760 units over 3 iterations, pre-activations of
    order 1, fp32 deviations of order 1e-6, so the fp64 leg always has a few units that close to
    0) moves the boundary gradients and most parameters' gradients by 2e-3 .. 6e-3 norm_rel,
    between two runs of one torch-only leg as much as between it and the HIP leg (measured on the
    CPU and on an MI355X).  So the legs record the input of every ReLU of the update block that
    follows a torch convolution (KINK_SITES), and where they disagree about an ambiguous unit the
    reference legs are run again with every ambiguous unit on the HIP leg's side of the kink (a
    unit on the other side is moved to the smallest number on the HIP leg's side, a change within
    the noise that made it ambiguous), and the comparison is with those.  Ambiguous: |fp64
    pre-activation| <= factor * the fp32 reference legs' largest deviation from fp64 at that
    site, the bound of the module's own bar.  A sign that differs at any other unit is an error of
    the forward pass and fails.  (convc1's ReLU is inside the kernel when the lookup is fused with
    it; such a site has no record in the HIP leg and is left alone.)"""
    legs = [fp64_leg(cfg), fp32_cpu_leg(cfg), fp32_gpu_leg(cfg)]
    truth = legs[0]
    sides, agree, widest = [], True, 0.0
    for site in KINK_SITES:
        if not hip.acts[site]:
            continue
        scale = max(np.abs(a).max() for a in truth.acts[site])
        dev = max(np.abs(a - b).max() for leg in legs[1:] for a, b in zip(leg.acts[site], truth.acts[site]))
        tau = factor * dev
        widest = max(widest, tau / scale)
        for call, (t, h) in enumerate(zip(truth.acts[site], hip.acts[site])):
            t, h = t.reshape(-1), h.reshape(-1)
            near = np.abs(t) <= tau
            wrong = np.flatnonzero(((t > 0) != (h > 0)) & ~near)
            assert wrong.size == 0, (f"{site}, call {call}: {wrong.size} units on the other side of the ReLU with "
                                     f"|fp64 pre-activation| up to {np.abs(t[wrong]).max():.2e} > {tau:.2e}")
            idx = np.flatnonzero(near)
            sides += [(site, call, int(i), 1.0 if h[i] > 0 else -1.0) for i in idx]
            agree = agree and all(np.array_equal(leg.acts[site][call].reshape(-1)[idx] > 0, h[idx] > 0) for leg in legs)
    note = f"{len(sides)} update-block units within {widest:.1e} (relative) of a ReLU's kink"
    if agree:
        return (*legs, note + ", every leg on the same side")
    sides = tuple(sides)
    return fp64_leg(cfg, sides), fp32_cpu_leg(cfg, sides), fp32_gpu_leg(cfg, sides), note + ", references rerun on the HIP leg's side"
