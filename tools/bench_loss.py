"""The training tail, fused vs the chain it replaces: iters = 12 predictions' sequence loss, forward
and backward to every (flow_i, mask_i).
    fused   SequenceLoss.add_upsampled per iteration (corr_upsample_loss; corr_upsample_loss_bwd):
            no full-resolution prediction or gradient is stored
    chain   model._ConvexUpsampleFn (corr_convex_upsample / _bwd) per iteration, then the loss as
            torch composes it (tests/_train_ref.py's formula with the reference's `valid` mask)
Both run eagerly in ONE process on the same inputs, alternated window by window, so box-to-box
spread drops out; a step's time is wall time per step over a window that ends with a
synchronisation (the host's enqueueing of the chain's launches is part of what a trainer pays).
    python tools/bench_loss.py [--sizes dsec,b8,hires1920] [--trials 5] [--steps N] [--json profiles/loss_bench.json]
Per size: median / min / max ms per step over the windows, torch.cuda.max_memory_allocated of a
step above the inputs' own bytes, and the two losses.  Prints one JSON document.

--mask-head measures the tail with the mask head in it instead: forward and backward to every
(hidden_i, flow_i) and to the head's parameters, alternated in the same way.
    mask    today's path: torch mask[2] (MIOpen 1x1, 256 -> 576), 0.25 *, add_upsampled: a mask per
            iteration is stored and saved for backward
    hidden  SequenceLoss.add_hidden (corr_mask_upsample_loss; corr_mask_upsample_loss_bwd + the
            convolution's backward over dz): no mask is stored or saved
    python tools/bench_loss.py --mask-head --json profiles/loss_mask_head_bench.json"""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd.loss import SequenceLoss  # noqa: E402
from eraft_amd.model import _ConvexUpsampleFn  # noqa: E402

# name: (B, h, w) of the 1/8-resolution maps; the loss frame is the whole 8h x 8w (no pad)
SIZES = {"dsec": (1, 60, 80), "b8": (8, 36, 48), "hires1920": (1, 160, 240)}
ITERS, GAMMA, MAX_FLOW = 12, 0.8, 400.0


def fused_step(flows, masks, gt, valid):
    crit = SequenceLoss(gt, valid, GAMMA, MAX_FLOW)
    for i, (f, m) in enumerate(zip(flows, masks)):
        crit.add_upsampled(f, m, i, ITERS)
    loss, _ = crit.result()
    loss.backward()
    return loss.detach()


def chain_step(flows, masks, gt, valid):
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    v = (valid >= 0.5) & (mag < MAX_FLOW)
    loss = 0.0
    for i, (f, m) in enumerate(zip(flows, masks)):
        pred = _ConvexUpsampleFn.apply(f, m)
        loss = loss + GAMMA ** (ITERS - 1 - i) * (v[:, None] * (pred - gt).abs()).mean()
    epe = torch.sum((pred.detach() - gt) ** 2, dim=1).sqrt().view(-1)[v.view(-1)]
    _ = (epe.mean(), (epe < 1).float().mean(), (epe < 3).float().mean(), (epe < 5).float().mean())
    loss.backward()
    return loss.detach()


def mask_step(hiddens, flows, gt, valid, conv):
    crit = SequenceLoss(gt, valid, GAMMA, MAX_FLOW)
    for i, (x, f) in enumerate(zip(hiddens, flows)):
        crit.add_upsampled(f, 0.25 * conv(x), i, ITERS)
    loss, _ = crit.result()
    loss.backward()
    return loss.detach()


def hidden_step(hiddens, flows, gt, valid, conv):
    crit = SequenceLoss(gt, valid, GAMMA, MAX_FLOW)
    for i, (x, f) in enumerate(zip(hiddens, flows)):
        crit.add_hidden(conv, x, f, i, ITERS)
    loss, _ = crit.result()
    loss.backward()
    return loss.detach()


def run(step, args):
    for t in args[0] + args[1]:
        t.grad = None
    if len(args) > 4:
        args[4].zero_grad(set_to_none=True)
    return step(*args)


def bench_size(name, trials, dev, steps=None, mask_head=False):
    B, h, w = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    flows = [(2.0 * torch.randn(B, 2, h, w, device=dev, generator=gen)).requires_grad_(True) for _ in range(ITERS)]
    gt = 4.0 * torch.randn(B, 2, 8 * h, 8 * w, device=dev, generator=gen)
    valid = (torch.rand(B, 8 * h, 8 * w, device=dev, generator=gen) < 0.9).float()
    if mask_head:
        # relu(gauss) activations and a head whose mask has sigma 2, as the other mode's masks
        hiddens = [torch.relu(torch.randn(B, 256, h, w, device=dev, generator=gen)).requires_grad_(True)
                   for _ in range(ITERS)]
        conv = torch.nn.Conv2d(256, 576, 1).to(dev)
        with torch.no_grad():
            conv.weight.copy_(8.0 / 128 ** 0.5 * torch.randn(576, 256, 1, 1, device=dev, generator=gen))
        args = (hiddens, flows, gt, valid, conv)
        variants, (old, new) = {"mask": mask_step, "hidden": hidden_step}, ("mask", "hidden")
    else:
        masks = [(2.0 * torch.randn(B, 576, h, w, device=dev, generator=gen)).requires_grad_(True) for _ in range(ITERS)]
        args = (flows, masks, gt, valid)
        variants, (old, new) = {"chain": chain_step, "fused": fused_step}, ("chain", "fused")
    steps = steps or max(5, int(200 / max(1.0, B * h * w / 4800.0)))  # windows of about half a second
    res = {"B": B, "h": h, "w": w, "H": 8 * h, "W": 8 * w, "iters": ITERS, "steps_per_window": steps, "windows": trials}
    times = {n: [] for n in variants}
    for n, step in variants.items():  # warm up, then the peak memory of one step above what is live before it
        for _ in range(2):
            loss = run(step, args)
        for t in args[0] + args[1]:
            t.grad = None
        if mask_head:
            conv.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        loss = run(step, args)
        torch.cuda.synchronize()
        res[n] = {"loss": float(loss), "peak_bytes_above_inputs": torch.cuda.max_memory_allocated() - base}
    for t in range(trials):
        for n, step in variants.items():
            run(step, args)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                run(step, args)
            torch.cuda.synchronize()
            times[n].append((time.perf_counter() - t0) / steps * 1e3)
    for n, v in times.items():
        v = sorted(v)
        res[n].update({"step_ms_median": round(v[len(v) // 2], 4), "step_ms_min": round(v[0], 4),
                       "step_ms_max": round(v[-1], 4)})
    res[f"{new}_over_{old}_time"] = round(res[new]["step_ms_median"] / res[old]["step_ms_median"], 3)
    res[f"{new}_over_{old}_peak"] = round(res[new]["peak_bytes_above_inputs"] / res[old]["peak_bytes_above_inputs"], 3)
    del flows, args
    hiddens = masks = conv = None  # noqa: F841  (before empty_cache)
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dsec,b8,hires1920")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--steps", type=int, default=None, help="steps per window (default: by size; small under a profiler)")
    ap.add_argument("--mask-head", action="store_true", help="the tail with the mask head in it: mask[2] + add_upsampled "
                    "against add_hidden")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_loss needs an MI355X (the fused path has no CPU kernels)")
    if a.trials < 5:
        sys.exit("--trials must be >= 5 (the median of at least 5 windows is reported)")
    dev = torch.device("cuda", 0)
    call = ("12 iterations' sequence loss, forward + backward to every (flow_i, mask_i), eager, variants "
            "alternated; chain: corr_convex_upsample + torch loss + corr_convex_upsample_bwd; fused: "
            "corr_upsample_loss + corr_upsample_loss_bwd")
    if a.mask_head:
        call = ("12 iterations' mask head + sequence loss, forward + backward to every (hidden_i, flow_i) and to the "
                "head's parameters, eager, variants alternated; mask: torch mask[2], 0.25 *, corr_upsample_loss / _bwd; "
                "hidden: corr_mask_upsample_loss, corr_mask_upsample_loss_bwd + aten convolution_backward over dz")
    doc = {"device": torch.cuda.get_device_name(0), "call": call,
           "sizes": {n: bench_size(n, a.trials, dev, a.steps, a.mask_head) for n in a.sizes.split(",")}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
