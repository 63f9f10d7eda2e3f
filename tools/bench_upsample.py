"""The mask head fused with the convex upsampling (corr_mask_upsample_forward) vs the torch chain it
replaces: 0.25 * mask[2](hidden) (a 256 -> 576 1x1 convolution on rocBLAS / MIOpen and a torch
elementwise scale, the 576-channel mask written and re-read) then corr_convex_upsample.
Every variant is captured as one HIP graph and replayed; the variants are alternated in ONE process
on the same inputs, so box-to-box spread drops out.
    python tools/bench_upsample.py [--sizes dsec,b8,hires1920] [--trials 5] [--json profiles/upsample_bench.json]
Per size: the torch chain and the fused launch (median / min / max ms per call over the trial
windows), the chain's three pieces on their own (the convolution, the scale, the upsampling: where
its time goes), and both paths' norm-relative error against the fp64 formula on the CPU.  Prints
one JSON document; --json also writes it to a file."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd.model import ERAFT  # noqa: E402
from eraft_amd.upsample import mask_upsample  # noqa: E402

# name: (B, H, W)
SIZES = {"dsec": (1, 60, 80), "b8": (8, 36, 48), "hires1920": (1, 160, 240)}


def norm_rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def capture(fn, stream):
    """fn warmed up twice (MIOpen's solver search, the weight pack), then captured."""
    with torch.no_grad(), torch.cuda.stream(stream):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=stream):
            keep = fn()
    torch.cuda.synchronize()
    return gr, out, keep


def alternate(graphs, trials, steps):
    times = {n: [] for n in graphs}
    for t in range(trials + 1):
        for n, gr in graphs.items():
            gr.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                gr.replay()
            torch.cuda.synchronize()
            if t:  # trial 0 warms every variant
                times[n].append((time.perf_counter() - t0) / steps * 1e3)
    res = {}
    for n, v in times.items():
        v = sorted(v)
        res[n] = {"call_ms_median": round(v[len(v) // 2], 4), "call_ms_min": round(v[0], 4),
                  "call_ms_max": round(v[-1], 4)}
    return res


def upsample64(flow, mask):
    """The torch branch of ERAFT.upsample_flow (the reference's eraft.py:75-86), fp64 on the CPU."""
    return ERAFT.upsample_flow(flow, mask)


def bench_size(name, trials, dev):
    B, H, W = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    head = torch.nn.Conv2d(256, 576, 1).to(dev).eval()
    hd = torch.relu(torch.randn(B, 512, H, W, device=dev, generator=gen))  # [flow_head.conv1 | mask[0]]
    flow = 2.0 * torch.randn(B, 2, H, W, device=dev, generator=gen)
    hidden = hd[:, 256:]  # the update block's view: the torch chain reads it as MIOpen does today
    stream = torch.cuda.Stream()
    steps = max(5, int(2000 / max(1.0, B * H * W / 4800.0)))  # windows of 0.05 - 0.1 s at 25 - 90 us per call
    res = {"B": B, "H": H, "W": W, "steps_per_window": steps, "windows": trials}
    mask_fixed = (0.25 * head(hidden)).detach()
    conv_fixed = head(hidden).detach()
    variants = {
        "torch": lambda: ERAFT.upsample_flow(flow, 0.25 * head(hidden)),
        "fused": lambda: mask_upsample(head, hd, 256, flow),
        "torch_conv_only": lambda: head(hidden),
        "torch_scale_only": lambda: 0.25 * conv_fixed,
        "torch_upsample_only": lambda: ERAFT.upsample_flow(flow, mask_fixed),
    }
    graphs, outs, keep = {}, {}, []
    for vname, fn in variants.items():
        graphs[vname], outs[vname], k = capture(fn, stream)
        keep.append(k)
    r = alternate(graphs, trials, steps)
    with torch.no_grad():
        mask = 0.25 * F.conv2d(hidden.cpu().double(), head.weight.cpu().double(), head.bias.cpu().double())
        ref = upsample64(flow.cpu().double(), mask)
    for vname in ("torch", "fused"):
        r[vname]["rel_err_vs_fp64"] = norm_rel(outs[vname].cpu(), ref)
    r["fused_over_torch"] = round(r["fused"]["call_ms_median"] / r["torch"]["call_ms_median"], 3)
    res.update(r)
    del graphs, keep
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dsec,b8,hires1920")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_upsample needs an MI355X (no CPU fallback)")
    if a.trials < 5:
        sys.exit("--trials must be >= 5 (the median of at least 5 windows is reported)")
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0),
           "call": "one HIP graph per variant, variants alternated; torch: 0.25 * mask[2](hidden) then "
                   "corr_convex_upsample; fused: one corr_mask_upsample_forward launch; hidden is channels "
                   "256 .. 511 of the update block's heads buffer in both",
           "sizes": {n: bench_size(n, a.trials, dev) for n in a.sizes.split(",")}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
