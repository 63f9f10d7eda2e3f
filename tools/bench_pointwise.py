"""The two fused 1x1 convolutions of the update loop in the three precision modes: lookup + convc1
(CorrBlock.lookup_conv, corr_lookup_conv_prec) and the mask head with the convex upsampling
(upsample.mask_upsample, corr_mask_upsample_forward_prec).  Each launch in each mode is captured as
one HIP graph and replayed; the variants of a size are alternated in ONE process on the same inputs,
so box-to-box spread drops out (the method of tools/bench_gru.py --precision).
    python tools/bench_pointwise.py [--sizes dsec,b8,hires1920] [--trials 5]
                                    [--json profiles/pointwise_precision_bench.json]
Per size and launch: median / min / max ms per call over the trial windows in bf16x6, bf16x3 and
bf16, each mode's norm-relative error against an fp64 CPU evaluation of the same launch, the ratio
of each reduced mode to bf16x6, and "pays": false where a reduced mode is slower than bf16x6 beyond
the windows' spread (its fastest window slower than bf16x6's slowest).  Prints one JSON document;
--json also writes it to a file."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd import CorrBlock  # noqa: E402
from eraft_amd.model import ERAFT  # noqa: E402
from eraft_amd.upsample import mask_upsample  # noqa: E402
from eraft_amd.utils import coords_grid  # noqa: E402

# name: (B, H, W) at 1/8 resolution; fmap channels 256, 4 levels, radius 4 (E-RAFT)
SIZES = {"dsec": (1, 60, 80), "b8": (8, 36, 48), "hires1920": (1, 160, 240)}
MODES = ("bf16x6", "bf16x3", "bf16")
LAUNCHES = ("lookup_conv", "mask_upsample")


def norm_rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def bench_size(name, trials, dev):
    B, H, W = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    rnd = lambda *s, scale=1.0: torch.randn(*s, device=dev, generator=gen) * scale  # noqa: E731
    stream = torch.cuda.Stream()
    graphs, outs, keep, ref = {}, {}, [], {}
    with torch.no_grad():
        # lookup + convc1: a pyramid of unit-variance correlations, coordinates a few pixels off the grid
        blk = CorrBlock(rnd(B, 256, H, W), rnd(B, 256, H, W), num_levels=4, radius=4)
        coords = coords_grid(B, H, W, device=dev) + rnd(B, 2, H, W, scale=3.0)
        wc, bc = rnd(256, 324, 1, 1, scale=324 ** -0.5), rnd(256, scale=0.1)
        # the mask head: hidden = relu(gauss), logits of standard deviation near 1, a flow of a few pixels
        conv = torch.nn.Conv2d(256, 576, 1).to(dev)
        conv.weight.copy_(rnd(576, 256, 1, 1, scale=1.0 / (0.25 * 128 ** 0.5)))
        conv.bias.copy_(rnd(576, scale=0.4))
        hidden, flow = torch.relu(rnd(B, 256, H, W)), rnd(B, 2, H, W, scale=3.0)
        calls = {"lookup_conv": lambda p: blk.lookup_conv(coords, wc, bc, precision=p),
                 "mask_upsample": lambda p: mask_upsample(conv, hidden, 0, flow, precision=p)}
        for launch, call in calls.items():
            for mode in MODES:
                with torch.cuda.stream(stream):
                    for _ in range(2):  # warm-up: the weight packs
                        out = call(mode)
                    torch.cuda.synchronize()
                    outs[launch, mode] = out.cpu()
                    gr = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gr, stream=stream):
                        keep.append(call(mode))
                torch.cuda.synchronize()
                graphs[launch, mode] = gr
        look = blk(coords).cpu().double()
        ref["lookup_conv"] = torch.relu(torch.einsum("oc,bchw->bohw", wc.view(256, 324).cpu().double(), look)
                                        + bc.cpu().double().view(1, -1, 1, 1))
        mask = 0.25 * F.conv2d(hidden.cpu().double(), conv.weight.cpu().double(), conv.bias.cpu().double())
        ref["mask_upsample"] = ERAFT.upsample_flow(flow.cpu().double(), mask)
        del look, mask, blk
    steps = max(5, int(0.1 / (3e-5 * max(1.0, B * H * W / 4800.0))))  # ~0.1 s or more per window
    times = {k: [] for k in graphs}
    for t in range(trials + 1):
        for k, gr in graphs.items():
            gr.replay()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                gr.replay()
            torch.cuda.synchronize()
            if t:  # trial 0 warms every variant
                times[k].append((time.perf_counter() - t0) / steps * 1e3)
    res = {"B": B, "H": H, "W": W, "steps_per_window": steps, "windows": trials}
    for launch in LAUNCHES:
        r = {}
        for mode in MODES:
            v = sorted(times[launch, mode])
            r[mode] = {"call_ms_median": round(v[len(v) // 2], 5), "call_ms_min": round(v[0], 5),
                       "call_ms_max": round(v[-1], 5), "rel_err_vs_fp64": norm_rel(outs[launch, mode], ref[launch])}
        for mode in MODES[1:]:
            r[f"{mode}_over_bf16x6"] = round(r[mode]["call_ms_median"] / r["bf16x6"]["call_ms_median"], 3)
            r[f"{mode}_pays"] = not (r[mode]["call_ms_median"] > r["bf16x6"]["call_ms_median"]
                                     and r[mode]["call_ms_min"] > r["bf16x6"]["call_ms_max"])
        res[launch] = r
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
        sys.exit("bench_pointwise needs an MI355X (no CPU fallback)")
    if a.trials < 5:
        sys.exit("--trials must be >= 5 (the median of at least 5 windows is reported)")
    for n in a.sizes.split(","):
        if n not in SIZES:
            sys.exit(f"unknown size {n!r} (known: {', '.join(SIZES)})")
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0),
           "call": "one launch per HIP graph, the three modes of both launches alternated",
           "sizes": {n: bench_size(n, a.trials, dev) for n in a.sizes.split(",")}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
