"""Fused SepConvGRU (corr_gru_half_step x 2) vs the torch / MIOpen module: one full GRU call (both
half steps), each variant captured as one HIP graph and replayed; the variants of a size are
alternated in ONE process on the same inputs, so box-to-box spread drops out.
    python tools/bench_gru.py [--sizes dsec,b8,hires1920] [--trials 5] [--json profiles/gru_bench.json]
                              [--precision bf16x3,bf16]
Per size: median / min / max ms per call of both paths over the trial windows, and each path's
norm-relative error against an fp64 CPU run of the same module.  --precision adds the fused path in
each named reduced mode (variants fused_<mode>, eraft_amd/precision.py) beside "fused" (bf16x6) and
"torch", alternated with them in the same windows, and their ratio to "fused".  Prints one JSON
document; --json also writes it to a file."""
import argparse
import copy
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd.model import SepConvGRU  # noqa: E402
from eraft_amd.precision import code  # noqa: E402

# name: (B, H, W)   hidden = 128, input = 320 (E-RAFT's update block)
SIZES = {"dsec": (1, 60, 80), "b8": (8, 36, 48), "hires1920": (1, 160, 240)}
HID, INP = 128, 320


def norm_rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def bench_size(name, trials, dev, modes=()):
    B, H, W = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    m = SepConvGRU(HID, INP).to(dev).eval()
    h = torch.tanh(torch.randn(B, HID, H, W, device=dev, generator=gen))
    x = torch.randn(B, INP, H, W, device=dev, generator=gen)
    stream = torch.cuda.Stream()
    graphs, outs, keep = {}, {}, []
    with torch.no_grad():
        variants = [("torch", False, "bf16x6"), ("fused", True, "bf16x6")] + [(f"fused_{p}", True, p) for p in modes]
        for vname, fused, prec in variants:
            SepConvGRU.fused, m.precision = fused, prec
            with torch.cuda.stream(stream):
                for _ in range(2):  # warm-up: MIOpen's solver search / the weight packs
                    out = m(h, x)
                torch.cuda.synchronize()
                outs[vname] = out.clone()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    keep.append(m(h, x))
            torch.cuda.synchronize()
            graphs[vname] = gr
        SepConvGRU.fused, m.precision = False, "bf16x6"
        ref = copy.deepcopy(m).cpu().double()(h.cpu().double(), x.cpu().double())
    steps = max(5, int(0.2 / (1e-3 * max(1.0, B * H * W / 4800.0))))  # ~0.2 s or more per window
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
    res = {"B": B, "H": H, "W": W, "hidden": HID, "input": INP, "steps_per_window": steps, "windows": trials}
    for n, v in times.items():
        v = sorted(v)
        res[n] = {"call_ms_median": round(v[len(v) // 2], 4), "call_ms_min": round(v[0], 4),
                  "call_ms_max": round(v[-1], 4), "rel_err_vs_fp64": norm_rel(outs[n].cpu(), ref)}
    res["fused_over_torch"] = round(res["fused"]["call_ms_median"] / res["torch"]["call_ms_median"], 3)
    for p in modes:
        res[f"fused_{p}_over_fused"] = round(res[f"fused_{p}"]["call_ms_median"] / res["fused"]["call_ms_median"], 3)
    del graphs, keep
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dsec,b8,hires1920")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--precision", default="", help="reduced modes to time beside bf16x6, e.g. bf16x3,bf16")
    a = ap.parse_args()
    modes = tuple(p for p in a.precision.split(",") if p)
    for p in modes:
        if code(p) == 0:
            sys.exit("--precision names the reduced modes; bf16x6 is the variant 'fused'")
    if not torch.cuda.is_available():
        sys.exit("bench_gru needs an MI355X (no CPU fallback)")
    if a.trials < 5:
        sys.exit("--trials must be >= 5 (the median of at least 5 windows is reported)")
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0),
           "call": "SepConvGRU.forward (both half steps), one HIP graph per variant, variants alternated",
           "sizes": {n: bench_size(n, a.trials, dev, modes) for n in a.sizes.split(",")}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
