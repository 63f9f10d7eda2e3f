"""The update block's 3x3 convolutions on corr_conv_forward vs the torch / MIOpen ops they replace.
Every variant is captured as one HIP graph and replayed; the variants of a measurement are
alternated in ONE process on the same inputs, so box-to-box spread drops out.
    python tools/bench_update.py [--sizes dsec,b8,hires1920] [--trials 5] [--json profiles/update_bench.json]
Per size:
  (a) each of the four launches (convc2, convf2, conv, the stacked heads) against the torch ops it
      replaces: conv + bias + ReLU and the cat it removes (convf2 carries cat([c, f]); conv carries
      cat([out, flow]) and cat([inp, motion]) on the torch side and the copies of inp and flow
      into the GRU input on the kernel side);
  (b) one whole BasicUpdateBlock call (lookup already through convc1, the GRU by its own switch)
      with the switch off, with every convolution on the kernel ("all"), and with the committed
      table update.USE_KERNEL ("fused").
Median / min / max ms per call over the trial windows, and the kernel's norm-relative error
against an fp64 CPU run.  Prints one JSON document; --json also writes it to a file."""
import argparse
import copy
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd import _lib, update  # noqa: E402
from eraft_amd.model import BasicUpdateBlock  # noqa: E402

# name: (B, H, W)
SIZES = {"dsec": (1, 60, 80), "b8": (8, 36, 48), "hires1920": (1, 160, 240)}


def norm_rel(a, b):
    return float((a.double() - b).abs().max() / b.abs().max())


def capture(fn, stream):
    """fn warmed up twice (MIOpen's solver search, the weight packs), then captured."""
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


def bench_size(name, trials, dev):
    B, H, W = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    torch.manual_seed(1234)
    m = BasicUpdateBlock().to(dev).eval()
    enc = m.encoder
    rnd = lambda c: torch.randn(B, c, H, W, device=dev, generator=gen)
    net, inp, c1, flow = torch.tanh(rnd(128)), torch.relu(rnd(128)), torch.relu(rnd(256)), rnd(2)
    f1, c, f = torch.relu(rnd(128)), torch.relu(rnd(192)), torch.relu(rnd(64))
    cf = torch.cat([c, f], dim=1)
    stream = torch.cuda.Stream()
    steps = max(5, int(0.2 / (1e-3 * max(1.0, B * H * W / 4800.0))))  # ~0.2 s or more per window
    res = {"B": B, "H": H, "W": W, "steps_per_window": steps, "windows": trials, "launches": {}}
    buf = lambda ch: torch.empty(B, ch, H, W, device=dev)
    cfb, xb, hdb = buf(256), buf(256), buf(512)

    def kernel_conv(convs, x, out, off):
        packed, bias = update._conv_pack(convs)
        return _lib.conv_forward(x, None, packed, bias, sum(k.out_channels for k in convs), True, out=out,
                                 out_offset=off)

    def fused_conv():
        xb[:, :128].copy_(inp)
        xb[:, 254:].copy_(flow)
        return kernel_conv((enc.conv,), cf, xb, 128)

    heads = (m.flow_head.conv1, m.mask[0])
    pairs = {
        "convc2": (lambda: F.relu(enc.convc2(c1)),
                   lambda: kernel_conv((enc.convc2,), c1, cfb, 0),
                   lambda o: o[:, :192]),
        "convf2": (lambda: torch.cat([c, F.relu(enc.convf2(f1))], dim=1),
                   lambda: kernel_conv((enc.convf2,), f1, cfb, 192),
                   lambda o: o[:, 192:]),
        "conv": (lambda: torch.cat([inp, torch.cat([F.relu(enc.conv(cf)), flow], dim=1)], dim=1),
                 fused_conv,
                 lambda o: o[:, 128:254]),
        "heads": (lambda: (F.relu(heads[0](net)), F.relu(heads[1](net))),
                  lambda: kernel_conv(heads, net, hdb, 0),
                  lambda o: o),
    }
    for lname, (torch_fn, kernel_fn, window) in pairs.items():
        gt, ot, kt = capture(torch_fn, stream)
        gk, ok, kk = capture(kernel_fn, stream)
        r = alternate({"torch": gt, "kernel": gk}, trials, steps)
        ot = torch.cat(ot, dim=1) if isinstance(ot, tuple) else ot
        ot = {"convc2": ot, "convf2": ot[:, 192:], "conv": ot[:, 128:254], "heads": ot}[lname]
        convs = {"convc2": (enc.convc2,), "convf2": (enc.convf2,), "conv": (enc.conv,), "heads": heads}[lname]
        x = {"convc2": c1, "convf2": f1, "conv": cf, "heads": net}[lname]
        with torch.no_grad():
            ref = torch.cat([F.relu(F.conv2d(x.cpu().double(), k.weight.cpu().double(), k.bias.cpu().double(),
                                             padding=1)) for k in convs], dim=1)
        r["kernel"]["rel_err_vs_fp64"] = norm_rel(window(ok).cpu(), ref)
        r["torch"]["rel_err_vs_fp64"] = norm_rel(ot.cpu(), ref)
        r["kernel_over_torch"] = round(r["kernel"]["call_ms_median"] / r["torch"]["call_ms_median"], 3)
        res["launches"][lname] = r
        del gt, gk, kt, kk

    # (b) the whole block
    table = dict(update.USE_KERNEL)
    graphs, outs, keep = {}, {}, []
    for vname, on, tab in (("torch", False, table), ("all", True, dict.fromkeys(table, True)), ("fused", True, table)):
        BasicUpdateBlock.fused = on
        update.USE_KERNEL.update(tab)
        graphs[vname], outs[vname], k = capture(lambda: m(net, inp, c1, flow, True), stream)
        keep.append(k)
    BasicUpdateBlock.fused = False
    update.USE_KERNEL.update(table)
    with torch.no_grad():
        ref = copy.deepcopy(m).cpu().double()(*(t.cpu().double() for t in (net, inp, c1, flow)), True)
    r = alternate(graphs, trials, steps)
    for vname in graphs:
        r[vname]["rel_err_vs_fp64"] = {nm: norm_rel(o.cpu(), q) for nm, o, q in
                                       zip(("net", "mask", "delta_flow"), outs[vname], ref)}
    r["use_kernel"] = table
    r["gru_fused"] = bool(type(m.gru).fused)
    r["fused_over_torch"] = round(r["fused"]["call_ms_median"] / r["torch"]["call_ms_median"], 3)
    r["all_over_torch"] = round(r["all"]["call_ms_median"] / r["torch"]["call_ms_median"], 3)
    res["block"] = r
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
        sys.exit("bench_update needs an MI355X (no CPU fallback)")
    if a.trials < 5:
        sys.exit("--trials must be >= 5 (the median of at least 5 windows is reported)")
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0),
           "call": "one HIP graph per variant, variants alternated; launches: kernel vs the torch ops it replaces; "
                   "block: BasicUpdateBlock.forward on relu(convc1(lookup))",
           "sizes": {n: bench_size(n, a.trials, dev) for n in a.sizes.split(",")}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
