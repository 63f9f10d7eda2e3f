"""The update block's 3x3 convolutions on corr_conv_forward vs the torch / MIOpen ops they replace.
Every variant is captured as one HIP graph and replayed; the variants of a measurement are
alternated in ONE process on the same inputs, so box-to-box spread drops out.
    python tools/bench_update.py [--sizes dsec,b8,hires1920] [--trials 5] [--json profiles/update_bench.json]
                                 [--precision bf16x3,bf16]
--precision adds, for each named reduced mode (eraft_amd/precision.py), the variant kernel_<mode> to
the four corr_conv_forward launches of (a) and iter_tail_<mode> (the block and its GRU in that mode;
the GRU is fused only under ERAFT_AMD_FUSE_GRU=1) to (b), alternated with the others in the same
windows, and their ratios to "kernel" and "iter_tail" (bf16x6).
Per size:
  (a) each of the four launches (convc2, convf2, conv, the stacked heads) against the torch ops it
      replaces: conv + bias + ReLU and the cat it removes (convf2 carries cat([c, f]); conv carries
      cat([out, flow]) and cat([inp, motion]) on the torch side and the copies of inp and flow
      into the GRU input on the kernel side); and the tail's two launches: convf1
      (corr_flow_enc_forward against conv + ReLU + .contiguous() + the flow's copy) and flow_head2
      (corr_flow_head_forward against the conv + coords1 + delta + coords1 - coords0, and against
      corr_conv_forward with cout = 2 on a contiguous copy of the hidden half plus the same two
      torch ops, "conv_kernel");
  (b) one whole BasicUpdateBlock call (lookup already through convc1, the GRU by its own switch)
      with the switch off, with every convolution on the kernel ("all"), and with the committed
      table update.USE_KERNEL ("fused"); then one refinement iteration's worth, the block plus the
      coordinate update: on torch ("iter_torch"), on the kernels without the tail ("iter_no_tail")
      and with the tail, a workspace and the update in the flow head's launch ("iter_tail").
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
from eraft_amd.precision import code  # noqa: E402

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


def bench_size(name, trials, dev, modes=()):
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

    def kernel_conv(convs, x, out, off, prec=0):
        packed, bias = update._conv_pack(convs)
        return _lib.conv_forward(x, None, packed, bias, sum(k.out_channels for k in convs), True, out=out,
                                 out_offset=off, precision=prec)

    def fused_conv(prec=0):
        xb[:, :128].copy_(inp)
        xb[:, 254:].copy_(flow)
        return kernel_conv((enc.conv,), cf, xb, 128, prec)

    # the same four launches in a reduced mode (into the same buffers: the variants run one at a time)
    in_mode = {"convc2": lambda p: kernel_conv((enc.convc2,), c1, cfb, 0, p),
               "convf2": lambda p: kernel_conv((enc.convf2,), f1, cfb, 192, p),
               "conv": fused_conv,
               "heads": lambda p: kernel_conv((m.flow_head.conv1, m.mask[0]), net, hdb, 0, p)}

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
        ok = ok.clone()  # the reduced modes below write into the same buffer
        gm, om = {}, {}
        for p in modes:  # each mode's output is copied before the next mode's warm-up overwrites the buffer
            gm[f"kernel_{p}"] = capture(lambda p=p: in_mode[lname](code(p)), stream)
            om[f"kernel_{p}"] = window(gm[f"kernel_{p}"][1]).clone()
        r = alternate({"torch": gt, "kernel": gk, **{n: cp[0] for n, cp in gm.items()}}, trials, steps)
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
        for n in gm:
            r[n]["rel_err_vs_fp64"] = norm_rel(om[n].cpu(), ref)
            r[f"{n}_over_kernel"] = round(r[n]["call_ms_median"] / r["kernel"]["call_ms_median"], 3)
        res["launches"][lname] = r
        del gt, gk, kt, kk, gm

    # (a) continued: the tail's two launches (corr_flow.hip), each against the torch ops it replaces
    hd = torch.relu(rnd(512))
    coords0 = torch.stack(torch.meshgrid(torch.arange(W, device=dev, dtype=torch.float32),
                                         torch.arange(H, device=dev, dtype=torch.float32), indexing="xy"))
    coords0 = coords0[None].repeat(B, 1, 1, 1).contiguous()
    coords1 = coords0 + flow
    head2 = m.flow_head.conv2
    f1b, hcopy = buf(128), hd[:, :256].contiguous()

    def torch_convf1():
        xb[:, 254:].copy_(flow)
        return F.relu(enc.convf1(flow)).contiguous()

    def kernel_convf1():
        packed, bias = update._flow_enc_pack(enc.convf1)
        return _lib.flow_enc_forward(flow, packed, bias, 128, True, out=f1b, flow_copy=xb, copy_offset=254)

    def torch_head2():
        d = head2(hd[:, :256])
        c = coords1 + d
        return d, c, c - coords0

    def kernel_head2():
        packed, bias = update._flow_head_pack(head2)
        return _lib.flow_head_forward(hd, 0, packed, bias, coords_in=coords1, coords0=coords0)

    def conv_head2():  # the cheapest alternative already in the library: corr_conv_forward with cout = 2
        packed, bias = update._conv_pack((head2,))
        d = _lib.conv_forward(hcopy, None, packed, bias, 2, False)
        c = coords1 + d
        return d, c, c - coords0

    with torch.no_grad():
        ref_f1 = F.relu(F.conv2d(flow.cpu().double(), enc.convf1.weight.cpu().double(), enc.convf1.bias.cpu().double(),
                                 padding=3))
        ref_d = F.conv2d(hd[:, :256].cpu().double(), head2.weight.cpu().double(), head2.bias.cpu().double(), padding=1)
    for lname, fns, ref in (("convf1", {"torch": torch_convf1, "kernel": kernel_convf1}, ref_f1),
                            ("flow_head2", {"torch": torch_head2, "kernel": kernel_head2, "conv_kernel": conv_head2},
                             ref_d)):
        caps = {n: capture(fn, stream) for n, fn in fns.items()}
        r = alternate({n: cp[0] for n, cp in caps.items()}, trials, steps)
        for n, cp in caps.items():
            o = cp[1][0] if isinstance(cp[1], tuple) else cp[1]
            r[n]["rel_err_vs_fp64"] = norm_rel(o.cpu(), ref)
        r["kernel_over_torch"] = round(r["kernel"]["call_ms_median"] / r["torch"]["call_ms_median"], 3)
        if "conv_kernel" in r:
            r["kernel_over_conv_kernel"] = round(r["kernel"]["call_ms_median"] / r["conv_kernel"]["call_ms_median"], 3)
        res["launches"][lname] = r
        del caps

    # (b) the whole block, then one iteration's worth of it: the block and the coordinate update, on
    # torch, on the kernels without the tail ("no_tail": convf1 and flow_head2 on torch, fresh
    # buffers, torch's coords1 + delta and coords1 - coords0) and on the tail with a workspace
    table = dict(update.USE_KERNEL)
    no_tail = dict(table, convf1=False, flow_head2=False)
    ws = update.UpdateWorkspace(inp)

    def plain_iter():
        out = m(net, inp, c1, flow, True)
        c = coords1 + out[2]
        return out + (c, c - coords0)

    def iter_tail():
        return m(net, inp, c1, flow, True, workspace=ws, coords1=coords1, coords0=coords0)

    graphs, outs, keep = {}, {}, []
    for vname, on, tab, fn, prec in [
            ("torch", False, table, None, "bf16x6"), ("all", True, dict.fromkeys(table, True), None, "bf16x6"),
            ("fused", True, table, None, "bf16x6"), ("iter_torch", False, table, plain_iter, "bf16x6"),
            ("iter_no_tail", True, no_tail, plain_iter, "bf16x6"), ("iter_tail", True, table, iter_tail, "bf16x6"),
            *((f"iter_tail_{p}", True, table, iter_tail, p) for p in modes)]:
        BasicUpdateBlock.fused = on
        m.precision = m.gru.precision = prec
        update.USE_KERNEL.update(tab)
        graphs[vname], out, k = capture(fn or (lambda: m(net, inp, c1, flow, True)), stream)
        outs[vname] = tuple(None if t is None else t.clone() for t in out)  # iter_tail's variants share the workspace
        keep.append(k)
    BasicUpdateBlock.fused = False
    m.precision = m.gru.precision = "bf16x6"
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
    r["iter_tail_over_iter_no_tail"] = round(r["iter_tail"]["call_ms_median"] / r["iter_no_tail"]["call_ms_median"], 3)
    r["iter_tail_over_iter_torch"] = round(r["iter_tail"]["call_ms_median"] / r["iter_torch"]["call_ms_median"], 3)
    for p in modes:
        r[f"iter_tail_{p}_over_iter_tail"] = round(r[f"iter_tail_{p}"]["call_ms_median"] / r["iter_tail"]["call_ms_median"], 3)
    res["block"] = r
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
            sys.exit("--precision names the reduced modes; bf16x6 is the variants 'kernel' and 'iter_tail'")
    if not torch.cuda.is_available():
        sys.exit("bench_update needs an MI355X (no CPU fallback)")
    if a.trials < 5:
        sys.exit("--trials must be >= 5 (the median of at least 5 windows is reported)")
    dev = torch.device("cuda", 0)
    doc = {"device": torch.cuda.get_device_name(0),
           "call": "one HIP graph per variant, variants alternated; launches: kernel vs the torch ops it replaces; "
                   "block: BasicUpdateBlock.forward on relu(convc1(lookup))",
           "sizes": {n: bench_size(n, a.trials, dev, modes) for n in a.sizes.split(",")}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
