"""The encoders' pieces on the project's kernels vs the torch / MIOpen / rocBLAS ops they replace.
Every variant is captured as one HIP graph and replayed; the variants of a measurement are
alternated in ONE process on the same inputs, so box-to-box spread drops out.
    python tools/bench_encoder.py [--sizes dsec,b8,hires1920] [--kinds layer1.first,stem,...] [--trials 5]
                                  [--precision bf16x3,bf16] [--json profiles/encoder_bench.json]
Per size (the encoder's input; fnet sees both voxel grids as one batch, cnet one) and per encoder
(fnet: instance norm, cnet: eval-mode batch norm):
  (a) each kind of convolution against the torch ops it replaces.  "first": a block's conv1 (at
      its stride), torch conv + norm + ReLU against the kernel with statistics + finalize (instance)
      or the kernel alone (batch; the norm and the ReLU are its consumer's).  "second": a block's
      conv2, torch conv + norm + ReLU + add + ReLU against the kernel with norm on load (and
      statistics + finalize) + join.  "stem": torch conv 7x7 + norm + ReLU, then corr_enc_join of a
      fixed y with that map as its skip, against the stem kernel (+ finalize) and
      corr_enc_join_affine of the same y with the raw map; "layerN.proj": torch downsample(x) (1x1
      conv + norm) and corr_enc_join against the pointwise kernel (+ finalize) and
      corr_enc_join_affine; "head": torch conv2 against the pointwise kernel.  Both sides of a stem
      or projection row carry one join, so their difference holds the extra skip arithmetic;
  (b) one whole encoder call with the switch off, with the stem, the projections and the head on
      torch and the 3x3 convolutions on the committed table ("stages": the switch before these
      pieces had kernels), with every piece on the kernel ("all"), and with the committed table
      encoder.USE_KERNEL ("fused").
Median / min / max ms per call over the trial windows; for (a) each path's norm-relative error
against the same formula in fp64 on the GPU, for (b) the kernel path's norm-relative difference
from the torch path (the parity against the reference is tests/test_encoder.py's).
--precision adds, to every row of (a), the kernel side in each named mode ("kernel_<mode>", with its
own error against fp64 and its time over the bf16x6 kernel's) and, to (b), the committed table in
that mode ("fused_<mode>", module.precision), all in the same alternation.  Prints one JSON
document; --json also writes it to a file."""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd import _lib, encoder, precision  # noqa: E402
from eraft_amd.model import BasicEncoder  # noqa: E402

# name: (pairs per batch, C_in, H, W) of the model input
SIZES = {"dsec": (1, 15, 480, 640), "b8": (8, 15, 288, 384), "hires1920": (1, 15, 1280, 1920)}
# key of encoder.USE_KERNEL: (layer, block, first conv?)
KINDS = {"layer1.first": ("layer1", 0, True), "layer1.second": ("layer1", 0, False),
         "layer2.s2": ("layer2", 0, True), "layer2.first": ("layer2", 1, True), "layer2.second": ("layer2", 0, False),
         "layer3.s2": ("layer3", 0, True), "layer3.first": ("layer3", 1, True), "layer3.second": ("layer3", 0, False)}
FRONT = ("stem", "layer2.proj", "layer3.proj", "head")


def norm_rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def norm64(norm, y):
    """norm(y) in fp64 on the GPU (instance norm without affine, or eval-mode batch norm)."""
    if isinstance(norm, torch.nn.InstanceNorm2d):
        return F.instance_norm(y, eps=norm.eps)
    return F.batch_norm(y, norm.running_mean.double(), norm.running_var.double(), norm.weight.double(),
                        norm.bias.double(), False, 0.0, norm.eps)


def conv64(conv, x):
    return F.conv2d(x.double(), conv.weight.double(), conv.bias.double(), stride=conv.stride, padding=1)


def capture(fn, stream):
    """fn warmed up twice (MIOpen's solver search, the weight packs), then captured."""
    torch.cuda.synchronize()  # the inputs were made on the default stream
    with torch.no_grad(), torch.cuda.stream(stream):
        for _ in range(2):
            out = fn()
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=stream):
            keep = fn()
    torch.cuda.synchronize()
    return gr, out, keep


def alternate(graphs, trials, budget=0.15):
    """Windows of about `budget` seconds each (sized by the first variant's replay time)."""
    g0 = next(iter(graphs.values()))
    g0.replay()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    g0.replay()
    torch.cuda.synchronize()
    steps = max(3, min(200, int(budget / max(time.perf_counter() - t0, 1e-5))))
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
    res = {"steps_per_window": steps}
    for n, v in times.items():
        v = sorted(v)
        res[n] = {"call_ms_median": round(v[len(v) // 2], 4), "call_ms_min": round(v[0], 4),
                  "call_ms_max": round(v[-1], 4)}
    return res


def front_fns(m, kind, x, maps, instance):
    """(torch_fn, kernel_fn, check, ref, src) of one of the FRONT rows; kernel_fn(prec) runs in the
    CORR_PREC_* mode prec."""
    if kind == "head":
        with torch.no_grad():
            src = m.layer3(maps["layer3"])
            ref = F.conv2d(src.double(), m.conv2.weight.double(), m.conv2.bias.double())
        return (lambda: m.conv2(src)), (lambda prec=0: encoder._pw(m.conv2, src, prec=prec)), (lambda o: o), ref, src
    if kind == "stem":
        src, conv, norm, relu = x, m.conv1, m.norm1, True
    else:
        block = getattr(m, kind.split(".")[0])[0]
        src, conv, norm, relu = maps[kind.split(".")[0]], block.downsample[0], block.downsample[1], False
    with torch.no_grad():
        raw = conv(src)
        y = torch.randn_like(raw)
        sc = 1.0 + 0.1 * torch.randn(raw.shape[:2] if instance else raw.shape[1:2], device=x.device)
        sh = 0.1 * torch.randn_like(sc)
        skip = norm64(norm, F.conv2d(src.double(), conv.weight.double(), conv.bias.double(), stride=conv.stride,
                                     padding=conv.padding))
        view = (raw.shape[0], raw.shape[1], 1, 1) if instance else (1, raw.shape[1], 1, 1)
        ref = F.relu((F.relu(skip) if relu else skip) + F.relu(y.double() * sc.double().view(view) + sh.double().view(view)))

    def torch_fn():
        s = norm(conv(src))
        return _lib.enc_join(y, sc, sh, F.relu(s) if relu else s)

    def kernel_fn(prec=0):
        if kind == "stem":
            packed, bias = encoder._front_pack(conv, _lib.enc_stem_pack_weights)
            p = _lib.enc_stem_forward(src, packed, bias, conv.out_channels, stats=instance, precision=prec)
        else:
            p = encoder._pw(conv, src, stats=instance, prec=prec)
        p, st = p if instance else (p, None)
        return _lib.enc_join_affine(y, sc, sh, p, *encoder._norm_of(p, st, norm, instance), skip_relu=relu)
    return torch_fn, kernel_fn, (lambda o: o), ref, src


def bench_encoder(m, x, which, trials, stream, kinds, modes=()):
    """(a) and (b) for one encoder `m` on the input x; modes: the reduced modes measured beside."""
    instance = m.norm_fn == "instance"
    res = {"norm": m.norm_fn, "B": x.shape[0], "convs": {}}
    with torch.no_grad():
        maps = {"layer1": F.relu(m.norm1(m.conv1(x)))}
        maps["layer2"] = m.layer1(maps["layer1"])
        maps["layer3"] = m.layer2(maps["layer2"])
    for kind in kinds:
        layer, blk, first = KINDS.get(kind, (None, 0, False))
        block = getattr(m, layer)[blk] if layer else None
        if kind in FRONT:
            torch_fn, kernel_fn, check, ref, src = front_fns(m, kind, x, maps, instance)
            conv = {"stem": m.conv1, "head": m.conv2}.get(kind) or getattr(m, kind.split(".")[0])[0].downsample[0]
        elif first:
            with torch.no_grad():
                src = maps[layer] if blk == 0 else getattr(m, layer)[0](maps[layer])
                conv, norm = block.conv1, block.norm1
                ref = F.relu(norm64(norm, conv64(conv, src)))
            torch_fn = lambda: F.relu(norm(conv(src)))

            def kernel_fn(prec=0):
                y, sc, sh = encoder._conv_norm("on", conv, norm, src, None, instance, prec)
                return y, sc, sh
            check = lambda o: encoder._affine(*o)
        else:
            with torch.no_grad():
                src = block.conv1(maps[layer])  # conv2's input before its norm
            sc0 = 1.0 + 0.1 * torch.randn(src.shape[:2] if instance else src.shape[1:2], device=x.device)
            sh0 = 0.1 * torch.randn_like(sc0)
            skip = torch.randn_like(src)
            conv, norm = block.conv2, block.norm2
            view = (src.shape[0], src.shape[1], 1, 1) if instance else (1, src.shape[1], 1, 1)
            act = F.relu(src * sc0.view(view) + sh0.view(view))  # what torch's conv2 reads (already stored there)
            with torch.no_grad():
                ref = F.relu(skip.double() + F.relu(norm64(norm, conv64(conv, act))))
            torch_fn = lambda: F.relu(skip + F.relu(norm(conv(act))))

            def kernel_fn(prec=0):
                y, sc, sh = encoder._conv_norm("on", conv, norm, src, (sc0, sh0), instance, prec)
                return _lib.enc_join(y, sc, sh, skip, out=y)
            check = lambda o: o
        gt, ot, kt = capture(torch_fn, stream)
        gk, ok, kk = capture(kernel_fn, stream)
        reduced = {mode: capture(lambda mode=mode: kernel_fn(precision.code(mode)), stream) for mode in modes}
        r = alternate(dict({"torch": gt, "kernel": gk}, **{f"kernel_{mode}": c[0] for mode, c in reduced.items()}), trials)
        r["shape_in"] = list(src.shape)
        r["cout"], r["stride"] = conv.out_channels, conv.stride[0]
        with torch.no_grad():
            r["kernel"]["rel_err_vs_fp64"] = norm_rel(check(ok), ref)
            r["torch"]["rel_err_vs_fp64"] = norm_rel(ot, ref)
            for mode, c in reduced.items():
                r[f"kernel_{mode}"]["rel_err_vs_fp64"] = norm_rel(check(c[1]), ref)
                r[f"{mode}_over_bf16x6"] = round(r[f"kernel_{mode}"]["call_ms_median"] / r["kernel"]["call_ms_median"], 3)
        r["kernel_over_torch"] = round(r["kernel"]["call_ms_median"] / r["torch"]["call_ms_median"], 3)
        res["convs"][kind] = r
        del gt, gk, kt, kk, ot, ok, ref, reduced
        torch.cuda.empty_cache()

    table = {k: v for k, v in encoder.USE_KERNEL.items() if k != "on"}
    graphs, outs, keep = {}, {}, []
    stages = dict(table, **dict.fromkeys(FRONT, False))
    variants = [("torch", False, table, "bf16x6"), ("stages", True, stages, "bf16x6"),
                ("all", True, dict.fromkeys(table, True), "bf16x6"), ("fused", True, table, "bf16x6")]
    variants += [(f"fused_{mode}", True, table, mode) for mode in modes]
    for vname, on, tab, mode in variants:
        BasicEncoder.fused = on
        encoder.USE_KERNEL.update(tab)
        m.precision = mode
        graphs[vname], outs[vname], k = capture(lambda: m(x), stream)
        keep.append(k)
    BasicEncoder.fused = False
    encoder.USE_KERNEL.update(table)
    m.precision = "bf16x6"
    r = alternate(graphs, trials)
    for vname, _, _, _ in variants[1:]:
        r[vname]["vs_torch_rel"] = norm_rel(outs[vname], outs["torch"])
        r[f"{vname}_over_torch"] = round(r[vname]["call_ms_median"] / r["torch"]["call_ms_median"], 3)
    for mode in modes:
        r[f"{mode}_over_bf16x6"] = round(r[f"fused_{mode}"]["call_ms_median"] / r["fused"]["call_ms_median"], 3)
    r["use_kernel"] = table
    res["whole"] = r
    del graphs, keep, outs
    torch.cuda.empty_cache()
    return res


def bench_size(name, trials, dev, kinds, modes=()):
    pairs, C, H, W = SIZES[name]
    torch.manual_seed(1234)
    stream = torch.cuda.Stream()
    res = {"input": [pairs, C, H, W]}
    for which, norm, B in (("fnet", "instance", 2 * pairs), ("cnet", "batch", pairs)):
        m = BasicEncoder(output_dim=256, norm_fn=norm, n_first_channels=C).to(dev).eval()
        if norm == "batch":
            with torch.no_grad():
                for mod in m.modules():
                    if isinstance(mod, torch.nn.BatchNorm2d):
                        mod.running_mean.normal_(0.0, 0.1)
                        mod.running_var.uniform_(0.5, 1.5)
        x = torch.randn(B, C, H, W, device=dev) * (torch.rand(B, C, H, W, device=dev) < 0.15)
        res[which] = bench_encoder(m, x, which, trials, stream, kinds, modes)
        del m, x
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dsec,b8,hires1920")
    ap.add_argument("--kinds", default=",".join(list(KINDS) + list(FRONT)), help="the rows of (a) to measure")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--precision", default="", help="reduced modes to measure beside bf16x6, e.g. bf16x3,bf16")
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_encoder needs an MI355X (no CPU fallback)")
    if a.trials < 5:
        sys.exit("--trials must be >= 5 (the median of at least 5 windows is reported)")
    kinds = [k for k in a.kinds.split(",") if k]
    if any(k not in KINDS and k not in FRONT for k in kinds):
        sys.exit(f"--kinds must be among {list(KINDS) + list(FRONT)}")
    modes = [p for p in a.precision.split(",") if p]
    if any(p not in ("bf16x3", "bf16") for p in modes):
        sys.exit("--precision must be among bf16x3, bf16")
    dev = torch.device("cuda", 0)
    encoder.USE_KERNEL["on"] = True  # the key the single-convolution measurements run under
    doc = {"device": torch.cuda.get_device_name(0),
           "call": "one HIP graph per variant, variants alternated; convs: kernel launches vs the torch ops they "
                   "replace; whole: BasicEncoder.forward",
           "precision": modes,
           "sizes": {n: bench_size(n, a.trials, dev, kinds, modes) for n in a.sizes.split(",")}}
    del encoder.USE_KERNEL["on"]
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
