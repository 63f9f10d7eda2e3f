"""On-demand lookup vs CorrBlock's build + lookups: one step = prepare (or build) + 12 lookups,
captured as one HIP graph per variant and replayed; the variants of a size are alternated in ONE
process on the same inputs, so box-to-box spread drops out.
    python tools/bench_ondemand.py [--sizes dsec,hires1280,hires1920,uhd] [--trials 5] [--json PATH]
Per size and coordinate kind (coherent = grid + smooth flow, what the GRU produces; sigma4 = grid +
N(0, 4)): median ms per step of on-demand auto, on-demand forced-general and (where the pyramid
fits) CorrBlock, each variant's peak device allocation, and the on-demand output's norm-relative
difference from CorrBlock's.  Prints one JSON document; --json also writes it to a file.
    python tools/bench_ondemand.py --train [--sizes ...] [--json profiles/ondemand_train_bench.json]
--train: one step = prepare (or build) + 12 lookups + the backward to both feature maps
(corr_ondemand_backward / corr_backward) with coherent coordinates and gauss upstream gradients,
on-demand against CorrBlock (where the pyramid and its gradient fit) in the same way; also the
on-demand step's split: forward only, and the backward to fmap1 only / fmap2 only (the window
kernel alone / the window kernel without dF1 plus the dP gather).
    python tools/bench_ondemand.py --conv [--sizes ...] [--json profiles/ondemand_conv_bench.json]
--conv: one GRU iteration's lookup + convc1 + ReLU, 12 iterations (12 coordinate fields) per graph:
unfused (corr_ondemand_lookup + F.conv2d + ReLU) against fused (corr_ondemand_lookup_conv) and,
where the pyramid fits, CorrBlock's corr_lookup_conv for scale; us per iteration, each variant's
peak allocation during one eager iteration, and fused against unfused (norm-relative).
--variant-lib PATH times a second build of the library as "fused_variant" in the same process
(the other form of the product); --build-variant makes that build first: corr_ondemand_conv.hip
with -DCORR_OD_CONV_PRESPLIT=<the form that is not the default>, linked with the package's
objects into tools/_build/ (run it where the package was built)."""
import argparse
import ctypes
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd import _lib  # noqa: E402
from eraft_amd.corr import _alloc_grad_pyramid, _alloc_pyramid  # noqa: E402

# name: (H, W, CorrBlock fits)   B = 1, D = 256, 4 levels, r = 4, 12 lookups
SIZES = {"dsec": (60, 80, True), "hires1280": (120, 160, True), "hires1920": (160, 240, True),
         "uhd": (270, 480, False)}
B, D, L, R, ITERS = 1, 256, 4, 4, 12


def make_coords(kind, H, W, dev, gen):
    ys, xs = torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev), indexing="ij")
    base = torch.stack([xs, ys]).float()[None].repeat(B, 1, 1, 1)
    out = []
    for t in range(ITERS):
        if kind == "coherent":  # a smooth flow field growing over the iterations, plus sub-pixel noise
            fx = 3.0 * torch.sin(ys / H * math.pi) * (t + 1) / ITERS + 1.3
            fy = -2.0 * torch.cos(xs / W * math.pi) * (t + 1) / ITERS - 0.6
            flow = torch.stack([fx, fy])[None] + 0.05 * torch.randn(B, 2, H, W, device=dev, generator=gen)
        else:
            flow = 4.0 * torch.randn(B, 2, H, W, device=dev, generator=gen)
        out.append((base + flow).contiguous())
    return out


def norm_rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def bench_size(name, trials, dev):
    H, W, fits = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    f1 = torch.randn(B, D, H, W, device=dev, generator=gen)
    f2 = torch.randn(B, D, H, W, device=dev, generator=gen)
    K = (2 * R + 1) ** 2
    stream = torch.cuda.Stream()
    res = {"H": H, "W": W, "B": B, "D": D, "levels": L, "radius": R, "lookups": ITERS, "kinds": {}}
    for kind in ("coherent", "sigma4"):
        coords = make_coords(kind, H, W, dev, gen)
        variants, graphs, peaks, outs, keep = {}, {}, {}, {}, []

        def add(vname, alloc, step):
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            state = alloc()
            out = torch.empty(B, L * K, H, W, device=dev)
            with torch.cuda.stream(stream):
                step(state, out)
                torch.cuda.synchronize()
                outs[vname] = out.clone()
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    step(state, out)
            torch.cuda.synchronize()
            peaks[vname] = (torch.cuda.max_memory_allocated() - base - outs[vname].numel() * 4) / 1e6
            graphs[vname] = gr
            keep.append((state, out))

        def od_step(flags):
            def step(ws, out):
                _lib.ondemand_prepare(f1, f2, L, ws)
                for c in coords:
                    _lib.ondemand_lookup(ws, c, D, L, R, out, flags)
            return step

        od_alloc = lambda: _lib.ondemand_workspace(B, D, H, W, L, dev)  # noqa: E731
        add("ondemand_auto", od_alloc, od_step(0))
        add("ondemand_general", od_alloc, od_step(_lib.ONDEMAND_GENERAL))
        if fits:
            algo = _lib.default_algo()

            def cb_step(state, out):
                pyr, ws = state
                _lib.build(f1, f2, pyr, algo, ws)
                for c in coords:
                    _lib.lookup(pyr, c, R, out, H, W)

            add("corrblock", lambda: (_alloc_pyramid(B, H, W, L, f1), _lib.build_workspace(f1, f2, algo)), cb_step)
        steps = max(3, int(0.3 / (1e-3 * max(1.0, H * W / 4800.0))))  # ~0.3 s or more per window
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
        entry = {}
        for n, v in times.items():
            v = sorted(v)
            entry[n] = {"step_ms_median": round(v[len(v) // 2], 4), "step_ms_min": round(v[0], 4),
                        "step_ms_max": round(v[-1], 4), "peak_alloc_mb": round(peaks[n], 1)}
        entry["auto_vs_general_rel"] = norm_rel(outs["ondemand_auto"], outs["ondemand_general"])
        if fits:
            entry["ondemand_vs_corrblock_rel"] = norm_rel(outs["ondemand_auto"], outs["corrblock"])
        entry["steps_per_window"] = steps
        res["kinds"][kind] = entry
        del graphs, keep, outs
        torch.cuda.empty_cache()
    return res


def bench_train(name, trials, dev):
    """Training steps at one size: {variant: ms per step, peak allocation}, gradients' difference."""
    H, W, fits = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    f1 = torch.randn(B, D, H, W, device=dev, generator=gen)
    f2 = torch.randn(B, D, H, W, device=dev, generator=gen)
    K = (2 * R + 1) ** 2
    coords = make_coords("coherent", H, W, dev, gen)
    grads = [torch.randn(B, L * K, H, W, device=dev, generator=gen) for _ in range(ITERS)]
    out = torch.empty(B, L * K, H, W, device=dev)  # the lookups' output (its values are not kept)
    stream = torch.cuda.Stream()
    graphs, peaks, results, keep = {}, {}, {}, []

    def add(vname, alloc, step):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        state = alloc()
        with torch.cuda.stream(stream):
            results[vname] = step(state)
            torch.cuda.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=stream):
                keep.append(step(state))
        torch.cuda.synchronize()
        peaks[vname] = (torch.cuda.max_memory_allocated() - base) / 1e6
        graphs[vname] = gr
        keep.append(state)

    def od_alloc():
        ws = _lib.ondemand_workspace(B, D, H, W, L, dev)
        _lib.ondemand_prepare(f1, f2, L, ws)  # the backward-only variants read it
        return (ws, _lib.ondemand_bwd_workspace(B, D, H, W, L, R, dev))

    def od_step(fwd, want1, want2):
        def step(state):
            ws, bws = state
            if fwd:
                _lib.ondemand_prepare(f1, f2, L, ws)
                for c in coords:
                    _lib.ondemand_lookup(ws, c, D, L, R, out)
            if want1 or want2:
                return _lib.ondemand_backward(ws, coords, grads, D, L, R, bws, want1=want1, want2=want2)
        return step

    add("ondemand", od_alloc, od_step(True, True, True))
    add("ondemand_forward_only", od_alloc, od_step(True, False, False))
    add("ondemand_backward_dfmap1_only", od_alloc, od_step(False, True, False))
    add("ondemand_backward_dfmap2_only", od_alloc, od_step(False, False, True))
    if fits:
        algo = _lib.default_algo()

        def cb_step(state):
            pyr, ws, gl = state
            _lib.build(f1, f2, pyr, algo, ws)
            for c in coords:
                _lib.lookup(pyr, c, R, out, H, W)
            return _lib.backward(coords, grads, R, gl, f1, f2)

        add("corrblock", lambda: (_alloc_pyramid(B, H, W, L, f1), _lib.build_workspace(f1, f2, algo),
                                  _alloc_grad_pyramid(B, H, W, L, f1)), cb_step)
    steps = max(2, int(0.3 / (6e-3 * max(1.0, H * W / 4800.0))))
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
    res = {"H": H, "W": W, "B": B, "D": D, "levels": L, "radius": R, "lookups": ITERS, "coords": "coherent",
           "steps_per_window": steps}
    for n, v in times.items():
        v = sorted(v)
        res[n] = {"step_ms_median": round(v[len(v) // 2], 4), "step_ms_min": round(v[0], 4),
                  "step_ms_max": round(v[-1], 4), "peak_alloc_mb": round(peaks[n], 1)}
    if fits:
        res["dfmap1_vs_corrblock_rel"] = norm_rel(results["ondemand"][0], results["corrblock"][0])
        res["dfmap2_vs_corrblock_rel"] = norm_rel(results["ondemand"][1], results["corrblock"][1])
    del graphs, keep, results
    torch.cuda.empty_cache()
    return res


def build_variant():
    """The library with the other form of the fused product, for --variant-lib."""
    import re
    import subprocess
    from eraft_amd import build
    build.build_library()
    src = open(os.path.join(build.SRC, "corr_ondemand_conv.hip")).read()
    default = int(re.search(r"#define CORR_OD_CONV_PRESPLIT (\d)", src).group(1))
    out_dir = os.path.join(ROOT, "tools", "_build")
    os.makedirs(out_dir, exist_ok=True)
    obj = os.path.join(out_dir, "corr_ondemand_conv_variant.o")
    so = os.path.join(out_dir, "libcorr_mi355x_variant.so")
    flags = [f for f in build.FLAGS if f != "-shared"]
    subprocess.run([build.HIPCC, *flags, f"-DCORR_OD_CONV_PRESPLIT={1 - default}", "-c", "-o", obj,
                    os.path.join(build.SRC, "corr_ondemand_conv.hip")], check=True)
    objs = [obj if s == "corr_ondemand_conv.hip" else os.path.join(build.OBJ_DIR, os.path.splitext(s)[0] + ".o")
            for s in build.SOURCES]
    subprocess.run([build.HIPCC, "--offload-arch=gfx950", "-fPIC", "-shared", "-o", so, *objs], check=True)
    return so


def bench_conv(name, trials, dev, variant):
    """One iteration's lookup + convc1 + ReLU at one size: us per iteration and peak allocation."""
    import torch.nn.functional as F
    H, W, fits = SIZES[name]
    gen = torch.Generator(device=dev).manual_seed(1234)
    f1 = torch.randn(B, D, H, W, device=dev, generator=gen)
    f2 = torch.randn(B, D, H, W, device=dev, generator=gen)
    K = (2 * R + 1) ** 2
    w = 0.05 * torch.randn(256, L * K, 1, 1, device=dev, generator=gen)
    bias = 0.1 * torch.randn(256, device=dev, generator=gen)
    packed = _lib.lookup_conv_weights(w)
    ws = _lib.ondemand_workspace(B, D, H, W, L, dev)
    _lib.ondemand_prepare(f1, f2, L, ws)
    pyr = None
    if fits:
        pyr = _alloc_pyramid(B, H, W, L, f1)
        _lib.build(f1, f2, pyr, _lib.default_algo(), _lib.build_workspace(f1, f2, _lib.default_algo()))
    stream = torch.cuda.Stream()
    res = {"H": H, "W": W, "B": B, "D": D, "levels": L, "radius": R, "iterations_per_graph": ITERS, "kinds": {}}

    def unfused(c):
        look = torch.empty(B, L * K, H, W, device=dev)
        _lib.ondemand_lookup(ws, c, D, L, R, look)
        return F.relu(F.conv2d(look, w, bias))

    def fused(c):
        out = torch.empty(B, 256, H, W, device=dev)
        _lib.ondemand_lookup_conv(ws, c, D, L, R, packed, bias, out)
        return out

    def fused_variant(c):
        out = torch.empty(B, 256, H, W, device=dev)
        rc = variant.corr_ondemand_lookup_conv(ws.data_ptr(), c.data_ptr(), B, D, H, W, L, R, 0, packed.data_ptr(),
                                               bias.data_ptr(), 1, out.data_ptr(),
                                               torch.cuda.current_stream().cuda_stream)
        assert rc == 0, variant.corr_last_error()
        return out

    def corrblock(c):
        out = torch.empty(B, 256, H, W, device=dev)
        _lib.lookup_conv(pyr, c, R, packed, bias, out)
        return out

    fns = {"unfused": unfused, "fused": fused}
    if variant is not None:
        fns["fused_variant"] = fused_variant
    if fits:
        fns["corrblock_lookup_conv"] = corrblock
    for kind in ("coherent", "sigma4"):
        coords = make_coords(kind, H, W, dev, gen)
        graphs, peaks, outs, keep = {}, {}, {}, []
        for n, fn in fns.items():
            with torch.cuda.stream(stream):
                fn(coords[-1])  # MIOpen picks its kernel outside the measurement
                torch.cuda.synchronize()
                torch.cuda.reset_peak_memory_stats()
                base = torch.cuda.memory_allocated()
                outs[n] = fn(coords[-1])
                torch.cuda.synchronize()
                peaks[n] = (torch.cuda.max_memory_allocated() - base) / 1e6
                gr = torch.cuda.CUDAGraph()
                with torch.cuda.graph(gr, stream=stream):
                    keep.append([fn(c) for c in coords])
            torch.cuda.synchronize()
            graphs[n] = gr
        steps = max(3, int(0.3 / (0.5e-3 * max(1.0, H * W / 4800.0))))  # ~0.3 s or more per window
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
                    times[n].append((time.perf_counter() - t0) / (steps * ITERS) * 1e6)
        entry = {}
        for n, v in times.items():
            v = sorted(v)
            entry[n] = {"iteration_us_median": round(v[len(v) // 2], 2), "iteration_us_min": round(v[0], 2),
                        "iteration_us_max": round(v[-1], 2), "peak_alloc_mb": round(peaks[n], 2)}
        entry["fused_vs_unfused_rel"] = norm_rel(outs["fused"], outs["unfused"])
        if variant is not None:
            entry["fused_variant_vs_fused_rel"] = norm_rel(outs["fused_variant"], outs["fused"])
        if fits:
            entry["fused_vs_corrblock_rel"] = norm_rel(outs["fused"], outs["corrblock_lookup_conv"])
        entry["graph_replays_per_window"] = steps
        res["kinds"][kind] = entry
        del graphs, keep, outs
        torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dsec,hires1280,hires1920,uhd")
    ap.add_argument("--trials", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--train", action="store_true", help="training steps: forward + backward to both maps")
    ap.add_argument("--conv", action="store_true", help="one iteration's lookup + convc1 + ReLU, fused vs unfused")
    ap.add_argument("--variant-lib", default=None, help="--conv: a second build of the library, timed beside")
    ap.add_argument("--build-variant", action="store_true", help="build that library (no GPU needed) and exit")
    a = ap.parse_args()
    if a.build_variant:
        print(build_variant())
        return
    if not torch.cuda.is_available():
        sys.exit("bench_ondemand needs an MI355X (no CPU fallback)")
    dev = torch.device("cuda", 0)
    if a.conv:
        variant = _lib.load(a.variant_lib) if a.variant_lib else None
        doc = {"device": torch.cuda.get_device_name(0),
               "step": "one iteration's lookup + convc1 + ReLU; 12 iterations per HIP graph, us per iteration",
               "sizes": {n: bench_conv(n, a.trials, dev, variant) for n in a.sizes.split(",")}}
    elif a.train:
        doc = {"device": torch.cuda.get_device_name(0),
               "step": "prepare/build + 12 lookups + backward to both maps, one HIP graph",
               "sizes": {n: bench_train(n, a.trials, dev) for n in a.sizes.split(",")}}
    else:
        doc = {"device": torch.cuda.get_device_name(0), "step": "prepare/build + 12 lookups, one HIP graph",
               "sizes": {n: bench_size(n, a.trials, dev) for n in a.sizes.split(",")}}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
