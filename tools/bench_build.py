"""The correlation build in its three precision modes, side by side.

    python tools/bench_build.py [--sizes dsec,train,mvsec,hires1280,hires1920] [--json PATH]

Per size and mode (bf16x6, bf16x3, bf16): the pack alone, the MFMA kernel alone, the whole build
call, and the build plus 12 lookups (radius 4, 4 levels).  Every variant is one HIP graph of REP
back-to-back calls; the variants of a size run alternated in one process, and each figure is the
median of 5 windows.  Also each mode's norm-relative error against an fp64 product of the same
inputs (on up to 64 query rows).  Writes profiles/build_precision_bench.json by default.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "e-raft_amd"))
from eraft_amd import _lib  # noqa: E402
from eraft_amd.corr import _alloc_pyramid  # noqa: E402

SIZES = {"dsec": (1, 256, 60, 80), "train": (8, 256, 36, 48), "mvsec": (16, 256, 36, 44),
         "hires1280": (1, 256, 120, 160), "hires1920": (1, 256, 160, 240)}
MODES = {"bf16x6": 0, "bf16x3": 1, "bf16": 2}
LEVELS, RADIUS, LOOKUPS, WINDOWS = 4, 4, 12, 5


def graph_of(fn, rep, stream):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=stream):
        for _ in range(rep):
            fn()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="dsec,train,mvsec,hires1280,hires1920")
    ap.add_argument("--json", default=os.path.join(ROOT, "profiles", "build_precision_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.Stream()
    out = {"device": torch.cuda.get_device_name(0), "unit": "us", "windows": WINDOWS, "sizes": {}}
    for size in args.sizes.split(","):
        B, D, H, W = SIZES[size]
        big = B * (H * W) ** 2 > 1 << 28
        rep = 2 if big else 10
        gen = torch.Generator(device=dev).manual_seed(7)
        f1 = torch.randn((B, D, H, W), device=dev, generator=gen)
        f2 = torch.randn((B, D, H, W), device=dev, generator=gen)
        coords = (torch.rand((B, 2, H, W), device=dev, generator=gen) * torch.tensor([W - 1.0, H - 1.0], device=dev).view(1, 2, 1, 1))
        lv = _alloc_pyramid(B, H, W, LEVELS, f1)
        ws = _lib.build_workspace(f1, f2, _lib.BUILD_BF16X6)
        lk = torch.empty((B, LEVELS * (2 * RADIUS + 1) ** 2, H, W), device=dev)
        # accuracy first (the timed graphs overwrite the pyramid)
        rows = np.unique(np.linspace(0, H * W - 1, 64).astype(int))
        a = f1[0].reshape(D, H * W)[:, rows].double()
        ref = (a.T @ f2[0].reshape(D, H * W).double()) / np.sqrt(D)
        res = {"shape": [B, D, H, W], "rep": rep, "modes": {}}
        for mode, code in MODES.items():
            _lib.build(f1, f2, lv, _lib.BUILD_BF16X6, ws, precision=code)
            got = _lib.pyramid_export([lv[0][:H * W]], H, W)[0].reshape(H * W, H * W)[rows].double()
            res["modes"][mode] = {"norm_rel_err_vs_fp64": float((got - ref).norm() / ref.norm())}
        variants = {}
        with torch.cuda.stream(stream):
            for mode, code in MODES.items():
                fns = {
                    "pack": lambda c=code: _lib.build(f1, f2, lv, _lib.BUILD_BF16X6 | _lib.BUILD_ONLY_PACK, ws, precision=c),
                    "mfma": lambda c=code: _lib.build(f1, f2, lv, _lib.BUILD_BF16X6 | _lib.BUILD_ONLY_MFMA, ws, precision=c),
                    "build": lambda c=code: _lib.build(f1, f2, lv, _lib.BUILD_BF16X6, ws, precision=c),
                }

                def step(c=code):
                    _lib.build(f1, f2, lv, _lib.BUILD_BF16X6, ws, precision=c)
                    for _ in range(LOOKUPS):
                        _lib.lookup(lv, coords, RADIUS, lk)
                fns["build+12lookups"] = step
                for name, fn in fns.items():
                    fn()  # warm-up outside the capture (raises the kernels' LDS limits)
                    torch.cuda.synchronize()
                    variants[(mode, name)] = graph_of(fn, rep, stream)
        times = {k: [] for k in variants}
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for k, g in variants.items():  # one untimed replay each
            g.replay()
        torch.cuda.synchronize()
        for _ in range(WINDOWS):
            for k, g in variants.items():  # alternated: every variant once per window
                ev[0].record()
                g.replay()
                ev[1].record()
                ev[1].synchronize()
                times[k].append(ev[0].elapsed_time(ev[1]) * 1e3 / rep)
        for (mode, name), t in times.items():
            res["modes"][mode][name] = round(statistics.median(t), 2)
        base = res["modes"]["bf16x6"]
        for mode in ("bf16x3", "bf16"):
            res["modes"][mode]["ratio_to_bf16x6"] = {n: round(res["modes"][mode][n] / base[n], 3)
                                                     for n in ("pack", "mfma", "build", "build+12lookups")}
        out["sizes"][size] = res
        print(size, json.dumps(res["modes"]), flush=True)
        del variants, lv, ws, lk
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.json), exist_ok=True)
    with open(args.json, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
