"""bench.py's measurement arithmetic on CPU: the algorithmic counts SURVEY §8(d) quotes per
config, the roofline / ceiling formulas, the committed PMC traffic it reads, and the workload
table a `--full` run walks (no GPU: nothing here launches a kernel).  The two tests marked
`gpu` run a small workload through run_corr: what a plain run reports and dumps, and what
`--full` adds."""
import argparse
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_algorithmic_counts_match_survey():
    # DSEC build 11.80 GFLOP / 132.1 MB, lookup 13.94 MB per call;
    # MVSEC 36x44 B16 20.55 GFLOP, lookup 73.6 MB; train B8 36x48 12.23 GFLOP, lookup 40.1 MB
    B, D, H, W, L, r, _ = bench.WORKLOADS["dsec"]
    assert bench.build_flops(B, D, H, W) / 1e9 == pytest.approx(11.80, abs=0.005)
    assert bench.build_bytes(B, D, H, W, L) / 1e6 == pytest.approx(132.1, abs=0.05)
    assert bench.lookup_bytes(B, H, W, L, r) / 1e6 == pytest.approx(13.94, abs=0.005)
    B, D, H, W, L, r, _ = bench.WORKLOADS["mvsec"]
    assert bench.build_flops(B, D, H, W) / 1e9 == pytest.approx(20.55, abs=0.005)
    assert bench.lookup_bytes(B, H, W, L, r) / 1e6 == pytest.approx(73.6, abs=0.05)
    B, D, H, W, L, r, _ = bench.WORKLOADS["train"]
    assert bench.build_flops(B, D, H, W) / 1e9 == pytest.approx(12.23, abs=0.005)
    assert bench.lookup_bytes(B, H, W, L, r) / 1e6 == pytest.approx(40.1, abs=0.05)
    # per query: L (2r+2)^2 + L (2r+1)^2 floats + the 8 B of coords
    assert bench.lookup_bytes(1, 1, 1, 4, 4) == 4 * 100 * 4 + 4 * 81 * 4 + 8


def test_workload_table_covers_the_baseline_configs():
    for wl in bench.EXTRA_WORKLOADS:
        assert wl in bench.WORKLOADS or wl == "e2e", wl
    # configs 2-5 beside the DSEC value: train (4), mvsec (3), both config-5 sizes, e2e (2)
    assert set(bench.EXTRA_WORKLOADS) == {"train", "mvsec", "hires1280", "hires1920", "e2e"}
    assert bench.WORKLOADS["hires1920"][2:4] == (160, 240)  # 1920x1280 / 8
    assert bench.WORKLOADS["hires1280"][2:4] == (120, 160)


def test_build_roofline_prices_the_executed_pipe():
    B, D, H, W, L, _, _ = bench.WORKLOADS["dsec"]
    fl, bb = bench.build_flops(B, D, H, W), bench.build_bytes(B, D, H, W, L)
    t_ms = 0.075
    rf = bench.build_roofline(2, fl, bb, t_ms, None)  # bf16x6: 6 executed products per fp32 one
    assert rf["bound"] == "mfma" and rf["peak"] == bench.PEAK_F16_MFMA_TFLOPS
    assert rf["achieved"] == pytest.approx(6 * fl / (t_ms * 1e-3) / 1e12, rel=1e-3)
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], abs=1e-4)
    assert rf["fp32_equivalent_tflops"] == pytest.approx(fl / (t_ms * 1e-3) / 1e12, rel=1e-3)
    r0 = bench.build_roofline(0, fl, bb, t_ms, None)  # the fp32-operand build: fp32 MFMA peak
    assert r0["peak"] == bench.PEAK_FP32_MFMA_TFLOPS
    assert r0["achieved"] == pytest.approx(fl / (t_ms * 1e-3) / 1e12, rel=1e-3)


def test_lookup_ceiling_binds_the_lower_bound():
    lb = bench.lookup_bytes(1, 60, 80, 4, 4)
    c = bench.lookup_ceiling("dsec", lb, 0.0055, 2 * lb)
    floor = c["latency_floor"]["frac"]
    gran = c["line_granularity"]["frac"]
    assert floor == pytest.approx(lb / (bench.LOOKUP_NOLOAD_NOSTORE_US["dsec"] * 1e-6) / 1e9 / bench.PEAK_HBM_GBS,
                                  abs=1e-4)
    assert gran == pytest.approx(0.5 * bench.ACHIEVABLE_HBM_GBS / bench.PEAK_HBM_GBS, abs=1e-4)
    assert c["binding"] == ("latency_floor" if floor < gran else "line_granularity")
    frac = lb / 0.0055e-3 / 1e9 / bench.PEAK_HBM_GBS
    assert c["frac_of_ceiling"] == pytest.approx(frac / min(floor, gran), abs=1e-3)
    # no floor measured and no PMC pass: no ceiling claimed
    assert bench.lookup_ceiling("mvsec_crop", lb, 0.03, None) == {}
    # every workload the default line measures has a measured floor
    assert all(w in bench.LOOKUP_NOLOAD_NOSTORE_US for w in bench.EXTRA_WORKLOADS if w != "e2e")


def _args(**kw):
    base = dict(gpus=1, steps=3, warmup=1, workload="dsec", eager=False, full=False, dump_outputs=None,
                cpu_seconds=0.05, no_cpu_baseline=False, sharded=False, chunks=4, prefetch=False,
                no_sharded_leg=False, no_workloads=False)
    base.update(kw)
    return argparse.Namespace(**base)


def test_plain_run_is_the_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "d"
    assert vars(_args()).keys() == vars(a).keys()  # the namespace the GPU tests below hand to run_corr


def test_dump_outputs_samples_large_arrays_reproducibly(tmp_path):
    import torch

    big = torch.arange(3 * bench.DUMP_MAX_ELEMS, dtype=torch.float32).reshape(3, -1)  # exact in fp32
    small = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small, "other": big})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(a, b)                          # the same elements in every run
    assert np.all(np.diff(a) >= 0) and a.max() > 2 * bench.DUMP_MAX_ELEMS  # sorted indices over the whole array
    assert not np.array_equal(a, np.load(tmp_path / "a" / "other.npy"))    # seeded per name
    s = np.load(tmp_path / "a" / "small.npy")
    assert s.dtype == np.float64 and np.array_equal(s, small.numpy())      # small arrays whole
    assert sorted(p.name for p in (tmp_path / "a").iterdir()) == ["big.npy", "other.npy", "small.npy"]
    # the largest dump (train: 12 lookups + 4 levels + 2 gradients) stays under 64 MB
    assert 18 * (bench.DUMP_MAX_ELEMS * 4 + 128) < 64e6


TINY = (2, 32, 17, 23, 3, 3, 4)  # B, D, H, W, levels, radius, lookups: odd sizes, more than one tile
FULL_ONLY = {"roofline", "roofline_lookup", "kernel_timing", "hbm_gbs_algorithmic", "alt_values", "build_fp32",
             "build_f16x3", "cpu_baseline", "cpu_baseline_1thread", "speedup_vs_cpu", "workloads"}


@pytest.mark.gpu
def test_plain_run_dumps_what_the_timed_step_computed(tmp_path, monkeypatch):
    import torch
    from eraft_amd import CorrBlock

    monkeypatch.setitem(bench.WORKLOADS, "tiny", TINY)
    dev = torch.device("cuda", 0)
    res = bench.run_corr(_args(dump_outputs=str(tmp_path)), "tiny", False, 1, 0, dev)
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["config"]["launch"] == "hipgraph"
    assert res["value"] == pytest.approx(TINY[0] / (res["ms_per_step"] * 1e-3), rel=1e-2)
    assert (res["metric"], res["unit"], res["higher_is_better"], res["dtype"]) == \
        (bench.METRIC, "frame-pairs/s", True, "f32")
    assert not FULL_ONLY & res.keys()
    # the same inputs, drawn again as run_corr draws them, through the drop-in API
    B, D, H, W, L, r, iters = TINY
    g = torch.Generator(device=dev).manual_seed(1234)
    f1 = torch.randn(B, D, H, W, device=dev, generator=g)
    f2 = torch.randn(B, D, H, W, device=dev, generator=g)
    base = torch.stack(torch.meshgrid(torch.arange(H, device=dev), torch.arange(W, device=dev),
                                      indexing="ij")[::-1]).float()[None].repeat(B, 1, 1, 1)
    cb = CorrBlock(f1, f2, num_levels=L, radius=r)
    for t in range(iters):
        c = (base + 0.5 * t * torch.randn(B, 2, H, W, device=dev, generator=g)).contiguous()
        got = np.load(tmp_path / f"lookup_{t:02d}.npy")
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), cb(c).cpu().numpy().view(np.uint32)), t
    for l, p in enumerate(cb.corr_pyramid):
        assert np.array_equal(np.load(tmp_path / f"pyramid_{l}.npy").view(np.uint32), p.cpu().numpy().view(np.uint32))
    assert len(list(tmp_path.iterdir())) == iters + L


@pytest.mark.gpu
def test_full_run_adds_to_the_plain_line(monkeypatch):
    import torch

    monkeypatch.setitem(bench.WORKLOADS, "tiny", TINY)
    res = bench.run_corr(_args(full=True), "tiny", False, 1, 0, torch.device("cuda", 0))
    assert res["steps"] == 3 and res["ms_per_step"] > 0
    assert FULL_ONLY - {"workloads"} <= res.keys()  # `workloads` is main()'s, on the DSEC line
    assert res["roofline"]["avg_us"] > 0 and res["roofline_lookup"]["avg_us"] > 0
    assert res["cpu_baseline"]["value"] > 0


def test_traffic_reads_the_newest_committed_pmc_pass():
    t = bench.traffic("dsec", "lookup_kernel")
    assert t is not None and t > bench.lookup_bytes(1, 60, 80, 4, 4)  # line granularity: > algorithmic
    bt = bench.build_traffic("dsec", 2)
    assert bt is not None and bt >= bench.build_bytes(1, 256, 60, 80, 4)  # pyramid + packed operands
    assert bench.traffic("no_such_workload", "lookup_kernel") is None
