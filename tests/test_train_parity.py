"""Whole-model training gradients against fp64 autograd.

Every backward kernel has its own parity test; this module checks their composition inside ERAFT
(the token / stash protocol of corr.py, _LookupConvFn's needs_input_grad branches, _ConvexUpsampleFn
between the mask head and the flow chain, the weight-pack cache across an in-place update, the
inference-only switches' fall-back under autograd, the padder, flow_init, B > 1 and train-mode
batch norm) against an independent reference.  tests/_train_ref.py runs one training step as three
legs (fp64 on the CPU: the truth; fp32 torch-only on the CPU and on the GPU: the floor; the model
as shipped on the GPU: the code under test) and returns, per leg, the predictions, every
parameter's gradient and the gradients at fnet's two outputs and cnet's output.

Bars, all norm_rel per tensor (tests/_util.py), e(leg) = error of a leg against the fp64 leg:
  truth      e(HIP) <= FLOOR_FACTOR * max(e(fp32 CPU), e(fp32 torch-only GPU)), computed from the
             same configuration's reference legs, for the low-resolution flow, every prediction,
             the three boundary gradients, every parameter's gradient and the batch norms' running
             statistics.  The HIP leg's error is another draw of fp32 rounding noise of the same
             kind as the floor's two draws and can land a small factor above them, hence 8; the
             composition faults this module exists for change a gradient by 1e-2 or more and the
             floors are at most 5e-4 at the boundary and 7e-3 at encoder weights.
  torch-only the HIP leg against the fp32 torch-only GPU leg (they share MIOpen and differ only in
             this project's kernels): GPU_TOL = 1e-3 per parameter and per boundary gradient, and
             the whole gradient's absolute error <= 1e-3 * the largest reference entry, the bar of
             test_ondemand_bwd.py::test_model_trains_with_alternate_corr for this comparison.
  zeros      the biases whose gradient is 0 in exact arithmetic (_train_ref.structural_zero) are
             held to the whole-gradient absolute bar only, as that test does and for its reason:
             what any run computes for them is rounding noise.  Nothing else is exempt.

ReLU kinks.  The fp64 leg always has a few update-block units whose pre-activation lies within
fp32 rounding noise of 0, and a flow-head unit that lands on the other side moves most gradients
by 2e-3 .. 6e-3: between two runs of one torch-only leg as much as between it and the HIP leg
(found here: with the plain references the unfused CorrBlock and the on-demand paths missed both
bars in about every second run, with the same figures each time, and passed in the others).  At
such a unit the truth has two values, so the reference legs take the HIP leg's side there
(_train_ref.reference_legs has the rule and its bound, FLOOR_FACTOR * the references' own
deviation); a sign that differs at any unit outside that bound fails the test.  The bars
themselves are unchanged.

Measured on an MI355X (each case 0.2 .. 2 s after the first, which also makes the references).
Worst e(HIP) / floor over predictions, boundary gradients, fnet, cnet and update-block gradients,
then the worst norm_rel against the torch-only GPU leg and the whole-gradient figure:
  default bf16x6 / f16x3 / fp32   0.86 1.01 1.13 1.09 1.34 / 0.94 1.03 1.07 1.13 1.30 /
                                  1.09 1.14 1.04 1.26 1.43; vs GPU <= 2.4e-5, whole <= 4.4e-6
  fuse_lookup_conv off            0.99 0.93 1.00 1.29 1.37; 1.7e-5, 3.3e-6
  FUSED_BWD=0, EXACT_FOLD=1       0.86 1.01 1.13 1.09 1.34; 2.2e-5, 4.4e-6 (both)
  alternate_corr (both)           0.93 0.99 1.21 1.54 1.70; 1.8e-5, 3.3e-6
  B=2, train, warm, padded        0.97 1.09 1.00 1.24 1.10; 2.7e-5, 2.3e-6; bn statistics 1.00
  inference switches on           0.86 1.01 1.13 1.09 1.34; 2.1e-5, 4.4e-6
  frozen encoders / update        0.88 - - - 1.35; 1.4e-5, 3.7e-6 / 0.86 1.01 1.13 1.09 -; 2.1e-5, 1.6e-6
  second step                     1.30 1.14 1.38 1.46 2.17; 1.2e-5, 3.3e-6
  two losses                      0.86 0.99 1.18 1.18 1.32; 2.2e-5, 4.7e-6
The floors: predictions <= 5e-6, boundary <= 6e-5, update block <= 2e-5 (2.4e-3 in the train
case), cnet <= 1e-5 (1.7e-2 in the train case), fnet weights <= 1.2e-2.  The zero biases' own
norm_rel against the torch-only leg is 1.6 .. 2.1: noise, as expected.
Planted faults against the default case, each tried once and not committed: stash_backward
dropping the last lookup (fnet.out1 / out2 4.5e-1, 5.2e-1, both bars), _LookupConvFn.backward
returning dW * (1 + 2^-6) (convc1.weight 1.56e-2, both bars, and the whole-gradient bar at
2.0e-3), _ConvexUpsampleFn.backward returning a zero dmask (boundary gradients 1.5e-2 ..
1.7e-2, both bars); and against the second step a weight-pack cache that ignores in-place
updates (2640 of convc2's ReLU inputs on the wrong side, the forward-sign assertion).
"""
import numpy as np
import pytest
import torch

import prng
from _train_ref import (BOUNDARY, Config, fp32_cpu_leg, fp64_leg, hip_leg, make_model, reference_legs,
                        structural_zero, torch_build, torch_lookup, zero_set)
from _util import REL_TOL, bit_equal, norm_rel

FLOOR_FACTOR = 8  # e(HIP) <= FLOOR_FACTOR * the fp32 floor (module docstring)
GPU_TOL = 1e-3    # HIP leg vs torch-only GPU leg (test_model_trains_with_alternate_corr's bar)

BASE = Config()  # 128x160, 5 bins: 16x20 maps, the smallest whose level 3 is 2x2; 3 iterations, B = 1
TRAIN = Config(H=120, W=150, B=2, iters=4, train=True, warm=True)  # the padder pads to 128x160
ALL_SWITCHES = ("BasicEncoder.fused", "SepConvGRU.fused", "BasicUpdateBlock.fused", "ERAFT.fuse_mask_upsample")


# ---------------------------------------------------------------------------------------------
# the harness itself, without a GPU
# ---------------------------------------------------------------------------------------------
def test_device_aware_chain_equals_the_oracle_bit_for_bit():
    from oracle.torch_ops import cpu_build, cpu_lookup
    B, D, H, W, L, r = 2, 32, 16, 20, 4, 4
    f1, f2 = (torch.from_numpy(prng.gauss(s, (B, D, H, W))) for s in (501, 502))
    ref, got = cpu_build(f1, f2, L), torch_build(f1, f2, L)
    assert len(got) == L and all(bit_equal(a.numpy(), b.numpy()) for a, b in zip(got, ref))
    for coords in (prng.lookup_coords(503, B, H, W, 3.0), prng.special_coords(B, H, W)):
        c = torch.from_numpy(coords)
        assert bit_equal(torch_lookup(got, c, r).numpy(), cpu_lookup(ref, c, r).numpy())


@pytest.mark.parametrize("cfg", [BASE, TRAIN], ids=["eval", "train"])
def test_fp64_leg_reaches_every_parameter_and_zeros_are_structural(cfg):
    """None of the fp64 leg's gradients is None, and those below 1e-12 of the model's largest
    gradient entry are exactly the biases of the convolutions that feed an instance norm or a
    train-mode batch norm: fnet's 15 in eval(), cnet's 15 as well in train()."""
    g = fp64_leg(cfg).grads
    assert len(g) == 124 and all(v is not None for v in g.values())
    scale = max(np.abs(v).max() for v in g.values())
    small = {n for n, v in g.items() if np.abs(v).max() < 1e-12 * scale}
    zeros = zero_set(cfg)
    assert len(zeros) == (30 if cfg.train else 15) and all(n.endswith(".bias") for n in zeros)
    assert small == zeros, (sorted(small - zeros), sorted(zeros - small))


def test_structural_zero_follows_freezing():
    assert structural_zero(make_model(Config(freeze="encoders"))) == set()
    assert structural_zero(make_model(Config(freeze="update"))) == zero_set(BASE)


def test_fp32_cpu_leg_is_within_rel_tol_of_fp64():
    e = norm_rel(fp32_cpu_leg(BASE).low, fp64_leg(BASE).low)
    print(f"low-resolution flow, fp32 vs fp64 on the CPU: {e:.2e}")
    assert e <= REL_TOL


def test_substitutions_are_undone():
    import eraft_amd.model as M
    from eraft_amd.corr import CorrBlock
    from eraft_amd.utils import coords_grid
    fp64_leg(BASE)
    assert M.CorrBlock is CorrBlock and M.coords_grid is coords_grid


# ---------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------
def _group(name, zeros):
    if name in zeros:
        return "zero biases"
    if name in BOUNDARY:
        return "boundary gradients"
    if name == "low" or name.startswith("pred"):
        return "predictions"
    if name.endswith(("running_mean", "running_var")):
        return "bn statistics"
    return name.split(".")[0] + " gradients"


def _check(what, cfg, hip):
    """Every bar of the module docstring for one HIP leg; prints one line per tensor group."""
    truth, cpu, gpu, note = reference_legs(cfg, hip, FLOOR_FACTOR)
    print(f"{what}: {note}")
    zeros = zero_set(cfg)

    def items(leg):
        out = {"low": leg.low, **{f"pred{i}": p for i, p in enumerate(leg.preds)}}
        for part in (leg.boundary, leg.grads, leg.stats):
            out.update(part)
        return out

    t, c, g, h = items(truth), items(cpu), items(gpu), items(hip)
    assert t.keys() == c.keys() == g.keys() == h.keys()
    absent = {n for n, v in t.items() if v is None}
    assert cfg.freeze or not absent
    # a frozen parameter ends with grad None (and so does a boundary with nothing trainable upstream)
    for leg in (c, g, h):
        assert {n for n, v in leg.items() if v is None} == absent, what
    grad_scale = max(np.abs(gpu.grads[n]).max() for n in gpu.grads if n not in absent)
    whole, fails, rows = 0.0, [], {}
    for n in t:
        if n in absent:
            continue
        assert np.isfinite(h[n]).all(), n
        if n in hip.grads:
            whole = max(whole, np.abs(h[n] - g[n]).max() / grad_scale)
        e, floor, d = norm_rel(h[n], t[n]), max(norm_rel(c[n], t[n]), norm_rel(g[n], t[n])), norm_rel(h[n], g[n])
        ratio = e / floor if floor > 0 else (0.0 if e == 0 else np.inf)
        row = rows.setdefault(_group(n, zeros), [0, 0.0, 0.0, 0.0, 0.0])
        row[0] += 1
        row[1:] = [max(a, b) for a, b in zip(row[1:], (e, floor, ratio, d))]
        if n in zeros:
            continue  # rounding noise around an exact 0: the whole-gradient bar below
        if not e <= FLOOR_FACTOR * floor:
            fails.append(f"{n}: error {e:.2e} vs fp64 > {FLOOR_FACTOR} x floor {floor:.2e}")
        if (n in hip.grads or n in BOUNDARY or n in hip.stats) and not d <= GPU_TOL:
            fails.append(f"{n}: {d:.2e} from the torch-only GPU leg > {GPU_TOL}")
    for grp, (k, e, floor, ratio, d) in rows.items():
        print(f"{what}: {grp} ({k}): worst error vs fp64 {e:.2e}, worst floor {floor:.2e}, "
              f"worst error / floor {ratio:.2f}, worst vs torch-only GPU {d:.2e}")
    print(f"{what}: whole gradient vs torch-only GPU {whole:.2e}")
    if not whole <= GPU_TOL:
        fails.append(f"whole gradient: {whole:.2e} from the torch-only GPU leg > {GPU_TOL}")
    for f in fails:
        print(f"{what}: MISSED {f}")
    assert not fails, f"{what}: {len(fails)} missed bars, the first: " + "; ".join(fails[:4])


@pytest.fixture
def hip_env(monkeypatch):
    """The shipped defaults, whatever the process's environment says: CorrBlock, lookup fused with
    convc1, fused backward, bf16x6 build, every inference switch off."""
    import eraft_amd.model as M
    for var in ("ERAFT_AMD_ONDEMAND", "ERAFT_AMD_BUILD", "ERAFT_AMD_FUSED_BWD", "ERAFT_AMD_EXACT_FOLD",
                "ERAFT_AMD_PRECISION"):
        monkeypatch.delenv(var, raising=False)
    monkeypatch.setattr(M.ERAFT, "fuse_lookup_conv", True)
    monkeypatch.setattr(M.ERAFT, "fuse_ondemand_conv", False)
    for sw in ALL_SWITCHES:
        cls, attr = sw.split(".")
        monkeypatch.setattr(getattr(M, cls), attr, False)
    return monkeypatch


def _all_switches_on(monkeypatch):
    import eraft_amd.model as M
    for sw in ALL_SWITCHES:
        cls, attr = sw.split(".")
        monkeypatch.setattr(getattr(M, cls), attr, True)


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["bf16x6", "f16x3", "fp32"])
def test_default_path(hip_env, build):
    hip_env.setenv("ERAFT_AMD_BUILD", build)
    _check(f"default, {build}", BASE, hip_leg(BASE))


@pytest.mark.gpu
def test_unfused_lookup_and_convc1(hip_env):
    from eraft_amd.model import ERAFT
    hip_env.setattr(ERAFT, "fuse_lookup_conv", False)
    _check("fuse_lookup_conv off", BASE, hip_leg(BASE))


@pytest.mark.gpu
@pytest.mark.parametrize("var,value", [("ERAFT_AMD_FUSED_BWD", "0"), ("ERAFT_AMD_EXACT_FOLD", "1")])
def test_backward_variants(hip_env, var, value):
    hip_env.setenv(var, value)
    _check(f"{var}={value}", BASE, hip_leg(BASE))


@pytest.mark.gpu
@pytest.mark.parametrize("fuse_conv", [False, True], ids=["plain", "fuse_ondemand_conv"])
def test_alternate_corr(hip_env, fuse_conv):
    from eraft_amd.model import ERAFT
    hip_env.setattr(ERAFT, "fuse_ondemand_conv", fuse_conv)
    _check(f"alternate_corr, fuse_ondemand_conv {fuse_conv}", BASE, hip_leg(BASE, alternate=True))


@pytest.mark.gpu
def test_batch_of_two_train_mode_warm_start_padded(hip_env):
    """B = 2, train() (batch statistics in cnet), flow_init, 4 iterations, 120x150 images that the
    padder pads to 128x160; the batch norms' running statistics after the step are compared too."""
    assert fp64_leg(TRAIN).stats and fp64_leg(TRAIN).preds[0].shape == (2, 2, 120, 150)
    _check("B=2, train, warm, padded", TRAIN, hip_leg(TRAIN))


@pytest.mark.gpu
def test_every_inference_switch_on_under_autograd(hip_env):
    """The inference kernels have no backward: with everything trainable each switch must fall
    back to the torch path, or gradients are lost silently."""
    _all_switches_on(hip_env)
    _check("inference switches on", BASE, hip_leg(BASE))


@pytest.mark.gpu
@pytest.mark.parametrize("freeze", ["encoders", "update"])
def test_partial_freezing_with_inference_switches_on(hip_env, freeze):
    """encoders: fnet and cnet frozen (they may take their HIP path), the update block trains and
    _LookupConvFn runs with a constant token (dlk None, dW and dbias wanted).  update: the update
    block frozen, the encoders train (dW and dbias None, dlk wanted).  Frozen parameters end with
    grad None (asserted in _check against the reference legs, frozen the same way)."""
    _all_switches_on(hip_env)
    cfg = Config(freeze=freeze)
    hip = hip_leg(cfg)
    frozen = ("fnet.", "cnet.") if freeze == "encoders" else ("update_block.",)
    for n, v in hip.grads.items():
        assert (v is None) == n.startswith(frozen), n
    assert all((hip.boundary[b] is None) == (freeze == "encoders") for b in BOUNDARY)
    _check(f"frozen {freeze}", cfg, hip)


@pytest.mark.gpu
def test_second_step_after_an_in_place_update(hip_env):
    """Step 1, then p.sub_(lr * g) under no_grad in every leg (g: the fp64 leg's gradient cast to
    fp32), then step 2, whose predictions and gradients are checked: a weight pack kept from
    step 1 (_cache) would be stale."""
    cfg = Config(steps=2)
    # the update is large enough to matter: it moves step 2's gradients far beyond any bar
    one, two = fp64_leg(BASE).grads, fp64_leg(cfg).grads
    n = "update_block.encoder.convc1.weight"
    assert norm_rel(two[n], one[n]) > 100 * GPU_TOL
    _check("second step", cfg, hip_leg(cfg))


@pytest.mark.gpu
def test_two_backwards_over_one_forward(hip_env):
    """The sequence loss's backward(retain_graph=True), then a linear loss's backward(): the stash
    is emptied and refilled, and the accumulated gradients match the reference's single backward
    of the sum."""
    cfg = Config(two_losses=True)
    _check("two losses", cfg, hip_leg(cfg))
