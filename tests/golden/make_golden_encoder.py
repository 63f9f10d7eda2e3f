"""Generate tests/golden/encoder_reference.npz FROM THE REFERENCE's own BasicEncoder (model/extractor.py:119-189).
(Not named g_*.npz: test_oracle.py / test_gpu_parity.py treat every g_* file they do not exclude
by prefix as a CorrBlock build case.)

Run where the reference checkout is present (never on the GPU box):

    ERAFT_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_encoder.py

Both norms the model uses are covered, in eval(): norm_fn "instance" (fnet) and "batch" (cnet),
output_dim 256.  Weights come from encoder_param below, keyed by the module's own state-dict names
("layer2.0.conv1.weight", ...): prng.param_init, except that a batch norm's running variance is
0.5 + |gauss| so that the running statistics are far from the identity.  The input is
prng.gauss(seed, (B, C, H, W)).  The fixture holds the seeds, the shapes and the reference's fp32
CPU outputs only, never reference source.

The second case's maps are 17x25 -> 9x13 -> 5x7: odd sizes at both strided layers, partial tiles,
B > 1.  An instance norm over 35 pixels can be ill-conditioned (a channel whose variance is near
eps amplifies fp32 rounding), so before the fixture was committed the repository's restated module
was run on the CPU in fp32 and in fp64 on both cases and both norms: the norm-relative difference
was <= REL_TOL / 10 everywhere (largest 1.9e-6) with the seeds below; none had to be changed.
`--check` repeats that comparison (it needs no reference checkout).
"""
from __future__ import annotations

import os
import sys
import warnings
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prng  # noqa: E402

# (seed, B, C_in, H, W)
CASES = [(81, 1, 15, 32, 40), (83, 2, 3, 34, 50)]
NORMS = ("instance", "batch")
OUTPUT_DIM = 256


def encoder_param(name, shape):
    """The value of the encoder's state-dict entry `name` (None for num_batches_tracked)."""
    if name.endswith("running_var"):
        seed = zlib.crc32(name.encode()) & 0x3FFFFFFF
        return (0.5 + np.abs(prng.gauss(seed, shape).astype(np.float64))).astype(np.float32)
    return prng.param_init(name, shape)


def fill(module):
    with torch.no_grad():
        for name, t in module.state_dict().items():
            v = encoder_param(name, tuple(t.shape))
            if v is not None:
                t.copy_(torch.from_numpy(v))
    return module


def encoder_input(seed, B, C, H, W):
    return prng.gauss(seed, (B, C, H, W))


def check():
    """fp32 against fp64 of the repository's restated module, on the CPU."""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(HERE)), "e-raft_amd"))
    from eraft_amd.model import BasicEncoder
    worst = 0.0
    for norm in NORMS:
        for seed, B, C, H, W in CASES:
            m = fill(BasicEncoder(output_dim=OUTPUT_DIM, norm_fn=norm, n_first_channels=C).eval())
            x = torch.from_numpy(encoder_input(seed, B, C, H, W))
            with torch.no_grad():
                a, b = m(x).double(), m.double()(x.double())
            e = float((a - b).abs().max() / b.abs().max())
            worst = max(worst, e)
            print(f"{norm} seed={seed} B={B} C={C} {H}x{W}: fp32 vs fp64 {e:.2e}")
    return worst


def main():
    ref = os.environ.get("ERAFT_REFERENCE") or sys.exit("set ERAFT_REFERENCE to the reference E-RAFT checkout")
    sys.dont_write_bytecode = True
    sys.path.insert(0, ref)
    warnings.filterwarnings("ignore")
    from model.extractor import BasicEncoder  # (reference)
    torch.set_num_threads(8)
    out = {"cases": np.array(CASES, np.int64), "output_dim": np.array([OUTPUT_DIM], np.int64)}
    for norm in NORMS:
        for k, (seed, B, C, H, W) in enumerate(CASES):
            m = fill(BasicEncoder(output_dim=OUTPUT_DIM, norm_fn=norm, dropout=0.0, n_first_channels=C).eval())
            with torch.no_grad():
                out[f"{norm}{k}"] = m(torch.from_numpy(encoder_input(seed, B, C, H, W))).numpy()
    path = os.path.join(HERE, "encoder_reference.npz")
    np.savez_compressed(path, **out)
    print(f"encoder_reference:{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    if "--check" in sys.argv[1:]:
        sys.exit(0 if check() <= 1e-5 else 1)
    main()
