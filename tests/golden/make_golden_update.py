"""Generate tests/golden/update_reference.npz FROM THE REFERENCE's own BasicUpdateBlock (model/update.py:85-107).
(Not named g_*.npz: test_oracle.py / test_gpu_parity.py treat every g_* file they do not exclude
by prefix as a CorrBlock build case.)

Run where the reference checkout is present (never on the GPU box):

    ERAFT_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_update.py

Weights come from prng.param_init keyed by the module's own state-dict names
("encoder.convc2.weight", ...); net = tanh(prng.gauss(seed)), inp = relu(prng.gauss(seed + 1)),
corr = prng.gauss(seed + 2) [B, 324, H, W] (the raw lookup: convc1 runs inside the block) and
flow = prng.gauss(seed + 3).  The fixture holds the seeds, the shapes and the reference's fp32 CPU
outputs (net, mask, delta_flow) only, never reference source.
"""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import prng  # noqa: E402

REF = os.environ.get("ERAFT_REFERENCE") or sys.exit("set ERAFT_REFERENCE to the reference E-RAFT checkout")
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
from model.update import BasicUpdateBlock  # noqa: E402  (reference)

torch.set_num_threads(8)

# (seed, B, H, W)
CASES = [(51, 1, 5, 6), (53, 2, 9, 11)]
HID, LEVELS, RADIUS = 128, 4, 4


def update_inputs(seed, B, H, W):
    net = np.tanh(prng.gauss(seed, (B, HID, H, W)).astype(np.float64)).astype(np.float32)
    inp = np.maximum(prng.gauss(seed + 1, (B, HID, H, W)), 0.0).astype(np.float32)
    corr = prng.gauss(seed + 2, (B, LEVELS * (2 * RADIUS + 1) ** 2, H, W))
    return net, inp, corr, prng.gauss(seed + 3, (B, 2, H, W))


def main():
    out = {"cases": np.array(CASES, np.int64)}
    args = types.SimpleNamespace(corr_levels=LEVELS, corr_radius=RADIUS)
    for k, (seed, B, H, W) in enumerate(CASES):
        m = BasicUpdateBlock(args, hidden_dim=HID).eval()
        with torch.no_grad():
            for name, t in m.state_dict().items():
                t.copy_(torch.from_numpy(prng.param_init(name, tuple(t.shape))))
            net, mask, delta = m(*(torch.from_numpy(a) for a in update_inputs(seed, B, H, W)))
        out[f"net{k}"], out[f"mask{k}"], out[f"delta_flow{k}"] = net.numpy(), mask.numpy(), delta.numpy()
    path = os.path.join(HERE, "update_reference.npz")
    np.savez_compressed(path, **out)
    print(f"update_reference:{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
