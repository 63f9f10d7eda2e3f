"""Generate tests/golden/gru_reference.npz FROM THE REFERENCE's own SepConvGRU (model/update.py:33-60).
(Not named g_*.npz: test_oracle.py / test_gpu_parity.py treat every g_* file they do not exclude
by prefix as a CorrBlock build case.)

Run where the reference checkout is present (never on the GPU box):

    ERAFT_REFERENCE=<checkout> PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_gru.py

Weights come from prng.param_init keyed by the module's own parameter names ("convz1.weight",
...), h = tanh(prng.gauss(seed)) and x = prng.gauss(seed + 1); the fixture holds the seeds, the
shapes and the reference's fp32 CPU outputs only, never reference source.
"""
from __future__ import annotations

import os
import sys
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
from model.update import SepConvGRU  # noqa: E402  (reference)

torch.set_num_threads(8)

# (seed, B, hidden, input, H, W)
CASES = [(41, 1, 128, 320, 5, 6), (43, 2, 128, 320, 9, 11)]


def gru_inputs(seed, B, hidden, inp, H, W):
    h = np.tanh(prng.gauss(seed, (B, hidden, H, W)).astype(np.float64)).astype(np.float32)
    return h, prng.gauss(seed + 1, (B, inp, H, W))


def main():
    out = {"cases": np.array(CASES, np.int64)}
    for k, (seed, B, hidden, inp, H, W) in enumerate(CASES):
        m = SepConvGRU(hidden_dim=hidden, input_dim=inp).eval()
        with torch.no_grad():
            for name, t in m.state_dict().items():
                t.copy_(torch.from_numpy(prng.param_init(name, tuple(t.shape))))
            h, x = gru_inputs(seed, B, hidden, inp, H, W)
            out[f"h_out{k}"] = m(torch.from_numpy(h), torch.from_numpy(x)).numpy()
    path = os.path.join(HERE, "gru_reference.npz")
    np.savez_compressed(path, **out)
    print(f"gru_reference:{os.path.getsize(path) / 1e6:.2f} MB")


if __name__ == "__main__":
    main()
