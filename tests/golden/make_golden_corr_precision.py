"""Generate tests/golden/corr_precision_reference.npz FROM THE REFERENCE ITSELF: the yardsticks of the
correlation build's precision modes (tests/test_corr_precision.py).

Run in the survey container only (needs /root/reference, never present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_corr_precision.py

On the g_e2e_dsec inputs and weights, cold and warm (flow_init from that golden), it records the
end-point errors against the reference's own fp32 flow (g_e2e_dsec's low, up_sub, low_warm,
up_warm_sub) of

  emu_bf16x3, emu_bf16
      the reference with its all-pairs correlation (CorrBlock.corr) evaluated as the mode defines it:
      the sum, taken in fp64 and rounded once to fp32, of the products among the kept pieces of
      tests/_bf16x6.py's split3 of both feature maps, over sqrt(D).  Everything else is the
      reference's fp32.

Each is [low-res cold, full-res cold, low-res warm, full-res warm] in pixels (full-res on every
4th pixel, as the golden stores it).  The fixture is data (EPEs and the inputs' seeds), never
reference source.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import prng  # noqa: E402
import _bf16x6 as bx  # noqa: E402

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
import model.corr as ref_corr  # noqa: E402  (reference)
import model.eraft as ref_eraft  # noqa: E402  (reference)

torch.set_num_threads(8)

# (target piece, query piece) of each product a mode keeps (csrc/corr_build_bf16.hip)
PRODUCTS = {"bf16x3": ((1, 0), (0, 1), (0, 0)), "bf16": ((0, 0),)}


def init_model(model):
    with torch.no_grad():
        for name, t in model.state_dict().items():
            v = prng.param_init(name, tuple(t.shape))
            if v is not None:
                t.copy_(torch.from_numpy(v))


def mode_corr(mode):
    """The mode's value of the all-pairs volume [B, H, W, 1, H, W]."""

    def corr(fmap1, fmap2):
        B, D, H, W = fmap1.shape
        qp = [torch.from_numpy(p).double().view(B, D, H * W) for p in bx.split3(fmap1.detach().float().numpy())]
        tp = [torch.from_numpy(p).double().view(B, D, H * W) for p in bx.split3(fmap2.detach().float().numpy())]
        out = None
        for a, b in PRODUCTS[mode]:
            term = torch.matmul(qp[b].transpose(1, 2), tp[a])
            out = term if out is None else out + term
        return (out / np.sqrt(np.float64(D))).float().view(B, H, W, 1, H, W)

    return corr


def epe(a, b):
    return float(torch.sqrt(((a.float() - b) ** 2).sum(dim=1)).mean())


def run(g):
    """[low cold, up cold, low warm, up warm] EPE of a freshly initialised reference model against
    the fp32 golden."""
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W)))
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W)))
    out = []
    for init, low_k, up_k in ((None, "low", "up_sub"), (torch.from_numpy(g["flow_init"]), "low_warm", "up_warm_sub")):
        model = ref_eraft.ERAFT({"subtype": "warm_start"}, n_first_channels=bins).eval()
        init_model(model)
        with torch.no_grad():
            low, ups = model(im1, im2, iters=iters, flow_init=init)
        out += [epe(low, torch.from_numpy(g[low_k])), epe(ups[-1][..., ::4, ::4], torch.from_numpy(g[up_k]))]
    return np.array(out, np.float64)


def main():
    g = np.load(os.path.join(HERE, "g_e2e_dsec.npz"))
    res = {"meta": g["meta"]}
    res["fp32"] = run(g)          # the generator's own check: the golden again
    print("fp32", res["fp32"])
    assert res["fp32"].max() < 1e-3, "this torch does not reproduce the fp32 golden"
    real = ref_corr.CorrBlock.__dict__["corr"]
    try:
        for mode in PRODUCTS:
            ref_corr.CorrBlock.corr = staticmethod(mode_corr(mode))
            res["emu_" + mode] = run(g)
            print("emu", mode, res["emu_" + mode])
    finally:
        ref_corr.CorrBlock.corr = real
    path = os.path.join(HERE, "corr_precision_reference.npz")
    np.savez_compressed(path, **res)
    print(f"corr_precision_reference: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
