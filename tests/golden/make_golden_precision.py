"""Generate tests/golden/precision_reference.npz FROM THE REFERENCE ITSELF: the yardsticks of the
precision modes (tests/test_precision.py).

Run in the survey container only (needs /root/reference, never present on the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_precision.py

On the g_e2e_dsec inputs and weights, cold and warm (flow_init from that golden), it records the
end-point errors against the reference's own fp32 flow (g_e2e_dsec's low, up_sub, low_warm,
up_warm_sub) of

  autocast_float16, autocast_bfloat16
      the reference under its own mixed_precision=True, its module-level `autocast` pointed at
      torch.autocast("cpu", dtype);
  emu_bf16x3, emu_bf16
      the reference with the eleven convolutions of the feature (the GRU's six, convc2, convf2,
      conv, flow_head.conv1 and mask[0]) evaluated as the mode defines them: the sum of the fp32
      convolutions of the kept pieces of tests/_bf16x6.py's split3, everything else fp32.

Each is [low-res cold, full-res cold, low-res warm, full-res warm] in pixels (full-res on every
4th pixel, as the golden stores it).  The fixture is data (EPEs and meta), never reference source.
"""
from __future__ import annotations

import os
import sys
import warnings

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import prng  # noqa: E402
import _bf16x6 as bx  # noqa: E402

REF = "/root/reference"
sys.dont_write_bytecode = True
sys.path.insert(0, REF)
warnings.filterwarnings("ignore")
import model.eraft as ref_eraft  # noqa: E402  (reference)

torch.set_num_threads(8)

ELEVEN = [f"gru.conv{g}{t}" for t in "12" for g in "zrq"] + ["encoder.convc2", "encoder.convf2", "encoder.conv",
                                                              "flow_head.conv1", "mask.0"]
# (weight piece, activation piece) of each product, the small ones first (csrc/corr_bf16x6.h)
PRODUCTS = {"bf16x3": ((1, 0), (0, 1), (0, 0)), "bf16": ((0, 0),)}


def init_model(model):
    with torch.no_grad():
        for name, t in model.state_dict().items():
            v = prng.param_init(name, tuple(t.shape))
            if v is not None:
                t.copy_(torch.from_numpy(v))


def pieces(t):
    return [torch.from_numpy(p) for p in bx.split3(t.detach().numpy())]


def emulate(conv, mode):
    """conv.forward = the mode's value of the convolution: fp32 convolutions of the kept pieces, the
    smaller products summed first and the leading one added to them, then the bias."""
    wp = pieces(conv.weight)

    def forward(x):
        xp = pieces(x.contiguous())
        terms = [F.conv2d(xp[b], wp[a], None, conv.stride, conv.padding) for a, b in PRODUCTS[mode]]
        small = sum(terms[1:-1], terms[0]) if len(terms) > 1 else None
        out = terms[-1] if small is None else terms[-1] + small
        return out + conv.bias.view(1, -1, 1, 1)

    conv.forward = forward


def epe(a, b):
    return float(torch.sqrt(((a.float() - b) ** 2).sum(dim=1)).mean())


def run(g, prepare):
    """[low cold, up cold, low warm, up warm] EPE of a freshly initialised reference model after
    prepare(model) against the fp32 golden."""
    seed, H, W, bins, iters = (int(v) for v in g["meta"])
    im1 = torch.from_numpy(prng.voxel_grid(seed, (1, bins, H, W)))
    im2 = torch.from_numpy(prng.voxel_grid(seed + 2, (1, bins, H, W)))
    out = []
    for init, low_k, up_k in ((None, "low", "up_sub"), (torch.from_numpy(g["flow_init"]), "low_warm", "up_warm_sub")):
        model = ref_eraft.ERAFT({"subtype": "warm_start"}, n_first_channels=bins).eval()
        init_model(model)
        prepare(model)
        with torch.no_grad():
            low, ups = model(im1, im2, iters=iters, flow_init=init)
        out += [epe(low, torch.from_numpy(g[low_k])), epe(ups[-1][..., ::4, ::4], torch.from_numpy(g[up_k]))]
    return np.array(out, np.float64)


def main():
    g = np.load(os.path.join(HERE, "g_e2e_dsec.npz"))
    # mean_abs_flow: the mean magnitude of the fp32 golden's low-resolution cold flow, in px
    res = {"meta": g["meta"], "eleven": np.array(ELEVEN),
           "mean_abs_flow": np.array([float(np.sqrt((g["low"].astype(np.float64) ** 2).sum(axis=1)).mean())])}
    res["fp32"] = run(g, lambda m: None)          # the generator's own check: the golden again
    print("fp32", res["fp32"])
    assert res["fp32"].max() < 1e-3, "this torch does not reproduce the fp32 golden"
    for mode in PRODUCTS:
        def prepare(m, mode=mode):
            for name in ELEVEN:
                emulate(m.update_block.get_submodule(name), mode)
        res["emu_" + mode] = run(g, prepare)
        print("emu", mode, res["emu_" + mode])
    real = ref_eraft.autocast
    try:
        for dtype in (torch.float16, torch.bfloat16):
            ref_eraft.autocast = lambda enabled, dtype=dtype: torch.autocast("cpu", dtype=dtype, enabled=enabled)
            key = "autocast_" + str(dtype).split(".")[1]
            res[key] = run(g, lambda m: setattr(m.args, "mixed_precision", True))
            print(key, res[key])
    finally:
        ref_eraft.autocast = real
    path = os.path.join(HERE, "precision_reference.npz")
    np.savez_compressed(path, **res)
    print(f"precision_reference: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
