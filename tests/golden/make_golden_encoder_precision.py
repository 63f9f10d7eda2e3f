"""Generate tests/golden/encoder_precision_reference.npz FROM THE REFERENCE ITSELF: the emulated
end-point errors of the encoders' precision modes (tests/test_encoder_precision.py).

Run where the reference project is present (make_golden_precision.py locates it), never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_encoder_precision.py

The method is make_golden_precision.py's (its helpers are imported, not copied): on the g_e2e_dsec
inputs and weights, cold and warm, the reference runs with the named convolutions evaluated as a
mode defines them (the sum of the fp32 convolutions of the kept pieces of tests/_bf16x6.py's split3,
everything else fp32), and the end-point errors against the reference's own fp32 flow are recorded:

  emu_enc_bf16x3, emu_enc_bf16   the 32 convolutions of fnet and cnet only (`encoder_precision`)
  emu_all_bf16x3, emu_all_bf16   those and make_golden_precision.py's eleven (both knobs)

Each is [low-res cold, full-res cold, low-res warm, full-res warm] in pixels.  The autocast
yardsticks stay in precision_reference.npz.  The fixture is data (EPEs, names and meta), never
reference source.
"""
from __future__ import annotations

import os

import numpy as np
import torch.nn as nn

import make_golden_precision as base  # (puts the reference and tests/ on the path)

HERE = os.path.dirname(os.path.abspath(__file__))


def encoder_convs(model):
    """[(name, module)] of every convolution of fnet and cnet: 16 each (the stem, the twelve 3x3
    convolutions of the stages, the two 1x1 projections, the head)."""
    out = [(f"{enc}.{name}", m) for enc in ("fnet", "cnet") for name, m in getattr(model, enc).named_modules()
           if isinstance(m, nn.Conv2d)]
    assert len(out) == 32, len(out)
    return out


def main():
    g = np.load(os.path.join(HERE, "g_e2e_dsec.npz"))
    res = {"meta": g["meta"], "fp32": base.run(g, lambda m: None)}  # the generator's own check: the golden again
    print("fp32", res["fp32"])
    assert res["fp32"].max() < 1e-3, "this torch does not reproduce the fp32 golden"
    names = []
    for mode in base.PRODUCTS:
        for tag, eleven in (("enc", ()), ("all", base.ELEVEN)):
            def prepare(m, mode=mode, eleven=eleven):
                convs = encoder_convs(m)
                names[:] = [n for n, _ in convs]
                for _, conv in convs:
                    base.emulate(conv, mode)
                for name in eleven:
                    base.emulate(m.update_block.get_submodule(name), mode)
            key = f"emu_{tag}_{mode}"
            res[key] = base.run(g, prepare)
            print(key, res[key])
    res["convs"] = np.array(names)
    path = os.path.join(HERE, "encoder_precision_reference.npz")
    np.savez_compressed(path, **res)
    print(f"encoder_precision_reference: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
