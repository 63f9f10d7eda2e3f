"""Generate tests/golden/pointwise_precision_reference.npz FROM THE REFERENCE ITSELF: the emulated
end-point errors of the precision modes of lookup + convc1 and of the mask head (DESIGN §34;
tests/test_pointwise_precision.py).

Run where the reference project is present (make_golden_precision.py locates it), never on the GPU box:

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pointwise_precision.py

The method is make_golden_precision.py's (its helpers are imported, not copied): on the g_e2e_dsec
inputs and weights, cold and warm, the reference runs with the named convolutions evaluated as a
mode defines them (the sum of the fp32 convolutions of the kept pieces of tests/_bf16x6.py's split3,
everything else fp32), and the end-point errors against the reference's own fp32 flow are recorded:

  emu_bf16x3, emu_bf16       encoder.convc1 and mask.2 only (`pointwise_precision`)
  emu13_bf16x3, emu13_bf16   those two and make_golden_precision.py's eleven (with `mixed_precision`)

Each is [low-res cold, full-res cold, low-res warm, full-res warm] in pixels.  The fixture is data
(EPEs, names and meta), never reference source.
"""
from __future__ import annotations

import os

import numpy as np

import make_golden_precision as base  # (puts the reference and tests/ on the path)

HERE = os.path.dirname(os.path.abspath(__file__))
TWO = ["encoder.convc1", "mask.2"]


def main():
    g = np.load(os.path.join(HERE, "g_e2e_dsec.npz"))
    res = {"meta": g["meta"], "two": np.array(TWO), "eleven": np.array(base.ELEVEN),
           "fp32": base.run(g, lambda m: None)}  # the generator's own check: the golden again
    print("fp32", res["fp32"])
    assert res["fp32"].max() < 1e-3, "this torch does not reproduce the fp32 golden"
    for mode in base.PRODUCTS:
        for tag, names in (("emu", TWO), ("emu13", TWO + base.ELEVEN)):
            def prepare(m, mode=mode, names=names):
                for name in names:
                    base.emulate(m.update_block.get_submodule(name), mode)
            key = f"{tag}_{mode}"
            res[key] = base.run(g, prepare)
            print(key, res[key])
    path = os.path.join(HERE, "pointwise_precision_reference.npz")
    np.savez_compressed(path, **res)
    print(f"pointwise_precision_reference: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
