"""SepConvGRU on the MI355X: each half step is corr_gru_half_step (two HIP launches on the bf16
MFMA with the exact three-piece split, csrc/corr_gru.hip) instead of six MIOpen convolutions,
four cats and the elementwise kernels between them.  Inference only: there is no backward, so
model.SepConvGRU takes this path only when autograd is not recording.

The module's `precision` ("bf16x6", the class default, "bf16x3" or "bf16": precision.py) selects the
pieces of the split that the six convolutions keep; it acts here only, the torch path ignores it.
"""
from __future__ import annotations

import torch

from . import _lib
from ._cache import cached
from .precision import DEFAULT, code

def _gru_pack(wz, wr, wq):
    """The packed split of one half step's three gate weights (cached: _cache.py)."""
    return cached("gru", (wz, wr, wq), "sepconv_gru: the GRU weights' pack",
                  lambda: _lib.gru_pack_weights(wz, wr, wq))


def half_step(module, h, x, tag):
    """One half step of `module` (a SepConvGRU): tag "1" = convz1/convr1/convq1 (1x5), "2" = the
    5x1 ones, in the module's `precision` (the pack is the same in every mode)."""
    cz, cr, cq = (getattr(module, f"conv{g}{tag}") for g in "zrq")
    packed = _gru_pack(cz.weight, cr.weight, cq.weight)
    return _lib.gru_half_step(h, x, 0 if tag == "1" else 1, packed, cz.bias.detach(), cr.bias.detach(),
                              cq.bias.detach(), precision=code(getattr(module, "precision", DEFAULT)))


def sepconv_gru(module, h, x):
    """SepConvGRU.forward (update.py:45-60) for a module with convz1 .. convq2: the horizontal,
    then the vertical half step, in the module's `precision`.  h [B, 128, H, W], x [B, input, H, W],
    fp32 on the GPU."""
    for t, nm in ((h, "h"), (x, "x")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"{nm} must be a tensor on an MI355X (HIP) device: eraft_amd has no CPU fallback")
    h, x = h.detach().contiguous(), x.detach().contiguous()
    return half_step(module, half_step(module, h, x, "1"), x, "2")
