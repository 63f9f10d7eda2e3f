"""The update block's mask head fused with the convex upsampling on the MI355X: one
corr_mask_upsample_forward launch (csrc/corr_mask_upsample.hip: the 256 -> 576 1x1 convolution on
the bf16 MFMA with the exact three-piece split, softmax over the 9 taps and the convex combination
in registers) from relu(mask[0](net)) and the 1/8-resolution flow to the full-resolution
prediction, so the 576-channel mask never reaches memory.  Inference only: there is no backward,
so model.ERAFT takes this path only when autograd is not recording.
"""
from __future__ import annotations

import torch

from . import _lib, precision as _precision
from ._cache import cached

def _mask_pack(conv):
    """(pack, bias) of the mask head's 1x1 Conv2d (cached: _cache.py)."""
    return cached("mask", (conv.weight, conv.bias), "mask_upsample: the mask head's pack",
                  lambda: (_lib.mask_upsample_pack_weights(conv.weight),
                           conv.bias.detach().float().contiguous().clone()))


def channel_window(t):
    """(buffer, offset) with t = buffer[:, offset:offset + t.shape[1]] and buffer contiguous: t
    itself, the buffer a channel slice such as update_block's deferred `hidden` views (no copy), or
    a contiguous copy of anything else."""
    if t.is_contiguous():
        return t, 0
    base = t._base
    if (base is not None and base.dim() == 4 and t.dim() == 4 and base.is_contiguous() and base.shape[0] == t.shape[0]
            and base.shape[2:] == t.shape[2:] and t.stride() == base.stride()):
        hw = base.shape[2] * base.shape[3]
        d = t.storage_offset() - base.storage_offset()
        if d >= 0 and d % hw == 0 and d // hw + t.shape[1] <= base.shape[1]:
            return base, d // hw
    return t.contiguous(), 0


def mask_upsample(conv, hidden, hidden_offset, flow, scale=0.25, precision="bf16x6"):
    """ERAFT.upsample_flow(flow, scale * conv(hidden[:, hidden_offset:hidden_offset + 256])) for the
    1x1 Conv2d `conv` (256 -> 576, with bias): hidden [B, C, H, W] (read in place), flow
    [B, 2, H, W]; fp32 on the GPU.  precision: the convolution's mode, "bf16x6", "bf16x3" or "bf16"
    (precision.py; the softmax and the combination are fp32 in every mode).  Returns the prediction
    [B, 2, 8H, 8W]."""
    mode = _precision.code(precision)
    for t, nm in ((hidden, "hidden"), (flow, "flow")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"{nm} must be a tensor on an MI355X (HIP) device: eraft_amd has no CPU fallback")
    if tuple(conv.weight.shape) != (576, 256, 1, 1) or conv.bias is None:
        raise ValueError(f"mask_upsample needs a 256 -> 576 1x1 convolution with a bias "
                         f"(got weight {tuple(conv.weight.shape)})")
    packed, bias = _mask_pack(conv)
    return _lib.mask_upsample_forward(hidden.detach(), hidden_offset, flow.detach().contiguous(), packed, bias, scale,
                                      precision=mode)
