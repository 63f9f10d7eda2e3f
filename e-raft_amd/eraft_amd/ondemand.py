"""OnDemandCorrBlock — CorrBlock's lookups without the all-pairs volume.

RAFT's AlternateCorrBlock for the MI355X (the reference E-RAFT keeps the import commented out,
model/corr.py:5-9): same constructor and call signature as CorrBlock, same output within the
project's tolerance, but nothing of size N^2 is ever materialised.  The block holds only the
pixel-major feature rows of fmap1 and of fmap2 pooled 0 .. L-1 times (corr_ondemand_prepare); each
call computes just the correlation entries its taps touch (corr_ondemand_lookup).  Use it where the
pyramid does not fit (large maps, large batches); CorrBlock stays the default and the training
path: this block is inference only (no backward), has no corr_pyramid and no lookup_conv.
"""
from __future__ import annotations

import torch

from . import _lib
from .corr import _validate_fmaps


class OnDemandCorrBlock:
    """CorrBlock(fmap1, fmap2, num_levels, radius)'s lookups computed from the feature maps."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, flags=0):
        self.num_levels = num_levels
        self.radius = radius
        self.flags = flags
        if not (0 <= radius <= _lib.MAX_RADIUS):
            raise ValueError(f"radius must be in [0, {_lib.MAX_RADIUS}]")
        _validate_fmaps(fmap1, fmap2, num_levels)
        if torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad):
            raise NotImplementedError("OnDemandCorrBlock is inference only (no backward): construct it under "
                                      "torch.no_grad() or from detached maps; CorrBlock is the training path")
        fmap1 = fmap1.detach().contiguous().float()
        fmap2 = fmap2.detach().contiguous().float()
        self._B, self._D, self._H, self._W = fmap1.shape
        self._ws = _lib.ondemand_workspace(self._B, self._D, self._H, self._W, num_levels, fmap1.device)
        _lib.ondemand_prepare(fmap1, fmap2, num_levels, self._ws)

    def _check_coords(self, coords):
        if coords.dim() != 4 or coords.shape[1] != 2:
            raise ValueError(f"coords must be [B, 2, H, W] (got {tuple(coords.shape)})")
        B, _, H, W = coords.shape
        if B != self._B or (H, W) != (self._H, self._W):
            raise ValueError("coords do not match the feature maps this block was built from")

    def __call__(self, coords):
        self._check_coords(coords)
        B, _, H, W = coords.shape
        coords = coords.detach().contiguous()  # any strides, as CorrBlock
        K = (2 * self.radius + 1) ** 2
        out = torch.empty((B, self.num_levels * K, H, W), dtype=torch.float32, device=coords.device)
        _lib.ondemand_lookup(self._ws, coords, self._D, self.num_levels, self.radius, out, self.flags)
        return out
