"""OnDemandCorrBlock — CorrBlock's lookups without the all-pairs volume.

RAFT's AlternateCorrBlock for the MI355X (the reference E-RAFT keeps the import commented out,
model/corr.py:5-9): same constructor and call signature as CorrBlock, same output within the
project's tolerance, but nothing of size N^2 is ever materialised.  The block holds only the
pixel-major feature rows of fmap1 and of fmap2 pooled 0 .. L-1 times (corr_ondemand_prepare); each
call computes just the correlation entries its taps touch (corr_ondemand_lookup).  Use it where the
pyramid does not fit (large maps, large batches); CorrBlock stays the default.  The block has no
corr_pyramid and no lookup_conv.

OnDemandConvCorrBlock is the same block with CorrBlock's lookup_conv(coords, weight, bias): at
inference relu(convc1(lookup)) is one launch (corr_ondemand_lookup_conv) and the 324-channel
lookup is never stored; where autograd would record it is the unfused composition.  ERAFT builds
it with alternate_corr and ERAFT_AMD_ONDEMAND_FUSE_CONV=1 (default off).

train=True puts the block in the autograd graph (gradients to fmap1 / fmap2 only; coords are
detached, as in CorrBlock), following corr.py's pattern: the prepare is an autograd function whose
output is a token, every lookup is an autograd function of the token whose backward only stashes
its (coords, upstream gradient), and the prepare's backward runs corr_ondemand_backward once over
the stash in call order — window gradients and dF1 per query, dF2 as a deterministic gather per
8 x 8 tile of target cells, nothing of size N^2.  The forward workspace is kept for the backward;
the backward workspace is allocated in the backward.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from .corr import _validate_fmaps, _weight_pack


class _OdState:
    """Per-block state shared by the prepare and lookup autograd nodes."""

    __slots__ = ("ws", "D", "levels", "radius", "stash")

    def __init__(self, D, levels, radius):
        self.ws = None    # the forward workspace (corr_ondemand_prepare)
        self.stash = []   # (call number, coords, grad_out) of every lookup backward, in backward order
        self.D, self.levels, self.radius = D, levels, radius


class _PrepareFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, fmap1, fmap2, state):
        B, D, H, W = fmap1.shape
        state.ws = _lib.ondemand_workspace(B, D, H, W, state.levels, fmap1.device)
        _lib.ondemand_prepare(fmap1, fmap2, state.levels, state.ws)
        ctx.set_materialize_grads(False)
        ctx.state = state
        # autograd anchor: every lookup depends on it; its value is never read
        return fmap1.new_empty(())

    @staticmethod
    def backward(ctx, _token_grad):
        st = ctx.state
        stash, st.stash = st.stash, []
        want1, want2 = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not stash or not (want1 or want2):
            return None, None, None
        # lookups' backwards run in reverse call order: restore the call order
        stash.sort(key=lambda e: e[0])
        df1, df2 = _lib.ondemand_backward(st.ws, [c for _, c, _ in stash], [g for _, _, g in stash], st.D,
                                          st.levels, st.radius, want1=want1, want2=want2)
        return df1, df2, None


class _OdLookupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, coords, token, state, flags, seq):
        B, _, H, W = coords.shape
        K = (2 * state.radius + 1) ** 2
        out = torch.empty((B, state.levels * K, H, W), dtype=torch.float32, device=coords.device)
        _lib.ondemand_lookup(state.ws, coords, state.D, state.levels, state.radius, out, flags)
        ctx.save_for_backward(coords)
        ctx.state, ctx.seq = state, seq
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (coords,) = ctx.saved_tensors
        ctx.state.stash.append((ctx.seq, coords, grad_out.contiguous()))
        # no gradient for the token: the engine still runs the prepare's backward after every lookup's
        return None, None, None, None, None


class OnDemandCorrBlock:
    """CorrBlock(fmap1, fmap2, num_levels, radius)'s lookups computed from the feature maps."""

    def __init__(self, fmap1, fmap2, num_levels=4, radius=4, flags=0, train=False):
        self.num_levels = num_levels
        self.radius = radius
        self.flags = flags
        if not (0 <= radius <= _lib.MAX_RADIUS):
            raise ValueError(f"radius must be in [0, {_lib.MAX_RADIUS}]")
        _validate_fmaps(fmap1, fmap2, num_levels)
        self._token = self._state = None
        self._calls = 0
        self._B, self._D, self._H, self._W = fmap1.shape
        if torch.is_grad_enabled() and (fmap1.requires_grad or fmap2.requires_grad):
            if not train:
                raise NotImplementedError("OnDemandCorrBlock(train=False) has no backward: pass train=True, "
                                          "construct it under torch.no_grad() or from detached maps, or use "
                                          "CorrBlock")
            self._state = _OdState(self._D, num_levels, radius)
            self._token = _PrepareFn.apply(fmap1.contiguous().float(), fmap2.contiguous().float(), self._state)
            self._ws = self._state.ws
            return
        fmap1 = fmap1.detach().contiguous().float()
        fmap2 = fmap2.detach().contiguous().float()
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
        if self._token is not None and torch.is_grad_enabled():
            self._calls += 1
            return _OdLookupFn.apply(coords, self._token, self._state, self.flags, self._calls)
        K = (2 * self.radius + 1) ** 2
        out = torch.empty((B, self.num_levels * K, H, W), dtype=torch.float32, device=coords.device)
        _lib.ondemand_lookup(self._ws, coords, self._D, self.num_levels, self.radius, out, self.flags)
        return out


class OnDemandConvCorrBlock(OnDemandCorrBlock):
    """OnDemandCorrBlock with CorrBlock.lookup_conv: the lookup fused with the motion encoder's
    first layer (radius 4, at most 4 levels)."""

    def lookup_conv(self, coords, weight, bias, relu=True):
        """relu(convc1(self(coords))) (update.py:68,75) without materialising the lookup output.
        weight: convc1.weight [256, L*K, 1, 1]; bias [256].  One corr_ondemand_lookup_conv launch
        under no_grad or when nothing requires grad; where autograd would record (a train=True
        block with grad enabled, or a weight / bias that requires grad) it is the unfused
        composition, bit for bit — there is no fused backward."""
        self._check_coords(coords)
        B, _, H, W = coords.shape
        K = (2 * self.radius + 1) ** 2
        C = self.num_levels * K
        if tuple(weight.shape) not in ((256, C, 1, 1), (256, C)) or tuple(bias.shape) != (256,):
            raise ValueError(f"lookup_conv needs weight [256, {C}, 1, 1] and bias [256] "
                             f"(got {tuple(weight.shape)}, {tuple(bias.shape)})")
        if torch.is_grad_enabled() and (self._token is not None or weight.requires_grad or bias.requires_grad):
            out = F.conv2d(self(coords), weight.reshape(256, C, 1, 1), bias)
            return F.relu(out) if relu else out
        coords = coords.detach().contiguous()
        packed = _weight_pack(weight)  # CorrBlock.lookup_conv's pack and cache entry
        out = torch.empty((B, 256, H, W), dtype=torch.float32, device=coords.device)
        _lib.ondemand_lookup_conv(self._ws, coords, self._D, self.num_levels, self.radius, packed,
                                  bias.detach().contiguous().float(), out, relu, self.flags)
        return out
