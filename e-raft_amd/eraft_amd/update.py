"""BasicUpdateBlock on the MI355X: the block's 3x3 convolutions (convc2, convf2, conv and the two
heads' first convolutions) as corr_conv_forward launches (csrc/corr_conv.hip: bf16 MFMA with the
exact three-piece split, bias and ReLU in the epilogue) that write straight into the buffer their
consumer reads, so the motion encoder's two cats and the [inp, motion] cat go away; the 7x7
convolution of the flow (convf1) as a corr_flow_enc_forward launch that also drops the flow into
the GRU input, and the flow head's second convolution as a corr_flow_head_forward launch that also
updates the coordinates (csrc/corr_flow.hip).  Inference only: there is no backward, so
model.BasicUpdateBlock takes this path only when autograd is not recording.

The module's `precision` ("bf16x6", the class default, "bf16x3" or "bf16": precision.py) selects the
pieces of the split that the five corr_conv_forward launches keep (convc2, convf2, conv,
flow_head.conv1 and mask[0]); the GRU follows its own module's.  convf1 and the flow head's second
convolution, through which the flow enters and the flow delta leaves, stay bf16x6, and the torch
path ignores the mode.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib
from ._cache import cached
from .precision import DEFAULT, code

# Which convolutions take the HIP kernel under the switch (each is judged on its
# own against the torch ops it replaces, at DSEC and at b8).  One that is False runs on MIOpen and
# is copied into the shared buffer.
USE_KERNEL = {"convc2": True, "convf2": True, "conv": True, "heads": True, "convf1": True, "flow_head2": True}

def _conv_pack(convs):
    """(pack, bias) of one launch's Conv2d modules, their weights stacked along cout (cached, as
    the two below: _cache.py)."""
    ts = tuple(c.weight for c in convs) + tuple(c.bias for c in convs)
    return cached("conv", ts, "update_block: the convolutions' pack",
                  lambda: (_lib.conv_pack_weights([c.weight for c in convs]),
                           torch.cat([c.bias.detach().float() for c in convs]).contiguous()))


def _flow_enc_pack(conv):
    """(pack, bias) of the 7x7 flow convolution."""
    return cached("flow_enc", (conv.weight, conv.bias), "update_block: the flow convolution's pack",
                  lambda: (_lib.flow_enc_pack_weights(conv.weight), conv.bias.detach().float().contiguous().clone()))


def _flow_head_pack(conv):
    """(pack, bias) of the flow head's second convolution."""
    return cached("flow_head", (conv.weight, conv.bias), "update_block: the flow head's pack",
                  lambda: (_lib.flow_head_pack_weights(conv.weight), conv.bias.detach().float().contiguous().clone()))


def _conv(name, convs, x, out, off, precision=0):
    """relu(conv(x)) of the stacked `convs` into channels off .. of `out`; `precision` (a
    CORR_PREC_* value) acts on the kernel only."""
    cout = sum(c.out_channels for c in convs)
    if USE_KERNEL[name]:
        packed, bias = _conv_pack(convs)
        _lib.conv_forward(x, None, packed, bias, cout, True, out=out, out_offset=off, precision=precision)
    else:
        for c in convs:
            out[:, off:off + c.out_channels].copy_(F.relu(c(x)))
            off += c.out_channels


class UpdateWorkspace:
    """The buffers update_block fills, kept across the refinement iterations of one forward:
    f1 = relu(convf1(flow)), cf = [convc2 | convf2], x = [inp | conv | flow] (the GRU input; `inp`
    is copied into it here, once), hd = [flow_head.conv1 | mask[0]], and two (coords, flow) pairs
    that the coordinate update alternates between, since it cannot run in place."""

    def __init__(self, inp):
        B, _, H, W = inp.shape
        new = lambda c: torch.empty((B, c, H, W), dtype=torch.float32, device=inp.device)
        self.f1, self.cf, self.x, self.hd = new(128), new(256), new(256), new(512)
        self.x[:, :128].copy_(inp)
        self._new, self._pairs, self._last = new, None, 1

    def coords_pair(self, *inputs):
        """The (coords_out, flow_out) buffers of the next update: the pair not written last, which
        none of `inputs` (this update's coordinates and flow) can be."""
        if self._pairs is None:
            self._pairs = tuple((self._new(2), self._new(2)) for _ in range(2))
        k = 1 - self._last
        taken = {t.data_ptr() for t in inputs}
        if any(b.data_ptr() in taken for b in self._pairs[k]):
            k = 1 - k
        self._last = k
        return self._pairs[k]


def update_block(module, net, inp, corr, flow, fused=False, defer_mask=False, workspace=None, coords1=None,
                 coords0=None):
    """BasicUpdateBlock.forward (update.py:85-107) for `module`: net, inp [B, 128, H, W], corr the
    lookup [B, 324, H, W] (or relu(convc1(lookup)) [B, 256, H, W] when `fused`), flow
    [B, 2, H, W]; fp32 on the GPU.  Returns (net, mask, delta_flow); with `defer_mask`
    (net, hidden, delta_flow), where hidden = relu(mask[0](net)) is the view of channels 256 .. 511
    of the stacked heads' buffer (hidden._base is that buffer, so upsample.mask_upsample reads it
    in place at offset 256) and mask[2] is left to the caller.

    `workspace` (an UpdateWorkspace made from this forward's `inp`) keeps the buffers across
    iterations; without one they are allocated here.  With `coords1` [B, 2, H, W] the result grows
    to (net, mask, delta_flow, coords_out, flow_out): coords_out = coords1 + delta_flow and, with
    `coords0`, flow_out = coords_out - coords0 (else None), in buffers of the workspace that the
    call after the next one overwrites."""
    for t, nm in ((net, "net"), (inp, "inp"), (corr, "corr"), (flow, "flow")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"{nm} must be a tensor on an MI355X (HIP) device: eraft_amd has no CPU fallback")
    if coords0 is not None and coords1 is None:
        raise ValueError("coords0 needs coords1")
    enc = module.encoder
    prec = code(getattr(module, "precision", DEFAULT))
    net, inp, corr, flow = (t.detach() for t in (net, inp, corr, flow))
    ws = workspace if workspace is not None else UpdateWorkspace(inp)
    if tuple(ws.x.shape) != (net.shape[0], 256, *net.shape[2:]) or ws.x.device != net.device:
        raise ValueError(f"workspace was made for {tuple(ws.x.shape)} on {ws.x.device}, net is {tuple(net.shape)} "
                         f"on {net.device}")
    c1 = (corr if fused else F.relu(enc.convc1(corr))).contiguous()
    cf, x, hd = ws.cf, ws.x, ws.hd
    _conv("convc2", (enc.convc2,), c1, cf, 0, prec)
    flow = flow.contiguous()
    if USE_KERNEL["convf1"]:
        packed, bias = _flow_enc_pack(enc.convf1)
        _lib.flow_enc_forward(flow, packed, bias, 128, True, out=ws.f1, flow_copy=x, copy_offset=254)
    else:
        ws.f1.copy_(F.relu(enc.convf1(flow)))
        x[:, 254:].copy_(flow)
    _conv("convf2", (enc.convf2,), ws.f1, cf, 192, prec)
    _conv("conv", (enc.conv,), cf, x, 128, prec)
    net = module.gru(net.contiguous(), x)
    _conv("heads", (module.flow_head.conv1, module.mask[0]), net.contiguous(), hd, 0, prec)
    head2 = module.flow_head.conv2
    coords_out = flow_out = None
    if coords1 is not None:
        coords1 = coords1.detach().contiguous()
        coords0 = None if coords0 is None else coords0.detach().contiguous()
        coords_out, flow_out = ws.coords_pair(coords1, flow, *(() if coords0 is None else (coords0,)))
        if coords0 is None:
            flow_out = None
    if USE_KERNEL["flow_head2"]:
        packed, bias = _flow_head_pack(head2)
        delta = _lib.flow_head_forward(hd, 0, packed, bias, coords_in=coords1, coords0=coords0,
                                       coords_out=coords_out, flow_out=flow_out)[0]
    else:
        delta = head2(hd[:, :256])
        if coords1 is not None:
            torch.add(coords1, delta, out=coords_out)
            if coords0 is not None:
                torch.sub(coords_out, coords0, out=flow_out)
    mask = hd[:, 256:] if defer_mask else 0.25 * module.mask[2](hd[:, 256:])
    if coords1 is None:
        return net, mask, delta
    return net, mask, delta, coords_out, flow_out
