"""BasicUpdateBlock on the MI355X: the block's 3x3 convolutions (convc2, convf2, conv and the two
heads' first convolutions) as corr_conv_forward launches (csrc/corr_conv.hip: bf16 MFMA with the
exact three-piece split, bias and ReLU in the epilogue) that write straight into the buffer their
consumer reads, so the motion encoder's two cats and the [inp, motion] cat go away.  Inference
only: there is no backward, so model.BasicUpdateBlock takes this path only when autograd is not
recording.
"""
from __future__ import annotations

import weakref

import torch
import torch.nn.functional as F

from . import _lib

# Which convolutions take the HIP kernel under the switch (each is judged on its own
# against the torch ops it replaces, at DSEC and at b8).  One that is False runs on MIOpen and is
# copied into the shared buffer.
USE_KERNEL = {"convc2": True, "convf2": True, "conv": True, "heads": True}

_CONV_PACKS = {}  # ids of the weights and biases -> (weakrefs to them, their (data_ptr, _version)s, pack, bias)


def _conv_pack(convs):
    """(pack, bias) of one launch's Conv2d modules (their weights stacked along cout), cached with
    gru._gru_pack's scheme: keyed by the parameters' ids, held by weak references, together with
    the (data_ptr, _version)s they were made from, so another module's tensors never see this
    pack and an in-place update re-packs."""
    ts = tuple(c.weight for c in convs) + tuple(c.bias for c in convs)
    ids = tuple(id(t) for t in ts)
    key = tuple((t.data_ptr(), t._version) for t in ts)
    ent = _CONV_PACKS.get(ids)
    if ent is None or any(r() is not t for r, t in zip(ent[0], ts)) or ent[1] != key:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("update_block: the convolution weights must be packed before a graph capture "
                               "(run one forward outside the capture first)")
        drop = lambda _r, ids=ids: _CONV_PACKS.pop(ids, None)
        bias = torch.cat([c.bias.detach().float() for c in convs]).contiguous()
        ent = (tuple(weakref.ref(t, drop) for t in ts), key, _lib.conv_pack_weights([c.weight for c in convs]), bias)
        _CONV_PACKS[ids] = ent
    return ent[2], ent[3]


def _conv(name, convs, x, out, off):
    """relu(conv(x)) of the stacked `convs` into channels off .. of `out`."""
    cout = sum(c.out_channels for c in convs)
    if USE_KERNEL[name]:
        packed, bias = _conv_pack(convs)
        _lib.conv_forward(x, None, packed, bias, cout, True, out=out, out_offset=off)
    else:
        for c in convs:
            out[:, off:off + c.out_channels].copy_(F.relu(c(x)))
            off += c.out_channels


def update_block(module, net, inp, corr, flow, fused=False, defer_mask=False):
    """BasicUpdateBlock.forward (update.py:85-107) for `module`: net, inp [B, 128, H, W], corr the
    lookup [B, 324, H, W] (or relu(convc1(lookup)) [B, 256, H, W] when `fused`), flow
    [B, 2, H, W]; fp32 on the GPU.  Returns (net, mask, delta_flow); with `defer_mask`
    (net, hidden, delta_flow), where hidden = relu(mask[0](net)) is the view of channels 256 .. 511
    of the stacked heads' buffer (hidden._base is that buffer, so upsample.mask_upsample reads it
    in place at offset 256) and mask[2] is left to the caller."""
    for t, nm in ((net, "net"), (inp, "inp"), (corr, "corr"), (flow, "flow")):
        if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
            raise RuntimeError(f"{nm} must be a tensor on an MI355X (HIP) device: eraft_amd has no CPU fallback")
    enc = module.encoder
    net, inp, corr, flow = (t.detach() for t in (net, inp, corr, flow))
    B, _, H, W = net.shape
    c1 = (corr if fused else F.relu(enc.convc1(corr))).contiguous()
    cf = torch.empty((B, 256, H, W), dtype=torch.float32, device=net.device)  # [convc2 | convf2]
    _conv("convc2", (enc.convc2,), c1, cf, 0)
    _conv("convf2", (enc.convf2,), F.relu(enc.convf1(flow)).contiguous(), cf, 192)
    x = torch.empty((B, 256, H, W), dtype=torch.float32, device=net.device)   # [inp | conv | flow]
    x[:, :128].copy_(inp)
    x[:, 254:].copy_(flow)
    _conv("conv", (enc.conv,), cf, x, 128)
    net = module.gru(net.contiguous(), x)
    hd = torch.empty((B, 512, H, W), dtype=torch.float32, device=net.device)  # [flow_head.conv1 | mask[0]]
    _conv("heads", (module.flow_head.conv1, module.mask[0]), net.contiguous(), hd, 0)
    if defer_mask:
        return net, hd[:, 256:], module.flow_head.conv2(hd[:, :256])
    return net, 0.25 * module.mask[2](hd[:, 256:]), module.flow_head.conv2(hd[:, :256])
