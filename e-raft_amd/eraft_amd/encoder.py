"""BasicEncoder's residual stages on the MI355X: each ResidualBlock's two 3x3 convolutions as
corr_enc_conv_forward launches (csrc/corr_conv.hip: bf16 MFMA with the exact three-piece split, at
stride 1 or 2).  The norm between two convolutions is never applied to a stored map: the producer
leaves per-tile statistics, corr_enc_norm_finalize turns them into a per-(b, c) scale and shift,
and the consumer normalises (and applies the ReLU) while it stages its input; corr_enc_join does
the same for the block's output and adds the skip.  An eval-mode batch norm brings its scale and
shift from its running statistics instead.  The 7x7 stem, the 1x1 head and the strided blocks'
1x1 projections stay on torch.  Inference only: there is no backward, so model.BasicEncoder takes
this path only when autograd is not recording.
"""
from __future__ import annotations

import weakref

import torch
import torch.nn.functional as F

from . import _lib
from .update import _conv_pack

# Which convolutions take the HIP kernel under the switch, per stage and stride (each is
# judged on its own against the torch ops it replaces, conv + norm + ReLU, at both DSEC encoder
# batch sizes).  One that is False runs on MIOpen with the torch norm.
USE_KERNEL = {"layer1": True, "layer2.s2": True, "layer2": True, "layer3.s2": True, "layer3": True}

_BN_AFFINE = {}  # ids of a BatchNorm2d's tensors -> (weakrefs to them, their (data_ptr, _version)s, scale, shift)


def _bn_affine(norm):
    """(scale, shift), [C] each, of an eval-mode BatchNorm2d: scale = gamma / sqrt(running_var +
    eps), shift = beta - running_mean * scale.  Cached like the packs: by the tensors' ids, held by
    weak references, with the (data_ptr, _version)s they were made from, so an in-place update of
    a parameter or a running statistic recomputes."""
    ts = tuple(t for t in (norm.weight, norm.bias, norm.running_mean, norm.running_var) if t is not None)
    ids = tuple(id(t) for t in ts)
    key = tuple((t.data_ptr(), t._version) for t in ts) + (norm.eps,)
    ent = _BN_AFFINE.get(ids)
    if ent is None or any(r() is not t for r, t in zip(ent[0], ts)) or ent[1] != key:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("encoder_forward: the batch norms' scale and shift must be made before a graph "
                               "capture (run one forward outside the capture first)")
        drop = lambda _r, ids=ids: _BN_AFFINE.pop(ids, None)
        scale = torch.rsqrt(norm.running_var.detach().float() + norm.eps)
        if norm.weight is not None:
            scale = norm.weight.detach().float() * scale
        shift = -norm.running_mean.detach().float() * scale
        if norm.bias is not None:
            shift = norm.bias.detach().float() + shift
        ent = (tuple(weakref.ref(t, drop) for t in ts), key, scale.contiguous(), shift.contiguous())
        _BN_AFFINE[ids] = ent
    return ent[2], ent[3]


def _affine(y, scale, shift):
    """relu(y * scale + shift) on torch, scale and shift [B, C] or [C]."""
    v = (y.shape[0], y.shape[1], 1, 1) if scale.dim() == 2 else (1, y.shape[1], 1, 1)
    return F.relu(y * scale.view(v) + shift.view(v))


def _conv_norm(key, conv, norm, x, in_norm, instance):
    """relu(norm(conv(n(x)))) as (y, scale, shift) with the result relu(y * scale + shift) left to
    the consumer, or as (result, None, None) when the convolution runs on torch.  n(x) is
    relu(x * in_norm[0] + in_norm[1]), or x when in_norm is None."""
    if not USE_KERNEL[key]:
        return F.relu(norm(conv(x if in_norm is None else _affine(x, *in_norm)))), None, None
    packed, bias = _conv_pack((conv,))
    sc, sh = in_norm if in_norm is not None else (None, None)
    if not instance:
        return (_lib.enc_conv_forward(x, packed, bias, conv.out_channels, conv.stride[0], sc, sh), *_bn_affine(norm))
    y, st = _lib.enc_conv_forward(x, packed, bias, conv.out_channels, conv.stride[0], sc, sh, stats=True)
    return (y, *_lib.enc_norm_finalize(st, y.shape[0], y.shape[1], y.shape[2], y.shape[3], norm.eps))


def _block(name, block, x, instance):
    """ResidualBlock.forward (extractor.py:43-52) for `block`."""
    s2 = block.downsample is not None
    y, sc, sh = _conv_norm(name + ".s2" if s2 else name, block.conv1, block.norm1, x, None, instance)
    y, sc, sh = _conv_norm(name, block.conv2, block.norm2, y, None if sc is None else (sc, sh), instance)
    skip = (block.downsample(x) if s2 else x).contiguous()
    if sc is None:
        return F.relu(skip + y)
    return _lib.enc_join(y, sc, sh, skip, out=y)


def encoder_forward(module, x):
    """BasicEncoder.forward (extractor.py:171-189) for `module` on one tensor x [B, C, H, W], fp32
    on the GPU, norm_fn "instance" or (eval mode) "batch".  Returns the [B, output_dim, H/8, W/8]
    features."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("x must be a tensor on an MI355X (HIP) device: eraft_amd has no CPU fallback")
    instance = module.norm_fn == "instance"
    x = F.relu(module.norm1(module.conv1(x.detach()))).contiguous()
    for name in ("layer1", "layer2", "layer3"):
        for block in getattr(module, name):
            x = _block(name, block, x, instance)
    return module.conv2(x)
