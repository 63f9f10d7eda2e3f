"""BasicEncoder on the MI355X: each ResidualBlock's two 3x3 convolutions as corr_enc_conv_forward
launches (csrc/corr_conv.hip: bf16 MFMA with the exact three-piece split, at stride 1 or 2), the
7x7 stem as corr_enc_stem_forward and the strided blocks' 1x1 projections and the 1x1 head as
corr_enc_pw_forward (csrc/corr_enc_front.hip, the same arithmetic).  A norm is never applied to a
stored map: the producer leaves per-tile statistics, corr_enc_norm_finalize turns them into a
per-(b, c) scale and shift, and the consumer normalises (and applies the ReLU) while it stages its
input; corr_enc_join does the same for the block's output and adds the skip, and
corr_enc_join_affine also normalises that skip (the raw stem map with its ReLU, the raw projection
without one).  An eval-mode batch norm brings its scale and shift from its running statistics
instead.  USE_KERNEL says which pieces take a kernel; the others run on torch as they always did.
module.precision (precision.py: "bf16x6", "bf16x3" or "bf16") is the mode of every convolution that
takes a kernel; a piece on torch stays fp32.
Inference only: there is no backward, so model.BasicEncoder takes this path only when autograd is
not recording.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from . import _lib, precision
from ._cache import cached
from .update import _conv_pack

# Which pieces take the HIP kernel under the switch (each is judged on its own
# against the torch ops it replaces at both DSEC encoder batch sizes: a 3x3 convolution against
# conv + norm + ReLU, the stem likewise, a projection against conv + norm, the head against the
# conv).  One that is False runs on MIOpen / rocBLAS with the torch norm and a stored map.
USE_KERNEL = {"layer1": True, "layer2.s2": True, "layer2": True, "layer3.s2": True, "layer3": True,
              "stem": True, "layer2.proj": True, "layer3.proj": True, "head": True}

STEM_MAX_CIN = 16  # corr_enc_stem_forward's bound; a wider stem runs on torch (the stem alone)

def _bn_affine(norm):
    """(scale, shift), [C] each, of an eval-mode BatchNorm2d: scale = gamma / sqrt(running_var +
    eps), shift = beta - running_mean * scale (cached: _cache.py; an in-place update of a parameter
    or a running statistic recomputes)."""
    def make():
        scale = torch.rsqrt(norm.running_var.detach().float() + norm.eps)
        if norm.weight is not None:
            scale = norm.weight.detach().float() * scale
        shift = -norm.running_mean.detach().float() * scale
        if norm.bias is not None:
            shift = norm.bias.detach().float() + shift
        return scale.contiguous(), shift.contiguous()
    ts = tuple(t for t in (norm.weight, norm.bias, norm.running_mean, norm.running_var) if t is not None)
    return cached("bn_affine", ts, "encoder_forward: the batch norms' scale and shift", make, extra=(norm.eps,))


def _front_pack(conv, pack):
    """(pack, bias) of the stem or a 1x1 Conv2d, made by `pack` (_lib.enc_stem_pack_weights or
    _lib.enc_pw_pack_weights; cached: _cache.py)."""
    return cached("front", (conv.weight, conv.bias), "encoder_forward: the convolutions' pack",
                  lambda: (pack(conv.weight), conv.bias.detach().float().contiguous().clone()))


def _affine(y, scale, shift):
    """relu(y * scale + shift) on torch, scale and shift [B, C] or [C]."""
    v = (y.shape[0], y.shape[1], 1, 1) if scale.dim() == 2 else (1, y.shape[1], 1, 1)
    return F.relu(y * scale.view(v) + shift.view(v))


def _norm_of(y, st, norm, instance):
    """(scale, shift) of `norm` on the kernel output y: from its statistics st (instance norm) or
    from the batch norm's running statistics."""
    if not instance:
        return _bn_affine(norm)
    return _lib.enc_norm_finalize(st, y.shape[0], y.shape[1], y.shape[2], y.shape[3], norm.eps)


def _conv_norm(key, conv, norm, x, in_norm, instance, prec=0):
    """relu(norm(conv(n(x)))) as (y, scale, shift) with the result relu(y * scale + shift) left to
    the consumer, or as (result, None, None) when the convolution runs on torch.  n(x) is
    relu(x * in_norm[0] + in_norm[1]), or x when in_norm is None.  prec: the kernel's CORR_PREC_* mode."""
    if not USE_KERNEL[key]:
        return F.relu(norm(conv(x if in_norm is None else _affine(x, *in_norm)))), None, None
    packed, bias = _conv_pack((conv,))
    sc, sh = in_norm if in_norm is not None else (None, None)
    if not instance:
        return (_lib.enc_conv_forward(x, packed, bias, conv.out_channels, conv.stride[0], sc, sh, precision=prec),
                *_bn_affine(norm))
    y, st = _lib.enc_conv_forward(x, packed, bias, conv.out_channels, conv.stride[0], sc, sh, stats=True,
                                  precision=prec)
    return (y, *_norm_of(y, st, norm, True))


def _pw(conv, x, stats=False, prec=0):
    """conv(x) for a 1x1 Conv2d on the pointwise kernel (with the statistics when asked) in the
    CORR_PREC_* mode prec."""
    packed, bias = _front_pack(conv, _lib.enc_pw_pack_weights)
    return _lib.enc_pw_forward(x, packed, bias, conv.out_channels, conv.stride[0], stats=stats, precision=prec)


def _block(name, block, x, x_norm, instance, prec):
    """ResidualBlock.forward (extractor.py:43-52) for `block` on relu(x * x_norm[0] + x_norm[1])
    (the raw stem map and its norm), or on x when x_norm is None."""
    s2 = block.downsample is not None
    y, sc, sh = _conv_norm(name + ".s2" if s2 else name, block.conv1, block.norm1, x, x_norm, instance, prec)
    y, sc, sh = _conv_norm(name, block.conv2, block.norm2, y, None if sc is None else (sc, sh), instance, prec)
    if sc is None:  # conv2 ran on torch: y is normalised already, the join is torch's
        if x_norm is not None:
            x = _affine(x, *x_norm)
        return F.relu((block.downsample(x) if s2 else x) + y)
    if s2 and USE_KERNEL[name + ".proj"]:
        conv, norm = block.downsample[0], block.downsample[1]
        p = _pw(conv, x, stats=instance, prec=prec)
        p, st = p if instance else (p, None)
        return _lib.enc_join_affine(y, sc, sh, p, *_norm_of(p, st, norm, instance), skip_relu=False, out=y)
    if s2:
        return _lib.enc_join(y, sc, sh, block.downsample(x).contiguous(), out=y)
    if x_norm is not None:
        return _lib.enc_join_affine(y, sc, sh, x, *x_norm, skip_relu=True, out=y)
    return _lib.enc_join(y, sc, sh, x, out=y)


def encoder_forward(module, x):
    """BasicEncoder.forward (extractor.py:171-189) for `module` on one tensor x [B, C, H, W], fp32
    on the GPU, norm_fn "instance" or (eval mode) "batch".  Returns the [B, output_dim, H/8, W/8]
    features."""
    if not isinstance(x, torch.Tensor) or x.device.type != "cuda":
        raise RuntimeError("x must be a tensor on an MI355X (HIP) device: eraft_amd has no CPU fallback")
    instance = module.norm_fn == "instance"
    prec = precision.code(module.precision)
    x, x_norm = x.detach().contiguous(), None
    if USE_KERNEL["stem"] and x.shape[1] <= STEM_MAX_CIN:
        packed, bias = _front_pack(module.conv1, _lib.enc_stem_pack_weights)
        y = _lib.enc_stem_forward(x, packed, bias, module.conv1.out_channels, stats=instance, precision=prec)
        x, st = y if instance else (y, None)
        x_norm = _norm_of(x, st, module.norm1, instance)
    else:
        x = F.relu(module.norm1(module.conv1(x))).contiguous()
    for name in ("layer1", "layer2", "layer3"):
        for block in getattr(module, name):
            x, x_norm = _block(name, block, x, x_norm, instance, prec), None
    return _pw(module.conv2, x, prec=prec) if USE_KERNEL["head"] else module.conv2(x)
