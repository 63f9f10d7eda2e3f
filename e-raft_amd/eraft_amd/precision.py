"""The precision modes of the convolution kernels and of the correlation build
(include/corr_mi355x.h: CORR_PREC_*), the counterpart of the reference's mixed_precision
(model/eraft.py:31,102-133).

A mode names the pieces of the exact three-piece bf16 split that a kernel keeps of both operands:

  "bf16x6"  hi, mid, lo: six products per fp32 product, no narrower than fp32 (the default)
  "bf16x3"  hi, mid: three products, operands to 2^-18 and the dropped mid x mid to 2^-16 relative
  "bf16"    hi: one product, operands to 2^-9 relative

Accumulation is fp32 in every mode.  Four knobs choose a mode, each for its own layers:

  `mixed_precision` / ERAFT_AMD_PRECISION (resolve)
      the fused GRU half steps (the eight convolutions of SepConvGRU) and the update block's fused
      3x3 convolutions (convc2, convf2, conv, the flow head's and the mask head's first), where those
      kernels run: inference with ERAFT_AMD_FUSE_GRU=1 / ERAFT_AMD_FUSE_UPDATE=1.
  `encoder_precision` / ERAFT_AMD_ENCODER_PRECISION (resolve_encoder)
      the 32 convolutions of fnet and cnet (each: the 7x7 stem, the twelve 3x3 convolutions of the
      residual stages, the two 1x1 projections and the 1x1 head), where encoder.encoder_forward runs:
      inference with ERAFT_AMD_FUSE_ENCODER=1 on fp32 GPU tensors.  A piece that encoder.USE_KERNEL
      leaves on torch stays fp32.
  `corr_precision` / ERAFT_AMD_CORR_PRECISION (resolve_corr)
      the all-pairs correlation build of CorrBlock (the bf16 MFMA build, ERAFT_AMD_BUILD unset or
      bf16x6), at inference.  The reference casts both feature maps to fp32 before CorrBlock,
      outside its autocast (model/eraft.py:106-108), so `mixed_precision` does NOT switch this on:
      only its own key and variable do.  A build recorded for autograd runs "bf16x6"; the
      on-demand blocks (no all-pairs volume) use the fp32 MFMA and ignore it.

  `pointwise_precision` / ERAFT_AMD_POINTWISE_PRECISION (resolve_pointwise)
      the two 1x1 convolutions of the update loop that are fused with their neighbours: convc1
      inside CorrBlock.lookup_conv (ERAFT_AMD_FUSE_CONV, on by default; the looked-up values are
      the same in every mode, only the product after them changes) and the mask head's second
      convolution inside upsample.mask_upsample (ERAFT_AMD_FUSE_UPSAMPLE=1), at inference.  A
      lookup_conv recorded for autograd runs "bf16x6"; the on-demand blocks ignore it.
      `mixed_precision` does NOT set it: it keeps the reach it had.

The reference's single switch wraps the encoders and the update block in one autocast
(model/eraft.py:102-133, model/update.py:68,75,99-107), so it corresponds to setting the first two
and the fourth.  The torch paths and training stay fp32 and ignore all four; convf1 and the flow
head's second convolution stay "bf16x6" under any of them (the flow enters and leaves through
them), as does the on-demand lookup fused with convc1 (the lookups read whatever values the build
left in the pyramid).
"""
from __future__ import annotations

import os

BF16X6, BF16X3, BF16 = 0, 1, 2
MODES = {"bf16x6": BF16X6, "bf16x3": BF16X3, "bf16": BF16}
DEFAULT = "bf16x6"
ENV = "ERAFT_AMD_PRECISION"
ENCODER_ENV = "ERAFT_AMD_ENCODER_PRECISION"
CORR_ENV = "ERAFT_AMD_CORR_PRECISION"
POINTWISE_ENV = "ERAFT_AMD_POINTWISE_PRECISION"


def code(name) -> int:
    """The CORR_PREC_* value of a mode name; anything else raises ValueError."""
    if not isinstance(name, str) or name not in MODES:
        raise ValueError(f"precision must be one of {sorted(MODES)} (got {name!r})")
    return MODES[name]


def _resolve(config, key_name, env_name) -> str:
    env = os.environ.get(env_name) or None
    if env is not None:
        name = env.lower()
    else:
        key = config.get(key_name, False) if hasattr(config, "get") else False
        if key is None or isinstance(key, bool):
            name = "bf16x3" if key else DEFAULT
        elif isinstance(key, str):
            name = key.lower()
        else:
            raise ValueError(f"{key_name} must be a bool or one of {sorted(MODES)} (got {key!r})")
    code(name)
    return name


def resolve(config=None) -> str:
    """The mode name of a model's GRU and update block: the config key `mixed_precision` (absent or
    False: "bf16x6"; True: "bf16x3"; a string: that mode), overridden by ERAFT_AMD_PRECISION=<name>; a
    variable that is set but empty counts as unset, any other unknown name raises."""
    return _resolve(config, "mixed_precision", ENV)


def resolve_encoder(config=None) -> str:
    """The mode name of a model's two encoders: the config key `encoder_precision` (absent, None or
    False: "bf16x6"; True: "bf16x3"; a string: that mode), overridden by
    ERAFT_AMD_ENCODER_PRECISION=<name>; a variable that is set but empty counts as unset, any other
    unknown name raises.  Independent of `mixed_precision`."""
    return _resolve(config, "encoder_precision", ENCODER_ENV)


def resolve_corr(config=None) -> str:
    """The mode name of a model's correlation build: the config key `corr_precision` (absent, None or
    False: "bf16x6"; True: "bf16x3"; a string: that mode), overridden by
    ERAFT_AMD_CORR_PRECISION=<name>; a variable that is set but empty counts as unset, any other
    unknown name raises.  Independent of `mixed_precision` and `encoder_precision`."""
    return _resolve(config, "corr_precision", CORR_ENV)


def resolve_pointwise(config=None) -> str:
    """The mode name of a model's lookup + convc1 and mask head launches: the config key
    `pointwise_precision` (absent, None or False: "bf16x6"; True: "bf16x3"; a string: that mode),
    overridden by ERAFT_AMD_POINTWISE_PRECISION=<name>; a variable that is set but empty counts as
    unset, any other unknown name raises.  Independent of the other three knobs."""
    return _resolve(config, "pointwise_precision", POINTWISE_ENV)
