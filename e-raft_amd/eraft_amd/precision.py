"""The precision modes of the per-iteration kernels (include/corr_mi355x.h: CORR_PREC_*), the
counterpart of the reference's mixed_precision (model/eraft.py:31,102-133).

A mode names the pieces of the exact three-piece bf16 split that the fused GRU half step and the
update block's fused 3x3 convolutions keep of both operands:

  "bf16x6"  hi, mid, lo: six products per fp32 product, no narrower than fp32 (the default)
  "bf16x3"  hi, mid: three products, operands to 2^-18 and the dropped mid x mid to 2^-16 relative
  "bf16"    hi: one product, operands to 2^-9 relative

Accumulation is fp32 in every mode.  The mode acts only where those kernels run (inference with
ERAFT_AMD_FUSE_GRU=1 / ERAFT_AMD_FUSE_UPDATE=1): the torch paths and training stay fp32 and ignore
it, and convf1, the flow head's second convolution, the mask head with the upsampling, the lookup
with convc1 and the encoders stay "bf16x6" by design.
"""
from __future__ import annotations

import os

BF16X6, BF16X3, BF16 = 0, 1, 2
MODES = {"bf16x6": BF16X6, "bf16x3": BF16X3, "bf16": BF16}
DEFAULT = "bf16x6"
ENV = "ERAFT_AMD_PRECISION"


def code(name) -> int:
    """The CORR_PREC_* value of a mode name; anything else raises ValueError."""
    if not isinstance(name, str) or name not in MODES:
        raise ValueError(f"precision must be one of {sorted(MODES)} (got {name!r})")
    return MODES[name]


def resolve(config=None) -> str:
    """The mode name a model runs in: the config key `mixed_precision` (absent or False: "bf16x6";
    True: "bf16x3"; a string: that mode), overridden by ERAFT_AMD_PRECISION=<name>; a variable that is
    set but empty counts as unset, any other unknown name raises."""
    env = os.environ.get(ENV) or None
    if env is not None:
        name = env.lower()
    else:
        key = config.get("mixed_precision", False) if hasattr(config, "get") else False
        if key is None or isinstance(key, bool):
            name = "bf16x3" if key else DEFAULT
        elif isinstance(key, str):
            name = key.lower()
        else:
            raise ValueError(f"mixed_precision must be a bool or one of {sorted(MODES)} (got {key!r})")
    code(name)
    return name
