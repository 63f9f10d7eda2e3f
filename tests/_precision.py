"""A numpy model of the reduced precision modes (csrc/corr_bf16x6.h: products<NP>) on tests/_bf16x6.py's
split3, and the fp64 evaluations that the GPU tests of tests/test_precision.py compare with.

A mode keeps the first NP pieces of both operands and multiplies, per K step and in this order,
  bf16x6 (NP = 3)  six()'s products (tests/_bf16x6.py: six_model)
  bf16x3 (NP = 2)  acs += wm xh;  acs += wh xm;  acc += wh xh
  bf16   (NP = 1)  acc += wh xh                                   (the result is acc alone)
"""
import numpy as np
import torch
import torch.nn.functional as F

import _bf16x6 as bx

F32, F64 = np.float32, np.float64
MODES = ("bf16x6", "bf16x3", "bf16")
CODE = {"bf16x6": 0, "bf16x3": 1, "bf16": 2}
KEEP = {"bf16x6": 3, "bf16x3": 2, "bf16": 1}
# (weight piece, activation piece) of each product of a mode, in the kernel's order; the last goes to acc
ORDER = {"bf16x6": ((2, 0), (0, 2), (1, 1), (1, 0), (0, 1), (0, 0)), "bf16x3": ((1, 0), (0, 1), (0, 0)),
         "bf16": ((0, 0),)}
# the operand-rounding coefficient of a mode's a-priori bound: |out - fp64| <= COEF sum |w| |x| + A,
# from |x - hi| <= 2^-9 |x| and |x - hi - mid| <= 2^-18 |x|
COEF = {"bf16x6": 0.0, "bf16x3": 2.0 ** -16, "bf16": 2.0 ** -8 + 2.0 ** -18}


def mode_model(w, x, mode):
    """The kernels' value of the single product w * x (elementwise) in `mode`: every partial sum
    rounded to fp32, acc and acs joined by split_sum (acc alone for bf16)."""
    if mode == "bf16x6":
        return bx.six_model(w, x)
    wp, xp = bx.split3(w), bx.split3(x)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = (wp[0] * xp[0]).astype(F32)
        if mode == "bf16":
            return acc
        acs = (wp[1] * xp[0]).astype(F32)
        acs = (acs + (wp[0] * xp[1]).astype(F32)).astype(F32)
        return np.where(np.isinf(acc), acc, (acc + acs).astype(F32)).astype(F32)


def kept(a, mode):
    """The sum of the pieces of `a` that the mode keeps, as fp32 (exact: at most 24 bits)."""
    p = bx.split3(a)
    out = p[0].astype(F64)
    for q in p[1:KEEP[mode]]:
        out = out + q.astype(F64)
    assert (out.astype(F32).astype(F64) == out).all()
    return out.astype(F32)


def conv64(x, w, mode, padding, bias=None):
    """The mode's definition of a convolution in fp64: the sum of the fp64 convolutions of the
    products among the kept pieces (+ bias).  x [B, C, H, W], w [O, C, kh, kw], fp32 numpy."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    wp, xp = bx.split3(w), bx.split3(x)
    out = None
    for a, b in ORDER[mode]:
        term = F.conv2d(t(xp[b]), t(wp[a]), None, 1, padding)
        out = term if out is None else out + term
    if bias is not None:
        out = out + t(bias).view(1, -1, 1, 1)
    return out.numpy()


def sigmoid64(v):
    return 1.0 / (1.0 + np.exp(-v))
