"""Helpers of tests/test_corr_precision.py: the correlation build in a precision mode through the raw
C ABI and through eraft_amd._lib, inputs on which every output of the build is ONE exactly
representable piece product (tests/_bf16x6.py's operand classes placed one-hot along D), and the
numpy value each mode must give on them.
"""
import ctypes

import numpy as np
import torch

import _bf16x6 as bx
import _precision as pm

F32, F64 = np.float32, np.float64
DEV = "cuda:0"
REDUCED = ("bf16x3", "bf16")
BF16X6 = 2  # CORR_BUILD_BF16X6
# the issue's shapes [B, D, H, W]: the specialised K loop with NQ = 171 (a second query group whose
# waves lie partly and wholly past NQ, H no multiple of 8, W none of 16), and two generic K loops
SHAPES = {"d256": (2, 256, 9, 19), "d40": (1, 40, 8, 16), "d96": (1, 96, 12, 20)}


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


def levels_for(B, NQ, H, W, L, fill=None):
    from _util import tiled_levels
    return tiled_levels(B, H, W, L, DEV, fill=fill, NQ=NQ)


def build(f1, f2, L, mode, levels=None, fill=None):
    """_lib.build of gpu tensors in `mode` -> the tiled levels."""
    from eraft_amd import _lib
    B, _, H, W = f2.shape
    lv = levels_for(B, f1.shape[2] * f1.shape[3], H, W, L, fill) if levels is None else levels
    _lib.build(f1, f2, lv, _lib.BUILD_BF16X6, precision=pm.CODE[mode])
    return lv


def export(levels, H, W):
    from _util import export_levels
    return export_levels(levels, H, W)


def _ptrs(ts):
    arr = (ctypes.c_void_p * len(ts))()
    for k, t in enumerate(ts):
        arr[k] = t.data_ptr()
    return arr


def raw_build(f1, f2, lv, ws, precision=None):
    """corr_build_ex (precision None) or corr_build_ex_prec straight through ctypes."""
    from eraft_amd import _lib
    lib = _lib.load()
    B, D, H, W = f2.shape
    NQ = f1.shape[2] * f1.shape[3]
    st = torch.cuda.current_stream().cuda_stream
    head = (BF16X6, f1.data_ptr(), NQ, f2.data_ptr(), B, D, H, W, len(lv), _ptrs(lv), ws.data_ptr(), ws.numel())
    rc = lib.corr_build_ex(*head, st) if precision is None else lib.corr_build_ex_prec(*head, precision, st)
    assert rc == 0, lib.corr_last_error().decode()


def raw_region(f1, f2_rows, y0, y1, H, lv, ws, pack_q, precision=None):
    """corr_build_region (precision None) or corr_build_region_prec straight through ctypes."""
    from eraft_amd import _lib
    lib = _lib.load()
    B, D, _, W = f2_rows.shape
    NQ = f1.shape[2] * f1.shape[3]
    st = torch.cuda.current_stream().cuda_stream
    head = (BF16X6, f1.data_ptr(), NQ, f2_rows.data_ptr(), y0, y1, B, D, H, W, len(lv), _ptrs(lv), ws.data_ptr(),
            ws.numel(), 1 if pack_q else 0)
    rc = lib.corr_build_region(*head, st) if precision is None else lib.corr_build_region_prec(*head, precision, st)
    assert rc == 0, lib.corr_last_error().decode()


def inv_sqrt(D):
    """The kernel's scale: 1.0f / sqrtf(D)."""
    return F32(1.0) / np.sqrt(F32(D))


class OneHot:
    """R launches of a [B, D, H, W] build in which one operand (`hot`: "q" queries or "t" targets)
    has ONE non-zero feature per pixel, at k = (pixel + launch shift) % D, and the other is dense.
    Output (q, t) of launch r is then the single product hot[pixel] * dense[k(pixel), other pixel],
    and over shifts 0 .. D - 1 every (query, target, k) position is observed.  Values: an exact
    operand class of tests/_bf16x6.py (the dense operand is the class's `full`)."""

    def __init__(self, cls, shape, hot, shifts, seed):
        B, D, H, W = shape
        N = H * W
        self.shape, self.hot, self.N = shape, hot, N
        self.R = (len(shifts) + B - 1) // B
        sh = np.resize(np.asarray(shifts), self.R * B).reshape(self.R, B)
        full, point = bx.operands(cls, seed, B * D * N, self.R * B * N, spread=10, pspread=6)
        self.dense = full.reshape(B, D, N)
        self.val = point.reshape(self.R, B, N)
        self.k = (np.arange(N)[None, None, :] + sh[:, :, None]) % D          # [R, B, N]
        self.seen = np.zeros((min(N, 128), D), bool)                         # (pixel position in a 128-tile, k)
        for r in range(self.R):
            for b in range(B):
                self.seen[np.arange(N) % 128, self.k[r, b]] = True

    def inputs(self, r):
        """(f1, f2) gpu tensors of launch r."""
        B, D, H, W = self.shape
        hot = np.zeros((B, D, self.N), F32)
        for b in range(B):
            hot[b, self.k[r, b], np.arange(self.N)] = self.val[r, b]
        dense = self.dense
        f1, f2 = (hot, dense) if self.hot == "q" else (dense, hot)
        return gpu(f1.reshape(B, D, H, W)), gpu(f2.reshape(B, D, H, W))

    def pairs(self, r):
        """(target value, query value) arrays [B, N(q), N(t)] of launch r's single products."""
        B = self.shape[0]
        d = np.stack([self.dense[b][self.k[r, b]] for b in range(B)])        # [B, N(hot pixel), N(other)]
        v = np.broadcast_to(self.val[r][:, :, None], d.shape)
        if self.hot == "q":
            return d, v                       # rows = queries already
        return np.swapaxes(v, 1, 2), np.swapaxes(d, 1, 2)

    def expected(self, r, mode):
        """Level 0 [B * N, N] of launch r in `mode`: the mode's value of each single product (the
        kept-piece products, acs then acc, joined), times the kernel's 1 / sqrt(D) in fp32."""
        t, q = self.pairs(r)
        D = self.shape[1]
        return (pm.mode_model(t, q, mode) * inv_sqrt(D)).astype(F32).reshape(-1, self.N)

    def kept_product(self, r, mode):
        """The same outputs from the definition "the product with the dropped pieces removed from
        both operands", exact in fp64 and rounded once."""
        t, q = self.pairs(r)
        D = self.shape[1]
        p = pm.kept(t, mode).astype(F64) * pm.kept(q, mode).astype(F64)
        assert (p.astype(F32).astype(F64) == p).all()
        return (p.astype(F32) * inv_sqrt(D)).astype(F32).reshape(-1, self.N)
