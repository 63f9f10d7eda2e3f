"""Buffer and stream discipline of the core entry points (include/corr_mi355x.h): the builds, the
lookups and their backward family, the lookup fused with convc1, the on-demand calls, splat,
convex upsampling, the voxel grids and the GRU half step.

The parity tests pin what these kernels compute; this file pins where they read and write and on
which stream they run.  One table of cases (CASES), each calling the raw C-ABI function through
ctypes on the current stream, and four properties checked for every case:

  1. writes stay inside        outputs, in/out buffers and workspaces are windows inside
                               sentinel-filled buffers (tests/_guard.py); the guards survive, every
                               fully written output is fully written, and the results are
                               bit-identical to the plain call into ordinary tensors.
  2. workspaces are honest     a workspace of exactly the bytes its size function returns,
                               prefilled with the sentinel: same results, guards intact.
  3. inputs only               every input is such a window, so NaN lies before and after it:
                               same results, and no result word carries the sentinel's payload;
                               again with the inputs on a 4-byte-only aligned address wherever the
                               header asks for no more.
  4. the caller's stream       the inputs receive their values on a side stream behind a long
                               producer; a launch, memset or reduction pass that went to another
                               stream would see the sentinel instead.

The plain call is what the parity tests pin to the oracle; no reference is recomputed here.
The last test is a ratchet (no GPU): every entry point of the header that takes a stream is in
CASES, forwards to one that is, or is in COVERED_ELSEWHERE, whose owner checks the same four
properties (tests/test_family_discipline.py).
"""
import ctypes
import functools
import os
import re
import sys

import numpy as np
import pytest
import torch

import _guard
import prng
from _util import DEV, _bwd_case, bit_equal, load

FP32, F16X3, BF16X6, EXACT_FOLD = 0, 1, 2, 0x400
ALGOS = {"bf16x6": BF16X6, "f16x3": F16X3, "fp32": FP32}
PRECS = {"bf16x3": 1, "bf16": 2}
HID = 128

# Correlation geometries (B, D, H, W, levels, radius).
#   A: N = 391 is no multiple of 8, 32 or 64; level widths 23, 11, 5 are ragged against the
#      4-cell tile; H is odd; D is no multiple of the MFMA K step; B > 1 shows stride errors.
#   B: fewer queries than one workgroup range (the "empty ranges" case).
#   G: the on-demand sizes that take the general path (tests/test_ondemand.py).
GEO = {"A": (2, 20, 17, 23, 3, 4), "B": (1, 16, 8, 12, 3, 4), "G": (1, 3, 9, 11, 3, 4)}
T = 3  # lookups per case: a regular window field, the integer grid, far taps near 2^20; NaN in each


def _lib():
    from eraft_amd import _lib as m
    return m.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ok(rc):
    assert rc == 0, f"rc {rc}: {_lib().corr_last_error().decode(errors='replace')}"


def _ptrs(ts):
    return (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])


def _gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _poison(t):
    t.view(torch.int32 if t.element_size() == 4 else torch.int64).fill_(
        _guard.SENTINEL if t.element_size() == 4 else _guard.SENTINEL64)
    return t


# ----------------------------------------------------------------------------------------------
# buffers by role
# ----------------------------------------------------------------------------------------------
class Arena:
    """Allocates a case's buffers by role.  With every switch off the buffers are what the parity
    tests use: ordinary tensors (the plain call).  guard_in / guard_out / guard_ws put the inputs /
    the outputs and in/out buffers / the workspaces into guarded windows; misalign moves every
    input whose contract is "4-byte aligned" one float off its 16-byte boundary; defer leaves the
    inputs holding the sentinel and keeps their values in `staged` for the caller to copy in."""

    def __init__(self, guard_in=False, guard_out=False, guard_ws=False, misalign=False, defer=False):
        self.guard_in, self.guard_out, self.guard_ws = guard_in, guard_out, guard_ws
        self.misalign, self.defer = misalign, defer
        self.guards = []   # (name, big, view)
        self.full = []     # (name, view): fully written outputs that sit in a window
        self.staged = []   # (view, values)
        self.fresh = []    # pure outputs and workspaces: no values to keep
        self.n_ws, self.last_ws = 0, None

    def _window(self, name, n, guard, align16=True, dtype=torch.float32):
        if not guard:
            return torch.empty(max(n, 1), dtype=dtype, device=DEV)[:n]
        big, view = _guard.guarded(n, DEV, align16, dtype)
        self.guards.append((name, big, view))
        return view

    def _filled(self, name, values, guard, align16):
        v = self._window(name, values.numel(), guard, align16 or not self.misalign, values.dtype).view(values.shape)
        if self.defer:
            if not guard:
                _poison(v)
            self.staged.append((v, values))
        else:
            v.copy_(values)
        return v

    def inp(self, name, values, align16=False):
        """An input holding `values`.  align16: the header requires 16-byte alignment (levels,
        packs, prepared workspaces); otherwise the contract is fp32, 4-byte aligned."""
        return self._filled(name, values, self.guard_in, align16)

    def inout(self, name, values, align16=False):
        """A buffer the call reads and overwrites or accumulates into."""
        return self._filled(name, values, self.guard_in or self.guard_out, align16)

    def out(self, name, shape, full=True):
        """A pure output.  full: the header says every element is written; otherwise (tiled value
        levels with their padding cells, scratch levels) it starts as the sentinel everywhere, so
        that untouched words compare equal."""
        v = self._window(name, int(np.prod(shape)), self.guard_out).view(shape)
        if full and self.guard_out:
            self.full.append((name, v))
        if not full and not self.guard_out:
            _poison(v)
        self.fresh.append(v)
        return v

    def ws(self, name, nbytes, full=False):
        """(pointer, bytes) of a workspace of exactly `nbytes` (the size function's answer): ceil(bytes / 4)
        floats, 256-byte aligned, holding the sentinel; the tensor itself is `last_ws`.  full: the
        header documents the layout and every word of it is written (a workspace that is an output)."""
        assert nbytes != ctypes.c_size_t(-1).value, f"{name}: the size function refused the sizes"
        self.n_ws += 1
        if nbytes == 0:
            return None, 0
        v = self.last_ws = self._window(name, (nbytes + 3) // 4, self.guard_ws)
        if not self.guard_ws:
            _poison(v)
        elif full:
            self.full.append((name, v))
        self.fresh.append(v)
        assert v.data_ptr() % 256 == 0
        return v.data_ptr(), nbytes

    def check(self):
        for name, big, view in self.guards:
            _guard.check_guards(big, view, name)
        for name, view in self.full:
            _guard.check_written(view, name)


# ----------------------------------------------------------------------------------------------
# shared data: built once on the default stream, read-only by convention
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _fmaps(geo):
    B, D, H, W, _, _ = GEO[geo]
    return _gpu(prng.gauss(61, (B, D, H, W))), _gpu(prng.gauss(62, (B, D, H, W)))


@functools.lru_cache(maxsize=None)
def _lookups(geo):
    """_bwd_case's coords and upstream gradients: ([B, 2, H, W]) * T, ([B, L*K, H, W]) * T."""
    B, _, H, W, L, r = GEO[geo]
    return _bwd_case(T, B, H, W, L, r, 700)


def _map_floats(h, w):
    return ((h + 3) // 4) * ((w + 3) // 4) * 16


def _level_shapes(geo, tiled):
    B, _, H, W, L, _ = GEO[geo]
    return [(B * H * W, _map_floats(H >> l, W >> l) if tiled else (H >> l) * (W >> l)) for l in range(L)]


@functools.lru_cache(maxsize=None)
def _pyramid(geo):
    """The value pyramid of a bf16x6 build into sentinel-prefilled tiled levels: a tile's padding
    cells past W_l / H_l are poison unless the build wrote them."""
    B, D, H, W, L, _ = GEO[geo]
    lib = _lib()
    f1, f2 = _fmaps(geo)
    lv = [_poison(torch.empty(s, device=DEV)) for s in _level_shapes(geo, True)]
    n = lib.corr_build_workspace(BF16X6, B, D, H * W, H, W)
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    _ok(lib.corr_build_ex(BF16X6, f1.data_ptr(), H * W, f2.data_ptr(), B, D, H, W, L, _ptrs(lv), ws.data_ptr(), n,
                          _stream()))
    torch.cuda.synchronize()
    return lv


@functools.lru_cache(maxsize=None)
def _grad_pyramid(geo):
    """Random gradient levels [B*N, H_l*W_l] (row-major, the reference's layout)."""
    return [_gpu(prng.gauss(300 + l, s)) for l, s in enumerate(_level_shapes(geo, False))]


@functools.lru_cache(maxsize=None)
def _convc1(geo):
    """convc1's weight [256, L*K], its pack, its bias, the fused forward's outputs for the T lookups
    and upstream gradients [B, 256, H, W]."""
    B, _, H, W, L, r = GEO[geo]
    C = L * (2 * r + 1) ** 2
    lib = _lib()
    w, bias = _gpu(prng.gauss(134, (256, C), 0.05)), _gpu(prng.gauss(135, (256,), 0.1))
    n = lib.corr_lookup_conv_weights_bytes()
    pack = torch.empty((n + 3) // 4, device=DEV)
    _ok(lib.corr_lookup_conv_weights(w.data_ptr(), 256, C, pack.data_ptr(), _stream()))
    outs = []
    for c in _lookups(geo)[0]:
        o = torch.empty(B, 256, H, W, device=DEV)
        _ok(lib.corr_lookup_conv(_ptrs(_pyramid(geo)), c.data_ptr(), B, H, W, L, r, pack.data_ptr(), bias.data_ptr(), 1,
                                 o.data_ptr(), _stream()))
        outs.append(o)
    gs = [_gpu(prng.gauss(136 + t, (B, 256, H, W))) for t in range(T)]
    torch.cuda.synchronize()
    return w, pack, bias, outs, gs


@functools.lru_cache(maxsize=None)
def _prepared(geo):
    """corr_ondemand_prepare's workspace (float32 words)."""
    B, D, H, W, L, _ = GEO[geo]
    lib = _lib()
    f1, f2 = _fmaps(geo)
    n = lib.corr_ondemand_workspace(B, D, H, W, L)
    assert n
    ws = torch.empty((n + 3) // 4, device=DEV)
    _ok(lib.corr_ondemand_prepare(f1.data_ptr(), f2.data_ptr(), B, D, H, W, L, ws.data_ptr(), n, _stream()))
    torch.cuda.synchronize()
    return ws


@functools.lru_cache(maxsize=None)
def _gru_data(B, H, W, inp, d):
    tag = "1" if d == 0 else "2"
    C = HID + inp
    shape = (HID, C, 1, 5) if d == 0 else (HID, C, 5, 1)
    ws = [_gpu(prng.param_init(f"conv{g}{tag}.weight", shape).reshape(HID, C, 5)) for g in "zrq"]
    bs = [_gpu(prng.param_init(f"conv{g}{tag}.bias", (HID,))) for g in "zrq"]
    h = _gpu(np.tanh(prng.gauss(7, (B, HID, H, W)).astype(np.float64)).astype(np.float32))
    x = _gpu(prng.gauss(8, (B, inp, H, W)))
    lib = _lib()
    n = lib.corr_gru_weights_bytes(HID, inp)
    assert n
    pack = torch.empty((n + 3) // 4, device=DEV)
    _ok(lib.corr_gru_pack_weights(*(w.data_ptr() for w in ws), HID, inp, pack.data_ptr(), _stream()))
    torch.cuda.synchronize()
    return ws, bs, h, x, pack


def _export(levels, geo):
    """The tiled levels in the reference's layout (corr_pyramid_export on the current stream)."""
    B, _, H, W, L, _ = GEO[geo]
    outs = [torch.empty(s, device=DEV) for s in _level_shapes(geo, False)]
    _ok(_lib().corr_pyramid_export(_ptrs(levels), B * H * W, H, W, L, _ptrs(outs), _stream()))
    return {f"pyr{l}": o for l, o in enumerate(outs)}


def _clones(**ts):
    return lambda: {k: v.clone() for k, v in ts.items()}


# ----------------------------------------------------------------------------------------------
# the cases: case(A) allocates through the arena A and returns (call, collect); call() enqueues the
# entry point on the current stream, collect() returns new tensors holding the results
# ----------------------------------------------------------------------------------------------
def case_build_ex(A, geo, algo):
    B, D, H, W, L, _ = GEO[geo]
    lib = _lib()
    f1, f2 = (A.inp(n, v) for n, v in zip(("fmap1", "fmap2"), _fmaps(geo)))
    lv = [A.out(f"pyr{l}", s, full=False) for l, s in enumerate(_level_shapes(geo, True))]
    wp, wn = A.ws("workspace", lib.corr_build_workspace(algo, B, D, H * W, H, W))

    def call():
        _ok(lib.corr_build_ex(algo, f1.data_ptr(), H * W, f2.data_ptr(), B, D, H, W, L, _ptrs(lv), wp, wn, _stream()))
    return call, lambda: _export(lv, geo)


def case_build_region(A, geo):
    """A partition of the target rows into regions of 8: together the whole pyramid."""
    B, D, H, W, L, _ = GEO[geo]
    lib = _lib()
    f1v, f2v = _fmaps(geo)
    f1 = A.inp("fmap1", f1v)
    regions = [(y0, min(y0 + 8, H)) for y0 in range(0, H, 8)]
    slabs = [A.inp(f"fmap2_rows{k}", f2v[:, :, y0:y1].contiguous()) for k, (y0, y1) in enumerate(regions)]
    lv = [A.out(f"pyr{l}", s, full=False) for l, s in enumerate(_level_shapes(geo, True))]
    wp, wn = A.ws("workspace", lib.corr_build_workspace(BF16X6, B, D, H * W, H, W))

    def call():
        for k, (y0, y1) in enumerate(regions):
            _ok(lib.corr_build_region(BF16X6, f1.data_ptr(), H * W, slabs[k].data_ptr(), y0, y1, B, D, H, W, L, _ptrs(lv),
                                      wp, wn, 1 if k == 0 else 0, _stream()))
    return call, lambda: _export(lv, geo)


def _pyr_in(A, geo):
    return [A.inp(f"pyr{l}", v, align16=True) for l, v in enumerate(_pyramid(geo))]


def _lookups_in(A, geo, grads=True):
    cs, gs = _lookups(geo)
    cs = [A.inp(f"coords{t}", c) for t, c in enumerate(cs)]
    return cs, [A.inp(f"grad_out{t}", g) for t, g in enumerate(gs)] if grads else None


def case_lookup_rows(A, geo):
    B, _, H, W, L, r = GEO[geo]
    lib = _lib()
    lv = _pyr_in(A, geo)
    cs, _ = _lookups_in(A, geo, grads=False)
    outs = [A.out(f"out{t}", (B, L * (2 * r + 1) ** 2, H, W)) for t in range(T)]

    def call():
        for c, o in zip(cs, outs):
            _ok(lib.corr_lookup_rows(_ptrs(lv), c.data_ptr(), B, H * W, H, W, L, r, o.data_ptr(), _stream()))
    return call, _clones(**{f"out{t}": o for t, o in enumerate(outs)})


def _grad_levels_inout(A, geo):
    return [A.inout(f"grad_pyr{l}", v) for l, v in enumerate(_grad_pyramid(geo))]


def _grad_levels_result(gl):
    return _clones(**{f"grad_pyr{l}": g for l, g in enumerate(gl)})


def case_lookup_bwd_rows(A, geo):
    """Accumulates the T lookups, in order, into a gradient pyramid that already holds values."""
    B, _, H, W, L, r = GEO[geo]
    lib = _lib()
    cs, gs = _lookups_in(A, geo)
    gl = _grad_levels_inout(A, geo)

    def call():
        for c, g in zip(cs, gs):
            _ok(lib.corr_lookup_bwd_rows(c.data_ptr(), g.data_ptr(), B, H * W, H, W, L, r, _ptrs(gl), _stream()))
    return call, _grad_levels_result(gl)


def case_lookup_bwd_multi(A, geo):
    B, _, H, W, L, r = GEO[geo]
    lib = _lib()
    cs, gs = _lookups_in(A, geo)
    gl = [A.out(f"grad_pyr{l}", s) for l, s in enumerate(_level_shapes(geo, False))]

    def call():
        _ok(lib.corr_lookup_bwd_multi(_ptrs(cs), _ptrs(gs), T, B, H * W, H, W, L, r, _ptrs(gl), _stream()))
    return call, _grad_levels_result(gl)


def case_pool_bwd(A, geo):
    B, _, H, W, L, _ = GEO[geo]
    lib = _lib()
    gl = _grad_levels_inout(A, geo)

    def call():
        _ok(lib.corr_pool_bwd(_ptrs(gl), B * H * W, H, W, L, _stream()))
    return call, _grad_levels_result(gl)


def case_pool_fold(A, geo):
    """Only level 0 is the result (the coarser levels are read)."""
    B, _, H, W, L, _ = GEO[geo]
    lib = _lib()
    gl = _grad_levels_inout(A, geo)

    def call():
        _ok(lib.corr_pool_fold(_ptrs(gl), B, H * W, H, W, L, _stream()))
    return call, _clones(grad_pyr0=gl[0])


def case_build_bwd_ex(A, geo, algo):
    B, D, H, W, _, _ = GEO[geo]
    lib = _lib()
    gc = A.inp("grad_c", _grad_pyramid(geo)[0])
    f1, f2 = (A.inp(n, v) for n, v in zip(("fmap1", "fmap2"), _fmaps(geo)))
    d1, d2 = A.out("dfmap1", (B, D, H, W)), A.out("dfmap2", (B, D, H, W))
    wp, wn = A.ws("workspace", lib.corr_build_bwd_ex_workspace(algo, B, D, H * W, H, W))

    def call():
        _ok(lib.corr_build_bwd_ex(algo, gc.data_ptr(), f1.data_ptr(), H * W, f2.data_ptr(), B, D, H, W, d1.data_ptr(),
                                  d2.data_ptr(), wp, wn, _stream()))
    return call, _clones(dfmap1=d1, dfmap2=d2)


def case_backward(A, geo, algo, exact):
    """grad_pyr is scratch: level 0 ends as dC (a result), the coarser levels are not results."""
    B, D, H, W, L, r = GEO[geo]
    lib = _lib()
    cs, gs = _lookups_in(A, geo)
    f1, f2 = (A.inp(n, v) for n, v in zip(("fmap1", "fmap2"), _fmaps(geo)))
    gl = [A.out(f"grad_pyr{l}", s, full=l == 0) for l, s in enumerate(_level_shapes(geo, False))]
    d1, d2 = A.out("dfmap1", (B, D, H, W)), A.out("dfmap2", (B, D, H, W))
    wp, wn = A.ws("workspace", lib.corr_backward_workspace(algo, B, D, H * W, H, W, r))
    flag = EXACT_FOLD if exact else 0

    def call():
        _ok(lib.corr_backward(algo | flag, _ptrs(cs), _ptrs(gs), T, f1.data_ptr(), H * W, f2.data_ptr(), B, D, H, W, L,
                              r, _ptrs(gl), d1.data_ptr(), d2.data_ptr(), wp, wn, _stream()))
    return call, _clones(dC=gl[0], dfmap1=d1, dfmap2=d2)


def case_lookup_conv_weights(A, geo):
    _, _, _, _, L, r = GEO[geo]
    lib = _lib()
    w = A.inp("weight", _convc1(geo)[0])
    n = lib.corr_lookup_conv_weights_bytes()
    pack = A.out("packed", ((n + 3) // 4,))

    def call():
        _ok(lib.corr_lookup_conv_weights(w.data_ptr(), 256, L * (2 * r + 1) ** 2, pack.data_ptr(), _stream()))
    return call, _clones(packed=pack)


def case_lookup_conv(A, geo):
    B, _, H, W, L, r = GEO[geo]
    lib = _lib()
    lv = _pyr_in(A, geo)
    cs, _ = _lookups_in(A, geo, grads=False)
    _, pack, bias, _, _ = _convc1(geo)
    pack, bias = A.inp("packed", pack, align16=True), A.inp("bias", bias)
    outs = [A.out(f"out{t}", (B, 256, H, W)) for t in range(T)]

    def call():
        for c, o in zip(cs, outs):
            _ok(lib.corr_lookup_conv(_ptrs(lv), c.data_ptr(), B, H, W, L, r, pack.data_ptr(), bias.data_ptr(), 1,
                                     o.data_ptr(), _stream()))
    return call, _clones(**{f"out{t}": o for t, o in enumerate(outs)})


def case_lookup_conv_bwd(A, geo):
    """All three gradients, for each of the T lookups; with ReLU, so `out` is read.  The entry point
    asks for 16-byte aligned out / grad_out when H*W is a multiple of 4 (it takes 16-byte loads)."""
    B, _, H, W, L, r = GEO[geo]
    C = L * (2 * r + 1) ** 2
    lib = _lib()
    lv = _pyr_in(A, geo)
    cs, _ = _lookups_in(A, geo, grads=False)
    _, pack, _, fwd, gs = _convc1(geo)
    pack = A.inp("packed", pack, align16=True)
    vec = (H * W) % 4 == 0
    fwd = [A.inp(f"out{t}", o, align16=vec) for t, o in enumerate(fwd)]
    gs = [A.inp(f"grad_out{t}", g, align16=vec) for t, g in enumerate(gs)]
    dW = [A.out(f"grad_weight{t}", (256, C)) for t in range(T)]
    db = [A.out(f"grad_bias{t}", (256,)) for t in range(T)]
    dl = [A.out(f"grad_lookup{t}", (B, C, H, W)) for t in range(T)]
    wp, wn = A.ws("workspace", lib.corr_lookup_conv_bwd_workspace(B, H, W, L))

    def call():
        for t in range(T):
            _ok(lib.corr_lookup_conv_bwd(_ptrs(lv), cs[t].data_ptr(), B, H, W, L, r, pack.data_ptr(), fwd[t].data_ptr(), 1,
                                         gs[t].data_ptr(), dW[t].data_ptr(), db[t].data_ptr(), dl[t].data_ptr(), wp, wn,
                                         _stream()))
    res = {f"grad_weight{t}": v for t, v in enumerate(dW)}
    res.update({f"grad_bias{t}": v for t, v in enumerate(db)})
    res.update({f"grad_lookup{t}": v for t, v in enumerate(dl)})
    return call, _clones(**res)


def case_ondemand_prepare(A, geo):
    """The workspace is the output: compared word for word, and through the lookup made from it."""
    B, D, H, W, L, r = GEO[geo]
    lib = _lib()
    f1, f2 = (A.inp(n, v) for n, v in zip(("fmap1", "fmap2"), _fmaps(geo)))
    c = A.inp("coords", _lookups(geo)[0][0])
    n = lib.corr_ondemand_workspace(B, D, H, W, L)
    assert n and n % 4 == 0
    wp, wn = A.ws("workspace", n, full=True)
    ws = A.last_ws
    out = A.out("out", (B, L * (2 * r + 1) ** 2, H, W))

    def call():
        _ok(lib.corr_ondemand_prepare(f1.data_ptr(), f2.data_ptr(), B, D, H, W, L, wp, wn, _stream()))
        _ok(lib.corr_ondemand_lookup(wp, c.data_ptr(), B, D, H, W, L, r, 0, out.data_ptr(), _stream()))
    return call, _clones(workspace=ws, out=out)


def case_ondemand_lookup(A, geo):
    B, D, H, W, L, r = GEO[geo]
    lib = _lib()
    ws = A.inp("workspace", _prepared(geo), align16=True)
    cs, _ = _lookups_in(A, geo, grads=False)
    outs = [A.out(f"out{t}", (B, L * (2 * r + 1) ** 2, H, W)) for t in range(T)]

    def call():
        for c, o in zip(cs, outs):
            _ok(lib.corr_ondemand_lookup(ws.data_ptr(), c.data_ptr(), B, D, H, W, L, r, 0, o.data_ptr(), _stream()))
    return call, _clones(**{f"out{t}": o for t, o in enumerate(outs)})


def case_ondemand_backward(A, geo):
    B, D, H, W, L, r = GEO[geo]
    lib = _lib()
    ws = A.inp("fwd_workspace", _prepared(geo), align16=True)
    cs, gs = _lookups_in(A, geo)
    d1, d2 = A.out("dfmap1", (B, D, H, W)), A.out("dfmap2", (B, D, H, W))
    wp, wn = A.ws("bwd_workspace", lib.corr_ondemand_bwd_workspace(B, D, H, W, L, r))
    assert wn

    def call():
        _ok(lib.corr_ondemand_backward(ws.data_ptr(), _ptrs(cs), _ptrs(gs), T, B, D, H, W, L, r, wp, wn, d1.data_ptr(),
                                       d2.data_ptr(), _stream()))
    return call, _clones(dfmap1=d1, dfmap2=d2)


@functools.lru_cache(maxsize=None)
def _splat_flow(B, H, W, sigma):
    """test_forward_splat_bitexact_vs_oracle's flow: most targets outside the map, integers, NaN."""
    f = prng.gauss(41, (B, 2, H, W), sigma)
    f[:, :, ::3, ::2] = np.round(f[:, :, ::3, ::2])
    f[0, :, 0, :2] = np.float32(np.nan)
    return _gpu(f)


def case_forward_splat(A, B, H, W, sigma):
    lib = _lib()
    flow = A.inp("flow", _splat_flow(B, H, W, sigma))
    out = A.out("out", (B, 2, H, W))
    wp, wn = A.ws("workspace", lib.corr_forward_splat_workspace(B, H, W))

    def call():
        _ok(lib.corr_forward_splat(flow.data_ptr(), B, H, W, out.data_ptr(), wp, wn, _stream()))
    return call, _clones(out=out)


@functools.lru_cache(maxsize=None)
def _upsample_data(N, h, w, scale):
    return (_gpu(prng.gauss(51, (N, 2, h, w), 3.0)), _gpu(prng.gauss(52, (N, 576, h, w), float(scale))),
            _gpu(prng.gauss(53, (N, 2, 8 * h, 8 * w))))


def case_convex_upsample(A, N, h, w, scale):
    lib = _lib()
    flow, mask, _ = _upsample_data(N, h, w, scale)
    flow, mask = A.inp("flow", flow), A.inp("mask", mask)
    out = A.out("out", (N, 2, 8 * h, 8 * w))

    def call():
        _ok(lib.corr_convex_upsample(flow.data_ptr(), mask.data_ptr(), N, h, w, out.data_ptr(), _stream()))
    return call, _clones(out=out)


def case_convex_upsample_bwd(A, N, h, w, scale):
    lib = _lib()
    flow, mask, g = (A.inp(n, v) for n, v in zip(("flow", "mask", "grad_out"), _upsample_data(N, h, w, scale)))
    dflow, dmask = A.out("dflow", (N, 2, h, w)), A.out("dmask", (N, 576, h, w))
    wp, wn = A.ws("workspace", lib.corr_convex_upsample_bwd_workspace(N, h, w))

    def call():
        _ok(lib.corr_convex_upsample_bwd(flow.data_ptr(), mask.data_ptr(), g.data_ptr(), N, h, w, dflow.data_ptr(),
                                         dmask.data_ptr(), wp, wn, _stream()))
    return call, _clones(dflow=dflow, dmask=dmask)


@functools.lru_cache(maxsize=None)
def _voxel_events(kind, tag):
    """Events and (C, H, W) of a case of tests/golden/g_voxel_edges.npz; tag None: no events."""
    g = load("g_voxel_edges")
    if tag is None:
        any_tag = next(k for k in g if k.startswith(f"{kind}_meta_"))
        return None, tuple(int(v) for v in g[any_tag][1:])
    return _gpu(g[f"{kind}_ev_{tag}"]), tuple(int(v) for v in g[f"{kind}_meta_{tag}"][1:])


def case_voxel_grid(A, tag, normalize):
    lib = _lib()
    ev, (C, H, W) = _voxel_events("d", tag)
    M = 0 if ev is None else ev.shape[1]
    rows = [None] * 4 if ev is None else [A.inp(n, ev[k].contiguous()) for k, n in enumerate("xytp")]
    out = A.out("out", (C, H, W))
    wp, wn = A.ws("workspace", lib.corr_voxel_grid_workspace(M, C, H, W))

    def call():
        _ok(lib.corr_voxel_grid(*(None if v is None else v.data_ptr() for v in rows), M, C, H, W, normalize, out.data_ptr(),
                                wp, wn, _stream()))
    return call, _clones(out=out)


def case_voxel_grid_tbilinear(A, tag, normalize):
    """events are float64 rows: 8-byte aligned is the contract."""
    lib = _lib()
    ev, (C, H, W) = _voxel_events("m", tag)
    M = 0 if ev is None else ev.shape[0]
    events = None if ev is None else A.inp("events", ev)
    out = A.out("out", (C, H, W))
    wp, wn = A.ws("workspace", lib.corr_voxel_grid_tbilinear_workspace(M, C, H, W))

    def call():
        _ok(lib.corr_voxel_grid_tbilinear(None if events is None else events.data_ptr(), M, C, H, W, normalize,
                                          out.data_ptr(), wp, wn, _stream()))
    return call, _clones(out=out)


def case_gru_pack_weights(A, inp, d):
    lib = _lib()
    ws = [A.inp(n, v) for n, v in zip(("wz", "wr", "wq"), _gru_data(1, 1, 1, inp, d)[0])]
    n = lib.corr_gru_weights_bytes(HID, inp)
    assert n and n % 4 == 0
    pack = A.out("packed", (n // 4,))

    def call():
        _ok(lib.corr_gru_pack_weights(*(w.data_ptr() for w in ws), HID, inp, pack.data_ptr(), _stream()))
    return call, _clones(packed=pack)


def case_gru_half_step(A, B, H, W, inp, d, precision=None):
    """precision None: corr_gru_half_step; otherwise corr_gru_half_step_prec in that mode."""
    lib = _lib()
    _, bs, h, x, pack = _gru_data(B, H, W, inp, d)
    h, x, pack = A.inp("h", h), A.inp("x", x), A.inp("packed", pack, align16=True)
    bs = [A.inp(n, v) for n, v in zip(("bz", "br", "bq"), bs)]
    out = A.out("h_out", (B, HID, H, W))
    wp, wn = A.ws("workspace", lib.corr_gru_workspace(B, HID, H, W))

    def call():
        args = (h.data_ptr(), x.data_ptr(), B, HID, inp, H, W, d, pack.data_ptr(), *(b.data_ptr() for b in bs), wp, wn,
                out.data_ptr())
        if precision is None:
            _ok(lib.corr_gru_half_step(*args, _stream()))
        else:
            _ok(lib.corr_gru_half_step_prec(*args, precision, _stream()))
    return call, _clones(h_out=out)


# ----------------------------------------------------------------------------------------------
# the table: id -> (entry point, case)
# ----------------------------------------------------------------------------------------------
def _table():
    t = {}

    def add(entry, label, fn, *args, **kw):
        name = f"{entry}[{label}]"
        assert name not in t, name
        t[name] = (entry, functools.partial(fn, *args, **kw))

    for geo in "AB":
        for an, a in ALGOS.items():
            add("corr_build_ex", f"{geo}-{an}", case_build_ex, geo=geo, algo=a)
            add("corr_build_bwd_ex", f"{geo}-{an}", case_build_bwd_ex, geo=geo, algo=a)
        add("corr_build_region", geo, case_build_region, geo=geo)
        add("corr_lookup_rows", geo, case_lookup_rows, geo=geo)
        add("corr_lookup_bwd_rows", geo, case_lookup_bwd_rows, geo=geo)
        add("corr_lookup_bwd_multi", geo, case_lookup_bwd_multi, geo=geo)
        add("corr_pool_bwd", geo, case_pool_bwd, geo=geo)
        add("corr_pool_fold", geo, case_pool_fold, geo=geo)
        add("corr_backward", f"{geo}-bf16x6-exact", case_backward, geo=geo, algo=BF16X6, exact=True)
        add("corr_backward", f"{geo}-bf16x6", case_backward, geo=geo, algo=BF16X6, exact=False)
        add("corr_backward", f"{geo}-f16x3", case_backward, geo=geo, algo=F16X3, exact=False)
        add("corr_backward", f"{geo}-fp32", case_backward, geo=geo, algo=FP32, exact=False)
        add("corr_lookup_conv_weights", geo, case_lookup_conv_weights, geo=geo)
        add("corr_lookup_conv", geo, case_lookup_conv, geo=geo)
        add("corr_lookup_conv_bwd", geo, case_lookup_conv_bwd, geo=geo)
    for geo in "AG":
        add("corr_ondemand_prepare", geo, case_ondemand_prepare, geo=geo)
        add("corr_ondemand_lookup", geo, case_ondemand_lookup, geo=geo)
        add("corr_ondemand_backward", geo, case_ondemand_backward, geo=geo)
    add("corr_forward_splat", "2x7x5-sigma30", case_forward_splat, B=2, H=7, W=5, sigma=30.0)
    for N, h, w in ((2, 7, 9), (1, 1, 1)):
        for scale in (1, 30):
            add("corr_convex_upsample", f"{N}x{h}x{w}-scale{scale}", case_convex_upsample, N=N, h=h, w=w, scale=scale)
            add("corr_convex_upsample_bwd", f"{N}x{h}x{w}-scale{scale}", case_convex_upsample_bwd, N=N, h=h, w=w,
                scale=scale)
    for normalize in (0, 1):
        for tag in ("nan_coords", "outside", None):
            add("corr_voxel_grid", f"{tag or 'empty'}-norm{normalize}", case_voxel_grid, tag=tag, normalize=normalize)
        for tag in ("wrap", None):
            add("corr_voxel_grid_tbilinear", f"{tag or 'empty'}-norm{normalize}", case_voxel_grid_tbilinear, tag=tag,
                normalize=normalize)
    for d in (0, 1):
        add("corr_gru_pack_weights", f"dir{d}", case_gru_pack_weights, inp=320, d=d)
        for B, H, W in ((2, 7, 9), (1, 1, 1)):
            add("corr_gru_half_step", f"{B}x{H}x{W}-dir{d}", case_gru_half_step, B=B, H=H, W=W, inp=320, d=d)
            for pn, p in PRECS.items():
                add("corr_gru_half_step_prec", f"{B}x{H}x{W}-dir{d}-{pn}", case_gru_half_step, B=B, H=H, W=W, inp=320,
                    d=d, precision=p)
    return t


CASES = _table()
IDS = list(CASES)


def _run_case(case, arena):
    call, collect = case(arena)
    call()
    res = collect()
    torch.cuda.synchronize()
    return res


def _run(name, arena):
    return _run_case(CASES[name][1], arena)


_PLAIN = {}


def _plain(name):
    """The same call made the ordinary way (plain tensors, the default stream); made once."""
    if name not in _PLAIN:
        _PLAIN[name] = {k: v.cpu() for k, v in _run(name, Arena()).items()}
    return _PLAIN[name]


def _same(ref, got, name, clean=False):
    """The results `got` are bit-identical to those of the plain call, `ref`."""
    assert sorted(got) == sorted(ref)
    for k, v in got.items():
        if clean:
            _guard.check_clean(v, k)
        a, b = v.cpu(), ref[k]
        assert bit_equal(a.numpy(), b.numpy()), f"{name}: {k} differs from the plain call"
        if k == "packed":  # bf16 pieces, not floats: every bit counts
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{name}: {k} differs from the plain call"


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    _lib()


# ----------------------------------------------------------------------------------------------
# the four properties
# ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_writes_stay_inside(gpu, name):
    """Property 1: every output, in/out buffer and workspace in a guarded window."""
    arena = Arena(guard_out=True, guard_ws=True)
    got = _run(name, arena)
    arena.check()
    _same(_plain(name), got, name)


def _has_workspace(name):
    """Whether the case asks for a workspace: known from its size-function calls alone, so the
    table is walked without a GPU call (the entry points that take one, by the header)."""
    return CASES[name][0] in WORKSPACE_ENTRIES


WORKSPACE_ENTRIES = {
    "corr_build_ex": "corr_build_workspace", "corr_build_region": "corr_build_workspace",
    "corr_build_bwd_ex": "corr_build_bwd_ex_workspace", "corr_backward": "corr_backward_workspace",
    "corr_lookup_conv_bwd": "corr_lookup_conv_bwd_workspace", "corr_ondemand_prepare": "corr_ondemand_workspace",
    "corr_ondemand_backward": "corr_ondemand_bwd_workspace", "corr_forward_splat": "corr_forward_splat_workspace",
    "corr_convex_upsample_bwd": "corr_convex_upsample_bwd_workspace", "corr_voxel_grid": "corr_voxel_grid_workspace",
    "corr_voxel_grid_tbilinear": "corr_voxel_grid_tbilinear_workspace", "corr_gru_half_step": "corr_gru_workspace",
    "corr_gru_half_step_prec": "corr_gru_workspace",
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", [n for n in IDS if _has_workspace(n)])
def test_workspace_is_as_large_as_claimed_and_needs_no_initialisation(gpu, name):
    """Property 2: the workspace is exactly the size function's bytes, in a guarded window, holding
    the sentinel.  (corr_ondemand_prepare: the lookup made from it is among the results.)"""
    arena = Arena(guard_ws=True)
    got = _run(name, arena)
    assert arena.n_ws >= 1
    arena.check()
    _same(_plain(name), got, name)


@pytest.mark.gpu
@pytest.mark.parametrize("misalign", [False, True], ids=["aligned16", "aligned4"])
@pytest.mark.parametrize("name", IDS)
def test_results_do_not_depend_on_memory_outside_the_inputs(gpu, name, misalign):
    """Property 3: NaN before and after every input; again with the 4-byte-aligned inputs one float
    off their 16-byte boundary."""
    arena = Arena(guard_in=True, misalign=misalign)
    got = _run(name, arena)
    arena.check()
    _same(_plain(name), got, name, clean=True)


# The producer that holds the side stream while the case is enqueued behind it: CHAIN dependent
# fp32 matmuls of PRODUCER_N x PRODUCER_N into two preallocated buffers (no allocation, so nothing
# in it can wait for the device).  The control leg (a clone of the first input, queued on the
# default stream after everything else) must still see the sentinel, i.e. the producer must
# outlast the host's enqueueing of the whole case.
# Measured on an MI355X with events (test_the_producer_outlasts_the_enqueue prints both): the
# chain of 48 takes 44.3 ms; the longest enqueue behind it (the case's copies, calls and clones) takes
# 1.17 ms of host time, a margin of 38; that test asserts a margin of 4.  (The longest cases of
# tests/test_family_discipline.py, which uses this producer too, take 1.00 and 0.96 ms.)
PRODUCER_N = 4096
CHAIN = 48


@functools.lru_cache(maxsize=None)
def _producer_buffers():
    a = torch.randn(PRODUCER_N, PRODUCER_N, device=DEV) / PRODUCER_N ** 0.5
    b, c = torch.empty_like(a), torch.empty_like(a)
    torch.mm(a, a, out=b)  # the first call's setup is not part of any measurement
    torch.cuda.synchronize()
    return a, b, c


def _produce():
    a, b, c = _producer_buffers()
    torch.mm(a, a, out=b)
    for _ in range(CHAIN - 1):
        torch.mm(b, a, out=c)
        b, c = c, b


def _control_holds(stream):
    """Whether work on the default stream overtakes work queued earlier on `stream`: a probe that
    receives its values behind the producer is read at once from the default stream."""
    probe = _poison(torch.empty(1024, device=DEV))
    values = torch.zeros(1024, device=DEV)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        _produce()
        probe.copy_(values)
    early = probe.clone()
    stream.synchronize()
    torch.cuda.synchronize()
    return bool((_guard._bits(early) == _guard.SENTINEL).all()) and not bool(probe.any())


@pytest.fixture(scope="module")
def side(gpu):
    """The side stream of property 4.  Streams share a small number of hardware queues, and a
    stream that shares the default stream's queue is served in order with it: nothing could
    overtake, so neither the control leg nor a mis-streamed launch would show.  Take the first
    stream on which the control holds."""
    _producer_buffers()
    with torch.cuda.stream(torch.cuda.Stream()):
        _produce()  # per-stream setup of the matmul, outside any measurement
    torch.cuda.synchronize()
    tried = []
    for _ in range(8):
        s = torch.cuda.Stream()
        tried.append(s)
        if _control_holds(s):
            return s
    pytest.fail("no side stream runs beside the default stream: the stream test can prove nothing")


def _ordered_on_the_callers_stream(case, ref, side, what):
    """Property 4 for one case: the inputs hold the sentinel until copies on the side stream, behind
    the producer, give them their values, and the outputs and workspaces are filled with the
    sentinel once more there; the case follows on that stream.  Work issued to any other stream
    runs at once: it reads the sentinel, and what it writes is overwritten.  Either way a wrong
    value, never a fault: every access stays inside live buffers."""
    arena = Arena(guard_in=True, guard_out=True, guard_ws=True, defer=True)
    call, collect = case(arena)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        _produce()
        for view, values in arena.staged:
            view.copy_(values)
        for view in arena.fresh:  # a memset or a store that ran ahead of the stream is undone here
            _poison(view)
        call()
        got = collect()
    early = arena.staged[0][0].clone() if arena.staged else None   # the control leg, on the default stream
    side.synchronize()
    torch.cuda.synchronize()
    if early is not None:
        assert bool((_guard._bits(early) == _guard._sentinel(early)).all()), \
            "the control read saw the inputs' values: the producer is too short to prove anything"
    arena.check()
    _same(ref, got, what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_work_is_ordered_on_the_callers_stream(gpu, side, name):
    """Property 4 (see _ordered_on_the_callers_stream)."""
    ref = _plain(name)  # also loads every kernel of the case, so that the enqueue only enqueues
    _ordered_on_the_callers_stream(CASES[name][1], ref, side, name)


def _fake_case(A, astray):
    """A torch-only "entry point" with the shape of the real ones (a memset of its workspace, an
    accumulation pass, a final pass), all of it inside its own buffers.  astray names the step
    that goes to the default stream instead of the caller's."""
    x = A.inp("x", torch.arange(1, 4097, dtype=torch.float32, device=DEV))
    y = A.out("y", (4096,))
    wp, _ = A.ws("workspace", 4096 * 4)
    w = A.last_ws

    def step(name, op):
        if name == astray:
            with torch.cuda.stream(torch.cuda.default_stream()):
                op()
        else:
            op()

    def call():
        step("memset", lambda: w.zero_())
        step("accumulate", lambda: w.add_(x))
        step("final", lambda: torch.mul(w, 2.0, out=y))
    return call, _clones(y=y)


@pytest.mark.gpu
@pytest.mark.parametrize("astray", [None, "memset", "accumulate", "final"])
def test_the_stream_test_notices_a_step_on_another_stream(gpu, side, astray):
    """Property 4's own check: it passes a fake entry point that keeps to the caller's stream and
    fails one whose memset, auxiliary pass or last pass goes to the default stream."""
    ref = {k: v.cpu() for k, v in _run_case(functools.partial(_fake_case, astray=None), Arena()).items()}
    assert torch.equal(ref["y"], 2.0 * torch.arange(1, 4097, dtype=torch.float32))
    case = functools.partial(_fake_case, astray=astray)
    if astray is None:
        _ordered_on_the_callers_stream(case, ref, side, "fake")
    else:
        with pytest.raises(AssertionError, match="differs from the plain call|not written"):
            _ordered_on_the_callers_stream(case, ref, side, "fake")


@pytest.mark.gpu
def test_the_producer_outlasts_the_enqueue(gpu, side):
    """The condition on property 4's test, measured: the producer's length by events against the
    host time to enqueue the longest cases behind it."""
    import time
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(side):
        e0.record()
        _produce()
        e1.record()
    torch.cuda.synchronize()
    producer_ms = e0.elapsed_time(e1)
    worst = 0.0
    import test_family_discipline as family  # (it imports this module: only here, when both are loaded)
    for name in ("corr_lookup_conv_bwd[A]", "corr_backward[A-bf16x6]", "corr_ondemand_backward[A]",
                 "corr_voxel_grid[nan_coords-norm1]", "corr_ondemand_lookup_conv[A]", "corr_enc_conv_forward[2x7x9-s2]"):
        owner = sys.modules[__name__] if name in CASES else family
        owner._plain(name)
        arena = Arena(guard_in=True, guard_out=True, guard_ws=True, defer=True)
        call, collect = owner.CASES[name][1](arena)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t0 = time.perf_counter()
            _produce()
            for view, values in arena.staged:
                view.copy_(values)
            for view in arena.fresh:
                _poison(view)
            call()
            collect()
            ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        print(f"enqueue of {name} behind the producer: {ms:.2f} ms")
        worst = max(worst, ms)
    print(f"producer {producer_ms:.1f} ms for {CHAIN} matmuls of {PRODUCER_N}; longest enqueue {worst:.2f} ms")
    assert producer_ms >= 4 * worst, (producer_ms, worst)


# ----------------------------------------------------------------------------------------------
# the ratchet (no GPU): a new entry point cannot arrive without someone deciding where it belongs
# ----------------------------------------------------------------------------------------------
# Entry points whose four properties (guarded outputs, honest statistics buffers, poisoned and
# misaligned inputs with the channels outside a channel window poisoned too, the caller's stream)
# tests/test_family_discipline.py checks with a table of its own: the convolution families, the
# on-demand lookup fused with convc1, the pyramid's import and export.  The family files keep
# their own window tests besides.
_FAMILY = "test_family_discipline.py::test_writes_stay_inside"
COVERED_ELSEWHERE = {
    "corr_conv_pack_weights": _FAMILY,
    "corr_conv_forward": _FAMILY,
    "corr_conv_forward_prec": _FAMILY,
    "corr_enc_conv_forward": _FAMILY,
    "corr_enc_norm_finalize": _FAMILY,
    "corr_enc_join": _FAMILY,
    "corr_enc_stem_pack_weights": _FAMILY,
    "corr_enc_stem_forward": _FAMILY,
    "corr_enc_pw_pack_weights": _FAMILY,
    "corr_enc_pw_forward": _FAMILY,
    "corr_enc_join_affine": _FAMILY,
    "corr_mask_upsample_pack_weights": _FAMILY,
    "corr_mask_upsample_forward": _FAMILY,
    "corr_flow_enc_pack_weights": _FAMILY,
    "corr_flow_enc_forward": _FAMILY,
    "corr_flow_head_pack_weights": _FAMILY,
    "corr_flow_head_forward": _FAMILY,
    "corr_ondemand_lookup_conv": _FAMILY,
    "corr_pyramid_export": _FAMILY,
    "corr_pyramid_import": _FAMILY,
}
# The reference-shaped wrappers: below their argument lists they are the code of the entry point
# named, which is in the table (csrc/corr_api.cpp: corr_build -> corr_build_rows <- corr_build_ex
# with CORR_BUILD_FP32; corr_lookup -> corr_lookup_rows; corr_lookup_bwd -> corr_lookup_bwd_rows;
# corr_build_bwd -> corr_build_bwd_rows <- corr_build_bwd_ex with CORR_BUILD_FP32).
FORWARDS_TO = {
    "corr_build": "corr_build_ex", "corr_build_rows": "corr_build_ex", "corr_lookup": "corr_lookup_rows",
    "corr_lookup_bwd": "corr_lookup_bwd_rows", "corr_build_bwd": "corr_build_bwd_ex",
    "corr_build_bwd_rows": "corr_build_bwd_ex",
}

def _header_entry_points():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "corr_mi355x.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    protos = re.findall(r"\b(corr_\w+)\s*\(([^;{]*?)\)\s*;", text)
    return {name for name, args in protos if re.search(r"void\s*\*\s*stream\b", args)}, {name for name, _ in protos}


def test_every_stream_taking_entry_point_is_accounted_for():
    with_stream, all_names = _header_entry_points()
    assert len(with_stream) >= 40 and "corr_build_ex" in with_stream and "corr_version" not in with_stream
    in_table = {entry for entry, _ in CASES.values()}
    groups = {"CASES": in_table, "COVERED_ELSEWHERE": set(COVERED_ELSEWHERE), "FORWARDS_TO": set(FORWARDS_TO)}
    homes = {n: [g for g, names in groups.items() if n in names] for n in with_stream}
    missing = sorted(n for n, h in homes.items() if not h)
    assert not missing, f"entry points with a stream argument and no discipline test: {missing}"
    twice = {n: h for n, h in homes.items() if len(h) > 1}
    assert not twice, f"listed in more than one place: {twice}"
    for g, names in groups.items():
        stale = sorted(names - with_stream)
        assert not stale, f"{g} names what the header does not declare with a stream: {stale}"
    assert set(FORWARDS_TO.values()) <= in_table
    assert set(WORKSPACE_ENTRIES) <= in_table
    assert set(WORKSPACE_ENTRIES.values()) <= all_names
    tests_dir = os.path.dirname(os.path.abspath(__file__))
    for name, owner in COVERED_ELSEWHERE.items():
        path, test = owner.split("::")
        with open(os.path.join(tests_dir, path)) as f:
            src = f.read()
        assert re.search(rf"^def {test}\b", src, flags=re.M), f"{owner} does not exist"
        assert name in src or name[len("corr_"):] in src, f"{owner}'s file never calls {name}"


def test_the_table_names_every_case_the_suite_promises():
    """The entry points of the core library, each with at least one case."""
    want = {"corr_build_ex": 3, "corr_build_region": 1, "corr_lookup_rows": 1, "corr_lookup_bwd_rows": 1,
            "corr_lookup_bwd_multi": 1, "corr_pool_bwd": 1, "corr_pool_fold": 1, "corr_build_bwd_ex": 3,
            "corr_backward": 4, "corr_lookup_conv_weights": 1, "corr_lookup_conv": 1, "corr_lookup_conv_bwd": 1,
            "corr_ondemand_prepare": 2, "corr_ondemand_lookup": 2, "corr_ondemand_backward": 2, "corr_forward_splat": 1,
            "corr_convex_upsample": 4, "corr_convex_upsample_bwd": 4, "corr_voxel_grid": 3,
            "corr_voxel_grid_tbilinear": 2, "corr_gru_pack_weights": 1, "corr_gru_half_step": 4,
            "corr_gru_half_step_prec": 8}
    have = {}
    for entry, _ in CASES.values():
        have[entry] = have.get(entry, 0) + 1
    assert set(have) == set(want)
    for entry, n in want.items():
        assert have[entry] >= n, (entry, have[entry], n)
