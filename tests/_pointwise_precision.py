"""Helpers of tests/test_pointwise_precision.py: the two fused 1x1 convolutions (lookup + convc1,
the mask head with the convex upsampling) in a precision mode, through the raw C ABI and through
eraft_amd._lib; the numpy value of products<NP>() on a single product as the MFMA rounds it; the
shared inputs (read-only by convention) and the fp64 evaluations the GPU tests compare with.
"""
import ctypes
import functools

import numpy as np
import torch
import torch.nn.functional as F

import _bf16x6 as bx
import _precision as pm
import prng

F32, F64 = np.float32, np.float64
DEV = "cuda:0"
REDUCED = ("bf16x3", "bf16")
SCALE = 0.25              # the reference's factor on the mask (update.py:106)
LC_STEPS, MU_STEPS = 11, 8  # K steps of 32 that feed one output: kLcKC (352 / 32) and kMuKS (256 / 32)
C_ROUND = 5               # tests/test_bf16x6_family.py::test_error_bound's c
# lookup + convc1: (B, D, H, W, L, coordinate spread).  The first is test_lookup_conv_weight_pieces's;
# the second has 60 queries (one full and one partial 32-query block) and K = 162 padded to 352.
# Their coordinates are wide, so that every window tap of every level meets the map somewhere: 10 %
# and 18 % of the lookups are non-zero.  "-dense" has the second shape's coordinates within a pixel
# of the grid (a realistic flow): 42 % non-zero, as dense as radius-4 windows on a 6x10 map get.
LC_SHAPES = {"16x24-L4": (2, 32, 16, 24, 4, 24.0), "6x10-L2": (1, 32, 6, 10, 2, 6.0),
             "6x10-L2-dense": (1, 32, 6, 10, 2, 1.0)}
LC_PIECES = ("16x24-L4", "6x10-L2")   # the shapes of the kept-products test
# mask head (B, H, W): whole blocks; partial blocks and B > 1; 3 blocks in all, so the last
# workgroup's second block is dead
MU_SHAPES = [(1, 8, 32), (2, 7, 9), (1, 3, 9)]


def gpu(a):
    return torch.from_numpy(np.ascontiguousarray(a, F32)).to(DEV)


# ----------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------
def mode_product(w, x, mode):
    """The kernels' value of the single product w * x (elementwise) in `mode`, products<NP>()'s
    order with the MFMA's rounding of every partial sum (bx.mfma_acc) and split_sum's fp32 join:
    bf16x6 is bx.six_model(mfma=True); bf16x3 is acs = (0 + wm xh) + wh xm, acc = wh xh, acc + acs;
    bf16 is acc = wh xh alone.  (A product of two bf16 pieces is exact in fp32.)"""
    if mode == "bf16x6":
        return bx.six_model(w, x, mfma=True)
    wp, xp = bx.split3(w), bx.split3(x)
    with np.errstate(invalid="ignore", over="ignore"):
        acc = (wp[0] * xp[0]).astype(F32)
        if mode == "bf16":
            return acc
        acs = bx.mfma_acc((wp[1] * xp[0]).astype(F32), wp[0], xp[1])
        return np.where(np.isinf(acc), acc, (acc + acs).astype(F32)).astype(F32)


# ----------------------------------------------------------------------------------------------
# lookup + convc1
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def lc_block(key):
    """(CorrBlock, coords on the GPU, the unfused lookup [B, C, H, W] as numpy) of a shape key."""
    import eraft_amd
    B, D, H, W, L, spread = LC_SHAPES[key]
    f1, f2 = prng.gauss(71, (B, D, H, W)), prng.gauss(72, (B, D, H, W))
    coords = gpu(prng.lookup_coords(73, B, H, W, spread))
    with torch.no_grad():
        blk = eraft_amd.CorrBlock(gpu(f1), gpu(f2), num_levels=L, radius=4)
        look = blk(coords).cpu().numpy()
    return blk, coords, look


def lc_run(blk, coords, w, bias, mode, relu=False):
    """_lib.lookup_conv in `mode` of numpy w [256, C] and bias [256] -> numpy [B, 256, H, W]."""
    from eraft_amd import _lib
    B, _, H, W = coords.shape
    out = torch.full((B, 256, H, W), float("nan"), dtype=torch.float32, device=DEV)
    _lib.lookup_conv(blk._state.levels, coords, 4, _lib.lookup_conv_weights(gpu(w)), gpu(bias), out, relu,
                     precision=pm.CODE[mode])
    return out.cpu().numpy()


def _ptrs(ts):
    arr = (ctypes.c_void_p * len(ts))()
    for k, t in enumerate(ts):
        arr[k] = t.data_ptr()
    return arr


def lc_raw(blk, coords, packed, bias, relu, precision=None):
    """corr_lookup_conv (precision None) or corr_lookup_conv_prec straight through ctypes."""
    from eraft_amd import _lib
    lib = _lib.load()
    B, _, H, W = coords.shape
    lv = blk._state.levels
    out = torch.full((B, 256, H, W), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    head = (_ptrs(lv), coords.data_ptr(), B, H, W, len(lv), 4, packed.data_ptr(), bias.data_ptr(), int(relu),
            out.data_ptr())
    rc = lib.corr_lookup_conv(*head, st) if precision is None else lib.corr_lookup_conv_prec(*head, precision, st)
    assert rc == 0, lib.corr_last_error().decode()
    return out


@functools.lru_cache(maxsize=None)
def lc_dense(key):
    """Dense Gaussian (w [256, C], bias [256]) of a shape key."""
    C = LC_SHAPES[key][4] * 81
    return prng.gauss(75, (256, C), 0.1), prng.gauss(76, (256,), 0.1)


# ----------------------------------------------------------------------------------------------
# the mask head
# ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mu_flow(B, H, W):
    return prng.gauss(62, (B, 2, H, W), 3.0)


def mu_run(hidden, w, bias, mode, off=0, flow=None, packed=None):
    """_lib.mask_upsample_forward in `mode` of numpy hidden [B, 256, H, W], w [576, 256], bias [576]
    -> numpy [B, 2, 8H, 8W]; with `off` hidden sits at channels off .. of a buffer whose other
    channels hold 1e30."""
    from eraft_amd import _lib
    B, _, H, W = hidden.shape
    buf = torch.full((B, 256 + off, H, W), 1e30, dtype=torch.float32, device=DEV)
    buf[:, off:] = gpu(hidden)
    pk = _lib.mask_upsample_pack_weights(gpu(w)) if packed is None else packed
    fl = gpu(mu_flow(B, H, W) if flow is None else flow)
    return _lib.mask_upsample_forward(buf, off, fl, pk, gpu(bias), SCALE, precision=pm.CODE[mode]).cpu().numpy()


def mu_raw(hidden, flow, packed, bias, precision=None):
    """corr_mask_upsample_forward (precision None) or ..._prec straight through ctypes (gpu tensors)."""
    from eraft_amd import _lib
    lib = _lib.load()
    B, hc, H, W = hidden.shape
    out = torch.full((B, 2, 8 * H, 8 * W), float("nan"), dtype=torch.float32, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    head = (hidden.data_ptr(), hc, 0, flow.data_ptr(), packed.data_ptr(), bias.data_ptr(), SCALE, B, H, W,
            out.data_ptr())
    rc = (lib.corr_mask_upsample_forward(*head, st) if precision is None
          else lib.corr_mask_upsample_forward_prec(*head, precision, st))
    assert rc == 0, lib.corr_last_error().decode()
    return out


@functools.lru_cache(maxsize=None)
def mu_dense(B, H, W, lscale=30):
    """(hidden = relu(gauss), w, bias) with logits of standard deviation near `lscale`, as
    tests/test_mask_upsample.py's.  The large scale (that suite's second one) is chosen a priori: the
    error of a logit grows with its magnitude in every mode, the fp32 softmax's own error (1e-7 of
    the output) does not, so at this scale the output's error is the logits' and the modes show."""
    sigma = lscale / (SCALE * np.sqrt(256 * 0.5))
    hidden = np.maximum(prng.gauss(911, (B, 256, H, W)), 0.0).astype(F32)
    return hidden, prng.gauss(901, (576, 256), sigma), prng.gauss(902, (576,), 0.1 * lscale / SCALE)


def upsample64(flow, logits):
    """The torch branch of ERAFT.upsample_flow in fp64: logits [B, 576, H, W] (already scaled)."""
    from eraft_amd.model import ERAFT
    return ERAFT.upsample_flow(torch.from_numpy(np.ascontiguousarray(flow)).double(), logits).numpy()


def mu_logits64(hidden, w, bias, mode=None):
    """SCALE (W hidden + bias) in fp64 as a torch tensor: exact operands (mode None) or the mode's
    definition, the sum of the products among the kept pieces (tests/_precision.py: conv64)."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    if mode is None:
        return SCALE * F.conv2d(t(hidden), t(w).view(576, 256, 1, 1), t(bias))
    return SCALE * torch.from_numpy(pm.conv64(hidden, w.reshape(576, 256, 1, 1), mode, 0, bias))
