"""ctypes binding of libcorr_mi355x.so (C-ABI: include/corr_mi355x.h).

This is the ONLY path to the kernels: there is no CPU or eager-PyTorch fallback.  If the
library is missing, or a tensor is not on a HIP device, calls raise.
torch is imported first so that the library binds to the HIP runtime torch already loaded
(both carry the SONAME libamdhip64.so.7), i.e. one runtime, one set of device pointers.
"""
from __future__ import annotations

import ctypes
import os

import torch

from .build import SO_PATH

CORR_OK = 0
CORR_EINVAL = -1
CORR_EUNSUPPORTED = -2
CORR_EHIP = -3
MAX_LEVELS = 8
MAX_RADIUS = 7

EXPORTS = ("corr_version", "corr_last_error", "corr_build", "corr_lookup", "corr_lookup_bwd",
           "corr_pool_bwd", "corr_build_bwd_workspace", "corr_build_bwd", "corr_build_rows",
           "corr_lookup_rows", "corr_lookup_bwd_rows", "corr_build_bwd_rows_workspace",
           "corr_build_bwd_rows", "corr_build_workspace", "corr_build_ex",
           "corr_build_bwd_ex_workspace", "corr_build_bwd_ex", "corr_forward_splat_workspace",
           "corr_forward_splat", "corr_convex_upsample", "corr_voxel_grid_workspace",
           "corr_voxel_grid", "corr_lookup_conv", "corr_lookup_conv_weights", "corr_lookup_conv_weights_bytes", "corr_voxel_grid_tbilinear_workspace",
           "corr_voxel_grid_tbilinear", "corr_lookup_bwd_multi", "corr_pool_fold", "corr_backward_workspace",
           "corr_backward", "corr_convex_upsample_bwd_workspace", "corr_convex_upsample_bwd", "corr_build_region",
           "corr_lookup_conv_bwd_workspace", "corr_lookup_conv_bwd", "corr_map_floats", "corr_pyramid_export",
           "corr_pyramid_import", "corr_ondemand_workspace", "corr_ondemand_prepare", "corr_ondemand_lookup",
           "corr_ondemand_bwd_workspace", "corr_ondemand_backward", "corr_gru_weights_bytes",
           "corr_gru_pack_weights", "corr_gru_workspace", "corr_gru_half_step", "corr_conv_weights_bytes",
           "corr_conv_pack_weights", "corr_conv_forward", "corr_enc_stats_bytes", "corr_enc_conv_forward",
           "corr_enc_norm_finalize", "corr_enc_join", "corr_mask_upsample_weights_bytes",
           "corr_mask_upsample_pack_weights", "corr_mask_upsample_forward", "corr_enc_stem_weights_bytes",
           "corr_enc_stem_pack_weights", "corr_enc_stem_forward", "corr_enc_pw_weights_bytes",
           "corr_enc_pw_pack_weights", "corr_enc_pw_forward", "corr_enc_join_affine",
           "corr_flow_enc_weights_bytes", "corr_flow_enc_pack_weights", "corr_flow_enc_forward",
           "corr_flow_head_weights_bytes", "corr_flow_head_pack_weights", "corr_flow_head_forward",
           "corr_ondemand_lookup_conv", "corr_gru_half_step_prec", "corr_conv_forward_prec")
# include/corr_mi355x_train.h: the sequence loss, alone and fused with the convex upsampling
TRAIN_EXPORTS = ("corr_upsample_loss_workspace", "corr_upsample_loss", "corr_upsample_loss_bwd",
                 "corr_sequence_loss_workspace", "corr_sequence_loss", "corr_sequence_loss_bwd")
# include/corr_mi355x_enc_prec.h: the encoders' convolutions in a precision mode
ENC_PREC_EXPORTS = ("corr_enc_conv_forward_prec", "corr_enc_stem_forward_prec", "corr_enc_pw_forward_prec")
# include/corr_mi355x_build_prec.h: the all-pairs build in a precision mode
BUILD_PREC_EXPORTS = ("corr_build_ex_prec", "corr_build_region_prec")
# include/corr_mi355x_pw_prec.h: lookup + convc1 and the mask head in a precision mode
PW_PREC_EXPORTS = ("corr_lookup_conv_prec", "corr_mask_upsample_forward_prec")
# include/corr_mi355x_train_head.h: the fused loss with the mask head inside the launch
TRAIN_HEAD_EXPORTS = ("corr_mask_upsample_loss_workspace", "corr_mask_upsample_loss", "corr_mask_upsample_loss_bwd")
ABI_VERSION = 202  # include/corr_mi355x.h: tiled value pyramid, separable fold, fp32 non-finite rule (bf16x6 bwd)

# Build algorithms (include/corr_mi355x.h).  BF16X6 is the default: every fp32 feature split
# exactly into three bf16 pieces, the six largest piece products on the bf16 MFMA, fp32
# accumulate — no narrower than the exact-fp32 MFMA build (test_build_bf16x6_not_narrower_than_fp32).
# ERAFT_AMD_BUILD=fp32 selects the fp32-operand MFMA build, =f16x3 the two-piece f16 split
# (~2^-22 per feature, narrower than fp32).
BUILD_FP32 = 0
BUILD_F16X3 = 1
BUILD_BF16X6 = 2
BUILD_ONLY_PACK = 0x100  # measurement: OR into BUILD_F16X3 / _BF16X6 to run only the operand pack
BUILD_ONLY_MFMA = 0x200  # ... or only the MFMA kernel (the workspace holds this pair's pack)
BACKWARD_EXACT_FOLD = 0x400  # OR into corr_backward's algo: the bit-exact fold (exact_fold())
_ALGOS = {"fp32": BUILD_FP32, "f16x3": BUILD_F16X3, "bf16x6": BUILD_BF16X6}


def default_algo() -> int:
    name = os.environ.get("ERAFT_AMD_BUILD", "bf16x6").lower()
    if name not in _ALGOS:
        raise ValueError(f"ERAFT_AMD_BUILD must be one of {sorted(_ALGOS)} (got {name!r})")
    return _ALGOS[name]


def backward_algo(algo=None) -> int:
    """The backward GEMMs' algorithm for a build algorithm: each build's own arithmetic (bf16x6:
    the exact three-piece bf16 split GEMMs, smaller worst / mean row error than fp32's; f16x3: the
    two-piece f16 split;
    fp32: the fp32-operand MFMA GEMMs)."""
    return default_algo() if algo is None else algo

_lib = None


class CorrError(RuntimeError):
    """A libcorr_mi355x call returned a negative status."""

    def __init__(self, code: int, msg: str):
        super().__init__(f"[corr {code}] {msg}")
        self.code = code


def load(path: str | None = None) -> ctypes.CDLL:
    """Load (once) and type the library.  Raises if it has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    so = path or SO_PATH
    if not os.path.exists(so):
        raise RuntimeError(
            f"{so} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(eraft_amd has no CPU fallback)")
    lib = ctypes.CDLL(so)
    vp, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    lib.corr_version.argtypes, lib.corr_version.restype = [], i
    lib.corr_last_error.argtypes, lib.corr_last_error.restype = [], ctypes.c_char_p
    lib.corr_map_floats.argtypes, lib.corr_map_floats.restype = [i, i], sz
    lib.corr_pyramid_export.argtypes = [vp, i, i, i, i, vp, vp]
    lib.corr_pyramid_import.argtypes = [vp, i, i, i, i, vp, vp]
    lib.corr_build.argtypes = [vp, vp, i, i, i, i, i, vp, vp]
    lib.corr_lookup.argtypes = [vp, vp, i, i, i, i, i, vp, vp]
    lib.corr_lookup_bwd.argtypes = [vp, vp, i, i, i, i, i, vp, vp]
    lib.corr_pool_bwd.argtypes = [vp, i, i, i, i, vp]
    lib.corr_build_bwd_workspace.argtypes = [i, i, i, i]
    lib.corr_build_bwd_workspace.restype = sz
    lib.corr_build_bwd.argtypes = [vp, vp, vp, i, i, i, i, vp, vp, vp, sz, vp]
    lib.corr_build_rows.argtypes = [vp, i, vp, i, i, i, i, i, vp, vp]
    lib.corr_lookup_rows.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp]
    lib.corr_lookup_bwd_rows.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp]
    lib.corr_build_bwd_rows_workspace.argtypes = [i, i, i, i, i]
    lib.corr_build_bwd_rows_workspace.restype = sz
    lib.corr_build_bwd_rows.argtypes = [vp, vp, i, vp, i, i, i, i, vp, vp, vp, sz, vp]
    lib.corr_build_workspace.argtypes = [i, i, i, i, i, i]
    lib.corr_build_workspace.restype = sz
    lib.corr_build_ex.argtypes = [i, vp, i, vp, i, i, i, i, i, vp, vp, sz, vp]
    lib.corr_build_bwd_ex_workspace.argtypes = [i, i, i, i, i, i]
    lib.corr_build_bwd_ex_workspace.restype = sz
    lib.corr_build_bwd_ex.argtypes = [i, vp, vp, i, vp, i, i, i, i, vp, vp, vp, sz, vp]
    lib.corr_forward_splat_workspace.argtypes = [i, i, i]
    lib.corr_forward_splat_workspace.restype = sz
    lib.corr_forward_splat.argtypes = [vp, i, i, i, vp, vp, sz, vp]
    lib.corr_convex_upsample.argtypes = [vp, vp, i, i, i, vp, vp]
    lib.corr_convex_upsample_bwd_workspace.argtypes = [i, i, i]
    lib.corr_convex_upsample_bwd_workspace.restype = sz
    lib.corr_convex_upsample_bwd.argtypes = [vp, vp, vp, i, i, i, vp, vp, vp, sz, vp]
    lib.corr_lookup_conv.argtypes = [vp, vp, i, i, i, i, i, vp, vp, i, vp, vp]
    lib.corr_lookup_conv_weights.argtypes = [vp, i, i, vp, vp]
    lib.corr_lookup_conv_weights_bytes.argtypes = []
    lib.corr_lookup_conv_weights_bytes.restype = sz
    lib.corr_voxel_grid_workspace.argtypes = [i, i, i, i]
    lib.corr_voxel_grid_workspace.restype = sz
    lib.corr_voxel_grid.argtypes = [vp, vp, vp, vp, i, i, i, i, i, vp, vp, sz, vp]
    lib.corr_voxel_grid_tbilinear_workspace.argtypes = [i, i, i, i]
    lib.corr_voxel_grid_tbilinear_workspace.restype = sz
    lib.corr_voxel_grid_tbilinear.argtypes = [vp, i, i, i, i, i, vp, vp, sz, vp]
    lib.corr_lookup_bwd_multi.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, vp]
    lib.corr_pool_fold.argtypes = [vp, i, i, i, i, i, vp]
    lib.corr_backward_workspace.argtypes = [i, i, i, i, i, i, i]
    lib.corr_backward_workspace.restype = sz
    lib.corr_backward.argtypes = [i, vp, vp, i, vp, i, vp, i, i, i, i, i, i, vp, vp, vp, vp, sz, vp]
    lib.corr_build_region.argtypes = [i, vp, i, vp, i, i, i, i, i, i, i, vp, vp, sz, i, vp]
    lib.corr_lookup_conv_bwd_workspace.argtypes = [i, i, i, i]
    lib.corr_lookup_conv_bwd_workspace.restype = sz
    lib.corr_lookup_conv_bwd.argtypes = [vp, vp, i, i, i, i, i, vp, vp, i, vp, vp, vp, vp, vp, sz, vp]
    lib.corr_ondemand_workspace.argtypes = [i, i, i, i, i]
    lib.corr_ondemand_workspace.restype = sz
    lib.corr_ondemand_prepare.argtypes = [vp, vp, i, i, i, i, i, vp, sz, vp]
    lib.corr_ondemand_lookup.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, vp]
    lib.corr_ondemand_lookup_conv.argtypes = [vp, vp, i, i, i, i, i, i, i, vp, vp, i, vp, vp]
    lib.corr_ondemand_bwd_workspace.argtypes = [i, i, i, i, i, i]
    lib.corr_ondemand_bwd_workspace.restype = sz
    lib.corr_ondemand_backward.argtypes = [vp, vp, vp, i, i, i, i, i, i, i, vp, sz, vp, vp, vp]
    lib.corr_gru_weights_bytes.argtypes, lib.corr_gru_weights_bytes.restype = [i, i], sz
    lib.corr_gru_pack_weights.argtypes = [vp, vp, vp, i, i, vp, vp]
    lib.corr_gru_workspace.argtypes, lib.corr_gru_workspace.restype = [i, i, i, i], sz
    lib.corr_gru_half_step.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp, vp, vp, vp, sz, vp, vp]
    lib.corr_gru_half_step_prec.argtypes = [vp, vp, i, i, i, i, i, i, vp, vp, vp, vp, vp, sz, vp, i, vp]
    lib.corr_conv_weights_bytes.argtypes, lib.corr_conv_weights_bytes.restype = [i, i], sz
    lib.corr_conv_pack_weights.argtypes = [vp, i, i, vp, vp]
    lib.corr_conv_forward.argtypes = [vp, i, vp, i, i, i, i, vp, vp, i, i, vp, i, i, vp]
    lib.corr_conv_forward_prec.argtypes = [vp, i, vp, i, i, i, i, vp, vp, i, i, vp, i, i, i, vp]
    lib.corr_enc_stats_bytes.argtypes, lib.corr_enc_stats_bytes.restype = [i, i, i, i], sz
    lib.corr_enc_conv_forward.argtypes = [vp, i, i, i, i, i, vp, vp, i, vp, vp, i, vp, vp, sz, vp]
    lib.corr_enc_norm_finalize.argtypes = [vp, i, i, i, i, ctypes.c_float, vp, vp, vp]
    lib.corr_enc_join.argtypes = [vp, vp, vp, i, vp, i, i, i, i, vp, vp]
    lib.corr_enc_stem_weights_bytes.argtypes, lib.corr_enc_stem_weights_bytes.restype = [i, i], sz
    lib.corr_enc_stem_pack_weights.argtypes = [vp, i, i, vp, vp]
    lib.corr_enc_stem_forward.argtypes = [vp, i, i, i, i, vp, vp, i, vp, vp, sz, vp]
    lib.corr_enc_pw_weights_bytes.argtypes, lib.corr_enc_pw_weights_bytes.restype = [i, i], sz
    lib.corr_enc_pw_pack_weights.argtypes = [vp, i, i, vp, vp]
    lib.corr_enc_pw_forward.argtypes = [vp, i, i, i, i, i, vp, vp, i, vp, vp, sz, vp]
    lib.corr_enc_join_affine.argtypes = [vp, vp, vp, i, vp, vp, vp, i, i, i, i, i, i, vp, vp]
    lib.corr_mask_upsample_weights_bytes.argtypes, lib.corr_mask_upsample_weights_bytes.restype = [], sz
    lib.corr_mask_upsample_pack_weights.argtypes = [vp, vp, vp]
    lib.corr_mask_upsample_forward.argtypes = [vp, i, i, vp, vp, vp, ctypes.c_float, i, i, i, vp, vp]
    lib.corr_flow_enc_weights_bytes.argtypes, lib.corr_flow_enc_weights_bytes.restype = [i], sz
    lib.corr_flow_enc_pack_weights.argtypes = [vp, i, vp, vp]
    lib.corr_flow_enc_forward.argtypes = [vp, i, i, i, vp, vp, i, i, vp, i, i, vp, i, i, vp]
    lib.corr_flow_head_weights_bytes.argtypes, lib.corr_flow_head_weights_bytes.restype = [], sz
    lib.corr_flow_head_pack_weights.argtypes = [vp, vp, vp]
    lib.corr_flow_head_forward.argtypes = [vp, i, i, i, i, i, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.corr_enc_conv_forward_prec.argtypes = [vp, i, i, i, i, i, vp, vp, i, vp, vp, i, vp, vp, sz, i, vp]
    lib.corr_enc_stem_forward_prec.argtypes = [vp, i, i, i, i, vp, vp, i, vp, vp, sz, i, vp]
    lib.corr_enc_pw_forward_prec.argtypes = [vp, i, i, i, i, i, vp, vp, i, vp, vp, sz, i, vp]
    lib.corr_build_ex_prec.argtypes = [i, vp, i, vp, i, i, i, i, i, vp, vp, sz, i, vp]
    lib.corr_build_region_prec.argtypes = [i, vp, i, vp, i, i, i, i, i, i, i, vp, vp, sz, i, i, vp]
    lib.corr_lookup_conv_prec.argtypes = [vp, vp, i, i, i, i, i, vp, vp, i, vp, i, vp]
    lib.corr_mask_upsample_forward_prec.argtypes = [vp, i, i, vp, vp, vp, ctypes.c_float, i, i, i, vp, i, vp]
    fl = ctypes.c_float
    lib.corr_upsample_loss_workspace.argtypes, lib.corr_upsample_loss_workspace.restype = [i, i, i], sz
    lib.corr_upsample_loss.argtypes = [vp, vp, vp, vp, i, i, i, i, i, fl, i, vp, vp, sz, vp]
    lib.corr_upsample_loss_bwd.argtypes = [vp, vp, vp, vp, vp, i, i, i, i, i, fl, vp, vp, vp, sz, vp]
    lib.corr_sequence_loss_workspace.argtypes, lib.corr_sequence_loss_workspace.restype = [i, i, i], sz
    lib.corr_sequence_loss.argtypes = [vp, vp, vp, i, i, i, fl, i, vp, vp, sz, vp]
    lib.corr_sequence_loss_bwd.argtypes = [vp, vp, vp, vp, i, i, i, fl, vp, vp]
    lib.corr_mask_upsample_loss_workspace.argtypes, lib.corr_mask_upsample_loss_workspace.restype = [i, i, i], sz
    lib.corr_mask_upsample_loss.argtypes = [vp, i, i, vp, vp, vp, fl, vp, vp, i, i, i, i, i, fl, i, vp, vp, sz, vp]
    lib.corr_mask_upsample_loss_bwd.argtypes = [vp, i, i, vp, vp, vp, fl, vp, vp, vp, i, i, i, i, i, fl, vp, vp, vp,
                                                sz, vp]
    for f in ("corr_upsample_loss", "corr_upsample_loss_bwd", "corr_sequence_loss", "corr_sequence_loss_bwd",
              "corr_mask_upsample_loss", "corr_mask_upsample_loss_bwd",
              "corr_gru_half_step_prec", "corr_conv_forward_prec", *ENC_PREC_EXPORTS, *BUILD_PREC_EXPORTS,
              *PW_PREC_EXPORTS):
        getattr(lib, f).restype = i
    for f in ("corr_ondemand_lookup_conv", "corr_flow_enc_pack_weights", "corr_flow_enc_forward", "corr_flow_head_pack_weights",
              "corr_flow_head_forward", "corr_enc_stem_pack_weights", "corr_enc_stem_forward", "corr_enc_pw_pack_weights", "corr_enc_pw_forward",
              "corr_enc_join_affine", "corr_mask_upsample_pack_weights", "corr_mask_upsample_forward", "corr_enc_conv_forward", "corr_enc_norm_finalize", "corr_enc_join", "corr_conv_pack_weights", "corr_conv_forward", "corr_gru_pack_weights", "corr_gru_half_step", "corr_ondemand_backward", "corr_ondemand_prepare", "corr_ondemand_lookup", "corr_build_region", "corr_build", "corr_lookup", "corr_lookup_bwd", "corr_pool_bwd", "corr_build_bwd",
              "corr_build_rows", "corr_lookup_rows", "corr_lookup_bwd_rows", "corr_build_bwd_rows",
              "corr_build_ex", "corr_build_bwd_ex", "corr_forward_splat",
              "corr_convex_upsample", "corr_voxel_grid", "corr_lookup_conv", "corr_lookup_conv_weights",
              "corr_voxel_grid_tbilinear", "corr_lookup_bwd_multi", "corr_pool_fold",
              "corr_backward", "corr_convex_upsample_bwd", "corr_lookup_conv_bwd", "corr_pyramid_export",
              "corr_pyramid_import"):
        getattr(lib, f).restype = i
    if lib.corr_version() != ABI_VERSION:
        raise RuntimeError(f"{so} has ABI {lib.corr_version()}, eraft_amd needs {ABI_VERSION}: rebuild it")
    if path is None:
        _lib = lib
    return lib


def _check(rc: int):
    if rc != CORR_OK:
        raise CorrError(rc, load().corr_last_error().decode(errors="replace"))


def _dev(t: torch.Tensor, name: str) -> int:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{name} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise RuntimeError(f"{name} is on {t.device}: eraft_amd runs only on an MI355X (HIP) device")
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (got {t.dtype})")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t.data_ptr()


def _ptrs(ts, name):
    arr = (ctypes.c_void_p * len(ts))()
    for k, t in enumerate(ts):
        arr[k] = _dev(t, f"{name}[{k}]")
    return arr


TILE_W = 4  # cells per tile row (include/corr_mi355x.h): tiles of 4 rows x TILE_W cells


def map_floats(Hl: int, Wl: int) -> int:
    """Floats of one query's tiled level map (include/corr_mi355x.h, corr_map_floats)."""
    return ((Hl + 3) // 4) * ((Wl + TILE_W - 1) // TILE_W) * 4 * TILE_W


def _check_levels(levels, BN: int, H: int, W: int, name: str, tiled: bool = True, exact: bool = False):
    """Every level tensor must hold the BN maps the library will read or write: BN * map_floats
    of the level for the tiled value pyramid, BN * H_l * W_l for the row-major ones (gradient
    pyramids, the reference-layout export).  The C-ABI takes bare pointers, so a short buffer
    (e.g. a caller still allocating the ABI-104 row-major [B*N, 1, H_l, W_l] value levels, which
    are smaller than the tiled maps whenever H_l or W_l is not a multiple of 4) would be an
    out-of-bounds device access: refuse it here."""
    if not 1 <= len(levels) <= MAX_LEVELS:
        raise ValueError(f"{name}: {len(levels)} levels (1..{MAX_LEVELS} supported)")
    for l, t in enumerate(levels):
        h, w = H >> l, W >> l
        need = BN * (map_floats(h, w) if tiled else h * w)
        n = t.numel()
        if n < need or (exact and n != need):
            what = f"{BN} maps of {'map_floats' if tiled else 'H_l*W_l'}({h}, {w})"
            raise ValueError(f"{name}[{l}] has {n} floats, needs {'exactly ' if exact else ''}{need} ({what})")


def _stream(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


# ---- arguments that the bf16x6 convolution wrappers share ----
def _new_pack(nbytes, device):
    return torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=device)


def _pack_weights(w, size_fn, pack_fn, args, what):
    """A new pack of the contiguous fp32 weight `w` (or a dict name -> weight, in the entry point's
    order): lib.size_fn(*args) bytes (0: CORR_EUNSUPPORTED, `what` tells the sizes), filled by
    lib.pack_fn(weights..., *args, pack, stream)."""
    ws = w if isinstance(w, dict) else {"w": w}
    first = next(iter(ws.values()))
    lib = load()
    n = getattr(lib, size_fn)(*args)
    if n == 0:
        raise CorrError(CORR_EUNSUPPORTED, f"{size_fn}: unsupported {what}")
    ptrs = [_dev(t, name) for name, t in ws.items()]
    packed = _new_pack(n, first.device)
    with torch.cuda.device(first.device):
        _check(getattr(lib, pack_fn)(*ptrs, *args, packed.data_ptr(), _stream(first)))
    return packed


def _pack_arg(packed, need, device, what):
    """The pointer of a pack, which must hold the `need` bytes that `what` reads, on `device`."""
    pk = _dev(packed, "packed")
    if packed.numel() * 4 < need or packed.device != device:
        raise ValueError(f"packed holds {packed.numel() * 4} bytes on {packed.device}, {what} needs "
                         f"{need} on {device}")
    return pk


def _bias_arg(bias, n, device, optional=True):
    """The pointer of a bias of n values on `device`; None for no bias where the kernel takes that."""
    if bias is None and optional:
        return None
    bp = _dev(bias, "bias")
    if bias.numel() != n or bias.device != device:
        raise ValueError(f"bias must hold {'cout = ' if optional else ''}{n} values on {device} "
                         f"(got {tuple(bias.shape)})")
    return bp


def _window_arg(t, name, B, H, W, offset, n, device):
    """The pointer of `t`, which must be a [B, *, H, W] map on `device` with channels offset ..
    offset + n - 1."""
    tp = _dev(t, name)
    if (t.dim() != 4 or t.shape[0] != B or tuple(t.shape[2:]) != (H, W) or t.device != device
            or offset < 0 or offset + n > t.shape[1]):
        raise ValueError(f"{name} {tuple(t.shape)} does not hold channels {offset} .. {offset + n - 1} "
                         f"of a [{B}, *, {H}, {W}] map on {device}")
    return tp


def _nq(t):
    """Query pixels per batch item of a [B, C, rows, W] (or [B, C, NQ]) tensor."""
    n = 1
    for d in t.shape[2:]:
        n *= d
    return n


def pyramid_export(levels, H, W, out=None):
    """corr_pyramid_export: the tiled levels ([BN, map_floats]) -> the reference's layout, a list
    of [BN, 1, H_l, W_l] tensors (allocated unless `out` is given)."""
    BN = levels[0].shape[0]
    _check_levels(levels, BN, H, W, "pyr")
    if out is None:
        out = [torch.empty((BN, 1, H >> l, W >> l), dtype=torch.float32, device=levels[0].device)
               for l in range(len(levels))]
    elif len(out) != len(levels):
        raise ValueError(f"out has {len(out)} levels, the pyramid {len(levels)}")
    _check_levels(out, BN, H, W, "out", tiled=False, exact=True)
    with torch.cuda.device(levels[0].device):
        _check(load().corr_pyramid_export(_ptrs(levels, "pyr"), BN, H, W, len(levels), _ptrs(out, "out"),
                                          _stream(levels[0])))
    return out


def pyramid_import(src, levels, H, W):
    """corr_pyramid_import: reference-layout levels [BN, 1, H_l, W_l] (any contiguous view) ->
    the tiled `levels` (padding cells zeroed)."""
    BN = levels[0].shape[0]
    src = [t.contiguous() for t in src]
    if len(src) != len(levels):
        raise ValueError(f"src has {len(src)} levels, the pyramid {len(levels)}")
    for l, t in enumerate(src):
        if t.numel() != BN * (H >> l) * (W >> l):
            raise ValueError(f"level {l} has {t.numel()} values, expected {BN}x{H >> l}x{W >> l}")
    _check_levels(levels, BN, H, W, "pyr")
    with torch.cuda.device(levels[0].device):
        _check(load().corr_pyramid_import(_ptrs(src, "src"), BN, H, W, len(levels), _ptrs(levels, "pyr"),
                                          _stream(levels[0])))


def build_workspace(fmap1, fmap2, algo=None):
    """A device workspace for corr_build_ex (None when the algorithm needs none).  fmap2: the
    target map or just its shape [B, D, H, W]."""
    algo = default_algo() if algo is None else algo
    B, D, H, W = fmap2 if isinstance(fmap2, (tuple, list, torch.Size)) else fmap2.shape
    n = load().corr_build_workspace(algo, B, D, _nq(fmap1), H, W)
    if n == ctypes.c_size_t(-1).value:
        raise CorrError(CORR_EUNSUPPORTED, f"build algorithm {algo} does not support D = {D}")
    if n == 0:
        return None
    return torch.empty(n, dtype=torch.uint8, device=fmap1.device)


def build(fmap1, fmap2, levels, algo=None, workspace=None, precision=0):
    """corr_build_ex_prec into caller-allocated tiled levels (corr._alloc_pyramid).  fmap1 may be a row
    slab [B, D, rows, W] of the query map; fmap2 is the full target map [B, D, H, W].
    algo: BUILD_BF16X6 (default, see default_algo), BUILD_F16X3 or BUILD_FP32.  precision: a
    CORR_PREC_* value (precision.code); a reduced one needs BUILD_BF16X6."""
    algo = default_algo() if algo is None else algo
    B, D, H, W = fmap2.shape
    a, b, pp = _dev(fmap1, "fmap1"), _dev(fmap2, "fmap2"), _ptrs(levels, "pyr")
    _check_levels(levels, B * _nq(fmap1), H, W, "pyr")
    if workspace is None:
        workspace = build_workspace(fmap1, fmap2, algo & 0xff)
    wp = 0 if workspace is None else workspace.data_ptr()
    wn = 0 if workspace is None else workspace.numel() * workspace.element_size()
    with torch.cuda.device(fmap1.device):
        _check(load().corr_build_ex_prec(algo, a, _nq(fmap1), b, B, D, H, W, len(levels), pp, wp, wn,
                                         int(precision), _stream(fmap1)))


REGION_PACK_QUERIES = 1


def build_region(fmap1, fmap2_rows, y0, y1, H, levels, workspace, pack_queries, algo=BUILD_BF16X6, precision=0):
    """corr_build_region_prec: the pyramid entries of target rows [y0, y1) (tiled levels, corr._alloc_pyramid)
    from fmap2_rows [B, D, y1 - y0, W]; workspace from build_workspace(fmap1, <full fmap2 shape>).
    precision: a CORR_PREC_* value, the same for every region call of one build."""
    B, D, rows, W = fmap2_rows.shape
    if rows != y1 - y0:
        raise ValueError(f"fmap2_rows has {rows} rows for the region [{y0}, {y1})")
    a, b, pp = _dev(fmap1, "fmap1"), _dev(fmap2_rows, "fmap2_rows"), _ptrs(levels, "pyr")
    _check_levels(levels, B * _nq(fmap1), H, W, "pyr")
    with torch.cuda.device(fmap1.device):
        _check(load().corr_build_region_prec(algo, a, _nq(fmap1), b, y0, y1, B, D, H, W, len(levels), pp,
                                             workspace.data_ptr(), workspace.numel() * workspace.element_size(),
                                             REGION_PACK_QUERIES if pack_queries else 0, int(precision),
                                             _stream(fmap1)))


def lookup(levels, coords, radius, out, H=None, W=None):
    """corr_lookup_rows: coords [B, 2, rows, W] -> out [B, L*K, rows, W].  (H, W) = target map
    (default: the coords' own, i.e. the reference shape)."""
    B = coords.shape[0]
    H = coords.shape[2] if H is None else H
    W = coords.shape[3] if W is None else W
    pp, c, o = _ptrs(levels, "pyr"), _dev(coords, "coords"), _dev(out, "out")
    _check_levels(levels, B * _nq(coords), H, W, "pyr")
    K = (2 * radius + 1) ** 2
    if out.numel() != B * len(levels) * K * _nq(coords):
        raise ValueError(f"out has {out.numel()} floats, the lookup writes {B}x{len(levels) * K}x{_nq(coords)}")
    with torch.cuda.device(coords.device):
        _check(load().corr_lookup_rows(pp, c, B, _nq(coords), H, W, len(levels), radius, o,
                                       _stream(coords)))


def lookup_bwd(coords, grad_out, radius, grad_levels, H=None, W=None):
    B = coords.shape[0]
    H = coords.shape[2] if H is None else H
    W = coords.shape[3] if W is None else W
    c, g, gp = _dev(coords, "coords"), _dev(grad_out, "grad_out"), _ptrs(grad_levels, "grad_pyr")
    _check_levels(grad_levels, B * _nq(coords), H, W, "grad_pyr", tiled=False)
    with torch.cuda.device(coords.device):
        _check(load().corr_lookup_bwd_rows(c, g, B, _nq(coords), H, W, len(grad_levels), radius, gp,
                                           _stream(coords)))


def pool_bwd(grad_levels, H, W):
    BN = grad_levels[0].shape[0]
    gp = _ptrs(grad_levels, "grad_pyr")
    _check_levels(grad_levels, BN, H, W, "grad_pyr", tiled=False)
    with torch.cuda.device(grad_levels[0].device):
        _check(load().corr_pool_bwd(gp, BN, H, W, len(grad_levels), _stream(grad_levels[0])))


def build_bwd(grad_c, fmap1, fmap2, algo=None):
    """Returns (dfmap1, dfmap2) for grad_c = dLoss/dcorr ([B*NQ, H*W] or any view of it).
    With a row slab fmap1, dfmap1 is the slab's and dfmap2 is this slab's partial sum.
    algo: BUILD_BF16X6 (default, see backward_algo), BUILD_F16X3 or BUILD_FP32 (corr_build_bwd_ex)."""
    algo = backward_algo() if algo is None else algo
    B, D, H, W = fmap2.shape
    for t, nm in ((grad_c, "grad_c"), (fmap1, "fmap1"), (fmap2, "fmap2")):
        _dev(t, nm)
    lib = load()
    NQ = _nq(fmap1)
    if grad_c.numel() != B * NQ * H * W:
        raise ValueError(f"grad_c has {grad_c.numel()} values, expected {B * NQ}x{H * W}")
    ws_bytes = lib.corr_build_bwd_ex_workspace(algo, B, D, NQ, H, W)
    if ws_bytes == ctypes.c_size_t(-1).value:
        raise CorrError(CORR_EUNSUPPORTED, f"unknown backward algorithm {algo}")
    df1 = torch.empty_like(fmap1)
    df2 = torch.empty_like(fmap2)
    ws = torch.empty(max(1, (ws_bytes + 3) // 4), dtype=torch.float32, device=fmap1.device)
    with torch.cuda.device(fmap1.device):
        _check(lib.corr_build_bwd_ex(algo, grad_c.data_ptr(), fmap1.data_ptr(), NQ, fmap2.data_ptr(), B,
                                     D, H, W, df1.data_ptr(), df2.data_ptr(), ws.data_ptr(),
                                     ws.numel() * 4, _stream(fmap1)))
    return df1, df2


def lookup_bwd_multi(coords_list, grad_list, radius, grad_levels, H=None, W=None):
    """corr_lookup_bwd_multi: the lookups' input-gradients, in order, into grad_levels, which it
    OVERWRITES (no zeroing needed)."""
    c0 = coords_list[0]
    B = c0.shape[0]
    H = c0.shape[2] if H is None else H
    W = c0.shape[3] if W is None else W
    cp, gp = _ptrs(coords_list, "coords"), _ptrs(grad_list, "grad_out")
    _check_levels(grad_levels, B * _nq(c0), H, W, "grad_pyr", tiled=False)
    with torch.cuda.device(c0.device):
        _check(load().corr_lookup_bwd_multi(cp, gp, len(coords_list), B, _nq(c0), H, W, len(grad_levels), radius,
                                            _ptrs(grad_levels, "grad_pyr"), _stream(c0)))


def pool_fold(grad_levels, B, H, W):
    """corr_pool_fold: the pool-backward chain folded into grad_levels[0] in one pass."""
    NQ = grad_levels[0].shape[0] // B
    _check_levels(grad_levels, B * NQ, H, W, "grad_pyr", tiled=False)
    with torch.cuda.device(grad_levels[0].device):
        _check(load().corr_pool_fold(_ptrs(grad_levels, "grad_pyr"), B, NQ, H, W, len(grad_levels),
                                     _stream(grad_levels[0])))


def exact_fold() -> bool:
    """ERAFT_AMD_EXACT_FOLD=1: corr_backward's fused fold replays grid_sampler_2d_backward's
    per-tap products bit for bit (CORR_BACKWARD_EXACT_FOLD) instead of the separable closed form
    (dC within ~1e-7 of the staged path, the default)."""
    return os.environ.get("ERAFT_AMD_EXACT_FOLD", "0") == "1"


def backward(coords_list, grad_list, radius, grad_levels, fmap1, fmap2, algo=None, exact=None):
    """corr_backward: (dfmap1, dfmap2) of one build and its lookups (all at once, in order).
    grad_levels: scratch gradient pyramid (overwritten; level 0 ends as dLoss/dcorr).
    algo: the GEMMs' algorithm (default: backward_algo()); exact: the bit-exact fold (default:
    exact_fold())."""
    algo = backward_algo() if algo is None else algo
    exact = exact_fold() if exact is None else exact
    B, D, H, W = fmap2.shape
    lib = load()
    NQ = _nq(fmap1)
    ws_bytes = lib.corr_backward_workspace(algo, B, D, NQ, H, W, radius)
    if exact:
        algo |= BACKWARD_EXACT_FOLD
    if ws_bytes == ctypes.c_size_t(-1).value:
        raise CorrError(CORR_EUNSUPPORTED, f"unknown backward algorithm {algo}")
    _check_levels(grad_levels, B * NQ, H, W, "grad_pyr", tiled=False)
    df1 = torch.empty_like(fmap1)
    df2 = torch.empty_like(fmap2)
    ws = torch.empty(max(1, (ws_bytes + 3) // 4), dtype=torch.float32, device=fmap1.device)
    cp, gp = _ptrs(coords_list, "coords"), _ptrs(grad_list, "grad_out")
    with torch.cuda.device(fmap1.device):
        _check(lib.corr_backward(algo, cp, gp, len(coords_list), _dev(fmap1, "fmap1"), NQ, _dev(fmap2, "fmap2"), B, D,
                                 H, W, len(grad_levels), radius, _ptrs(grad_levels, "grad_pyr"), df1.data_ptr(),
                                 df2.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream(fmap1)))
    return df1, df2


def fused_backward() -> bool:
    """ERAFT_AMD_FUSED_BWD=0 selects the per-lookup backward (lookup_bwd per call + pool_bwd +
    build_bwd) instead of corr_backward at the build's backward."""
    return os.environ.get("ERAFT_AMD_FUSED_BWD", "1") != "0"


def forward_splat(flow, out):
    """corr_forward_splat: flow [B, 2, H, W] -> out (same shape), caller-allocated."""
    B, C, H, W = flow.shape
    if C != 2:
        raise ValueError(f"flow must be [B, 2, H, W] (got {tuple(flow.shape)})")
    f, o = _dev(flow, "flow"), _dev(out, "out")
    lib = load()
    n = lib.corr_forward_splat_workspace(B, H, W)
    ws = torch.empty(max(1, (n + 3) // 4), dtype=torch.int32, device=flow.device)
    with torch.cuda.device(flow.device):
        _check(lib.corr_forward_splat(f, B, H, W, o, ws.data_ptr(), ws.numel() * 4, _stream(flow)))


def convex_upsample(flow, mask, out):
    """corr_convex_upsample: flow [N, 2, h, w], mask [N, 576, h, w] -> out [N, 2, 8h, 8w]."""
    N, C, h, w = flow.shape
    if C != 2 or tuple(mask.shape) != (N, 576, h, w) or tuple(out.shape) != (N, 2, 8 * h, 8 * w):
        raise ValueError(f"convex_upsample: flow {tuple(flow.shape)}, mask {tuple(mask.shape)}, "
                         f"out {tuple(out.shape)}")
    f, m, o = _dev(flow, "flow"), _dev(mask, "mask"), _dev(out, "out")
    with torch.cuda.device(flow.device):
        _check(load().corr_convex_upsample(f, m, N, h, w, o, _stream(flow)))


def convex_upsample_bwd(flow, mask, grad_out):
    """corr_convex_upsample_bwd: -> (dflow [N, 2, h, w], dmask [N, 576, h, w])."""
    N, _, h, w = flow.shape
    if tuple(mask.shape) != (N, 576, h, w) or tuple(grad_out.shape) != (N, 2, 8 * h, 8 * w):
        raise ValueError(f"convex_upsample_bwd: flow {tuple(flow.shape)}, mask {tuple(mask.shape)}, "
                         f"grad_out {tuple(grad_out.shape)}")
    lib = load()
    dflow = torch.empty_like(flow)
    dmask = torch.empty_like(mask)
    ws = torch.empty(lib.corr_convex_upsample_bwd_workspace(N, h, w), dtype=torch.uint8, device=flow.device)
    with torch.cuda.device(flow.device):
        _check(lib.corr_convex_upsample_bwd(_dev(flow, "flow"), _dev(mask, "mask"), _dev(grad_out, "grad_out"),
                                            N, h, w, _dev(dflow, "dflow"), _dev(dmask, "dmask"),
                                            ws.data_ptr(), ws.numel(), _stream(flow)))
    return dflow, dmask


def _loss_frame(name, gt, valid, N):
    """(H, W) of gt [N, 2, H, W] and valid [N, H, W]."""
    if gt.dim() != 4 or gt.shape[0] != N or gt.shape[1] != 2 or tuple(valid.shape) != (N, *gt.shape[2:]):
        raise ValueError(f"{name}: gt {tuple(gt.shape)}, valid {tuple(valid.shape)} for a batch of {N}")
    return gt.shape[2], gt.shape[3]


def _upsample_loss_args(name, flow, mask, gt, valid):
    N, C, h, w = flow.shape
    if C != 2 or tuple(mask.shape) != (N, 576, h, w):
        raise ValueError(f"{name}: flow {tuple(flow.shape)}, mask {tuple(mask.shape)}")
    H, W = _loss_frame(name, gt, valid, N)
    if not (0 < H <= 8 * h and 0 < W <= 8 * w):
        raise ValueError(f"{name}: a {H}x{W} loss frame does not lie in the {8 * h}x{8 * w} prediction")
    return N, h, w, H, W


def upsample_loss(flow, mask, gt, valid, max_flow, want_metrics):
    """corr_upsample_loss: flow [N, 2, h, w], mask [N, 576, h, w], gt [N, 2, H, W], valid [N, H, W]
    -> the six fp64 words (include/corr_mi355x_train.h) of the prediction's last H rows and W columns."""
    N, h, w, H, W = _upsample_loss_args("upsample_loss", flow, mask, gt, valid)
    lib = load()
    out = torch.empty(6, dtype=torch.float64, device=flow.device)
    ws = torch.empty((lib.corr_upsample_loss_workspace(N, h, w) + 7) // 8, dtype=torch.float64, device=flow.device)
    with torch.cuda.device(flow.device):
        _check(lib.corr_upsample_loss(_dev(flow, "flow"), _dev(mask, "mask"), _dev(gt, "gt"), _dev(valid, "valid"),
                                      N, h, w, H, W, float(max_flow), int(bool(want_metrics)), out.data_ptr(),
                                      ws.data_ptr(), ws.numel() * 8, _stream(flow)))
    return out


def upsample_loss_bwd(flow, mask, gt, valid, scale, max_flow):
    """corr_upsample_loss_bwd: scale is a one-element fp32 device tensor -> (dflow, dmask)."""
    N, h, w, H, W = _upsample_loss_args("upsample_loss_bwd", flow, mask, gt, valid)
    if scale.numel() != 1:
        raise ValueError(f"upsample_loss_bwd: scale must hold one float (got {tuple(scale.shape)})")
    lib = load()
    dflow, dmask = torch.empty_like(flow), torch.empty_like(mask)
    ws = torch.empty((lib.corr_upsample_loss_workspace(N, h, w) + 7) // 8, dtype=torch.float64, device=flow.device)
    with torch.cuda.device(flow.device):
        _check(lib.corr_upsample_loss_bwd(_dev(flow, "flow"), _dev(mask, "mask"), _dev(gt, "gt"), _dev(valid, "valid"),
                                          _dev(scale, "scale"), N, h, w, H, W, float(max_flow), _dev(dflow, "dflow"),
                                          _dev(dmask, "dmask"), ws.data_ptr(), ws.numel() * 8, _stream(flow)))
    return dflow, dmask


def sequence_loss(pred, gt, valid, max_flow, want_metrics):
    """corr_sequence_loss: pred, gt [N, 2, H, W], valid [N, H, W] -> the six fp64 words."""
    N = pred.shape[0]
    H, W = _loss_frame("sequence_loss", gt, valid, N)
    if pred.shape != gt.shape:
        raise ValueError(f"sequence_loss: pred {tuple(pred.shape)}, gt {tuple(gt.shape)}")
    lib = load()
    out = torch.empty(6, dtype=torch.float64, device=pred.device)
    ws = torch.empty((lib.corr_sequence_loss_workspace(N, H, W) + 7) // 8, dtype=torch.float64, device=pred.device)
    with torch.cuda.device(pred.device):
        _check(lib.corr_sequence_loss(_dev(pred, "pred"), _dev(gt, "gt"), _dev(valid, "valid"), N, H, W,
                                      float(max_flow), int(bool(want_metrics)), out.data_ptr(), ws.data_ptr(),
                                      ws.numel() * 8, _stream(pred)))
    return out


def sequence_loss_bwd(pred, gt, valid, scale, max_flow):
    """corr_sequence_loss_bwd: -> dpred = scale v sign(pred - gt)."""
    N = pred.shape[0]
    H, W = _loss_frame("sequence_loss_bwd", gt, valid, N)
    if pred.shape != gt.shape or scale.numel() != 1:
        raise ValueError(f"sequence_loss_bwd: pred {tuple(pred.shape)}, gt {tuple(gt.shape)}, scale {tuple(scale.shape)}")
    dpred = torch.empty_like(pred)
    with torch.cuda.device(pred.device):
        _check(load().corr_sequence_loss_bwd(_dev(pred, "pred"), _dev(gt, "gt"), _dev(valid, "valid"),
                                             _dev(scale, "scale"), N, H, W, float(max_flow), _dev(dpred, "dpred"),
                                             _stream(pred)))
    return dpred


def voxel_grid(x, y, t, p, out, normalize):
    """corr_voxel_grid: float32 device event arrays (x, y, t, p) -> out [C, H, W]."""
    C, H, W = out.shape
    M = x.numel()
    for v, nm in ((y, "y"), (t, "t"), (p, "p")):
        if v.numel() != M:
            raise ValueError(f"{nm} has {v.numel()} events, x has {M}")
    ptrs = [_dev(v, nm) if M else 0 for v, nm in ((x, "x"), (y, "y"), (t, "t"), (p, "p"))]
    o = _dev(out, "out")
    lib = load()
    n = lib.corr_voxel_grid_workspace(M, C, H, W)
    ws = torch.empty(max(1, (n + 3) // 4), dtype=torch.int32, device=out.device)
    with torch.cuda.device(out.device):
        _check(lib.corr_voxel_grid(*ptrs, M, C, H, W, int(bool(normalize)), o, ws.data_ptr(), ws.numel() * 4,
                                   _stream(out)))


def voxel_grid_tbilinear(events, out, normalize):
    """corr_voxel_grid_tbilinear: float64 device events [M, 4] (t, x, y, p) -> out [C, H, W]."""
    C, H, W = out.shape
    if events.dim() != 2 or events.shape[1] != 4:
        raise ValueError(f"events must be [M, 4] (t, x, y, p) (got {tuple(events.shape)})")
    if events.device.type != "cuda":
        raise RuntimeError(f"events is on {events.device}: eraft_amd runs only on an MI355X (HIP) device")
    if events.dtype != torch.float64 or not events.is_contiguous():
        raise TypeError("events must be a contiguous float64 tensor")
    M = events.shape[0]
    o = _dev(out, "out")
    lib = load()
    n = lib.corr_voxel_grid_tbilinear_workspace(M, C, H, W)
    ws = torch.empty(max(1, (n + 3) // 4), dtype=torch.int32, device=out.device)
    with torch.cuda.device(out.device):
        _check(lib.corr_voxel_grid_tbilinear(events.data_ptr() if M else 0, M, C, H, W, int(bool(normalize)), o,
                                             ws.data_ptr(), ws.numel() * 4, _stream(out)))


def lookup_conv_weights(weight):
    """corr_lookup_conv_weights: convc1.weight [256, C(, 1, 1)] -> the packed split (an opaque buffer)."""
    w = weight.detach().reshape(weight.shape[0], -1).contiguous().float()
    lib = load()
    packed = _new_pack(lib.corr_lookup_conv_weights_bytes(), w.device)
    with torch.cuda.device(w.device):
        _check(lib.corr_lookup_conv_weights(_dev(w, "weight"), w.shape[0], w.shape[1], packed.data_ptr(),
                                            _stream(w)))
    return packed


def lookup_conv(levels, coords, radius, packed, bias, out, relu=True, precision=0):
    """corr_lookup_conv_prec: fused lookup + 1x1 conv (+ReLU) -> out [B, 256, H, W].  precision is a
    CORR_PREC_* value (precision.py; 0 = bf16x6 is corr_lookup_conv itself, bit for bit)."""
    B, _, H, W = coords.shape
    pp, c = _ptrs(levels, "pyr"), _dev(coords, "coords")
    _check_levels(levels, B * H * W, H, W, "pyr")
    pw, bs, o = _dev(packed, "packed_weight"), _dev(bias, "bias"), _dev(out, "out")
    with torch.cuda.device(coords.device):
        _check(load().corr_lookup_conv_prec(pp, c, B, H, W, len(levels), radius, pw, bs, int(bool(relu)), o,
                                            int(precision), _stream(coords)))


def lookup_conv_bwd(levels, coords, radius, packed, out, relu, grad_out, grad_weight=None, grad_bias=None,
                    grad_lookup=None):
    """corr_lookup_conv_bwd: the fused lookup + conv's backward.  grad_weight [256, C] /
    grad_bias [256] / grad_lookup [B, C, H, W] (fp32, contiguous; None = not computed) are
    overwritten."""
    B, _, H, W = coords.shape
    lib = load()
    pp, c = _ptrs(levels, "pyr"), _dev(coords, "coords")
    _check_levels(levels, B * H * W, H, W, "pyr")
    g = _dev(grad_out, "grad_out")
    o = _dev(out, "out") if relu else None
    opt = lambda t, name: None if t is None else _dev(t, name)
    ws, nbytes = None, 0
    if grad_weight is not None or grad_bias is not None:
        nbytes = lib.corr_lookup_conv_bwd_workspace(B, H, W, len(levels))
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=coords.device)
    with torch.cuda.device(coords.device):
        _check(lib.corr_lookup_conv_bwd(pp, c, B, H, W, len(levels), radius, _dev(packed, "packed_weight"), o,
                                        int(bool(relu)), g, opt(grad_weight, "grad_weight"),
                                        opt(grad_bias, "grad_bias"), opt(grad_lookup, "grad_lookup"),
                                        None if ws is None else ws.data_ptr(), nbytes, _stream(coords)))


ONDEMAND_GENERAL = 1  # corr_ondemand_lookup flag: the general path for every workgroup


def ondemand_workspace(B, D, H, W, levels, device):
    """A device workspace for corr_ondemand_prepare / _lookup (the pixel-major operands)."""
    n = load().corr_ondemand_workspace(B, D, H, W, levels)
    if n == 0:
        raise CorrError(CORR_EINVAL, f"corr_ondemand_workspace: unsupported sizes B={B} D={D} {H}x{W}, {levels} levels")
    return torch.empty((n + 3) // 4, dtype=torch.float32, device=device)


def ondemand_prepare(fmap1, fmap2, levels, workspace):
    """corr_ondemand_prepare: fmap1 / fmap2 [B, D, H, W] -> the workspace's pixel-major rows of
    fmap1 and of fmap2 pooled 0 .. levels-1 times."""
    B, D, H, W = fmap2.shape
    a, b, ws = _dev(fmap1, "fmap1"), _dev(fmap2, "fmap2"), _dev(workspace, "workspace")
    with torch.cuda.device(fmap1.device):
        _check(load().corr_ondemand_prepare(a, b, B, D, H, W, levels, ws, workspace.numel() * 4, _stream(fmap1)))


def ondemand_lookup(workspace, coords, D, levels, radius, out, flags=0):
    """corr_ondemand_lookup: coords [B, 2, H, W] -> out [B, levels*K, H, W] from a prepared
    workspace of the same B, D, H, W, levels."""
    B, _, H, W = coords.shape
    ws, c, o = _dev(workspace, "workspace"), _dev(coords, "coords"), _dev(out, "out")
    lib = load()
    if workspace.numel() * 4 < lib.corr_ondemand_workspace(B, D, H, W, levels):
        raise ValueError("workspace is smaller than corr_ondemand_workspace for these sizes")
    K = (2 * radius + 1) ** 2
    if out.numel() != B * levels * K * H * W:
        raise ValueError(f"out has {out.numel()} floats, the lookup writes {B}x{levels * K}x{H * W}")
    with torch.cuda.device(coords.device):
        _check(lib.corr_ondemand_lookup(ws, c, B, D, H, W, levels, radius, flags, o, _stream(coords)))


def ondemand_lookup_conv(workspace, coords, D, levels, radius, packed, bias, out, relu=True, flags=0):
    """corr_ondemand_lookup_conv: coords [B, 2, H, W] -> out [B, 256, H, W] = relu(convc1(the on-demand
    lookup)) from a prepared workspace of the same B, D, H, W, levels and lookup_conv_weights' pack,
    in one launch."""
    B, _, H, W = coords.shape
    lib = load()
    # sizes first: they need no device, and a short buffer must never reach the kernel
    if workspace.numel() * 4 < lib.corr_ondemand_workspace(B, D, H, W, levels):
        raise ValueError("workspace is smaller than corr_ondemand_workspace for these sizes")
    if out.numel() != B * 256 * H * W:
        raise ValueError(f"out has {out.numel()} floats, the fused lookup writes {B}x256x{H * W}")
    ws, c, o = _dev(workspace, "workspace"), _dev(coords, "coords"), _dev(out, "out")
    pw = _pack_arg(packed, lib.corr_lookup_conv_weights_bytes(), coords.device, "corr_ondemand_lookup_conv")
    bs = _bias_arg(bias, 256, coords.device, optional=False)
    with torch.cuda.device(coords.device):
        _check(lib.corr_ondemand_lookup_conv(ws, c, B, D, H, W, levels, radius, flags, pw, bs, int(bool(relu)), o,
                                             _stream(coords)))


def ondemand_bwd_workspace(B, D, H, W, levels, radius, device):
    """A device workspace for corr_ondemand_backward (accumulator rows + one lookup's window blocks)."""
    n = load().corr_ondemand_bwd_workspace(B, D, H, W, levels, radius)
    if n == 0:
        raise CorrError(CORR_EINVAL, f"corr_ondemand_bwd_workspace: unsupported sizes B={B} D={D} {H}x{W}, "
                                     f"{levels} levels, radius {radius}")
    return torch.empty((n + 3) // 4, dtype=torch.float32, device=device)


def ondemand_backward(fwd_workspace, coords_list, grad_list, D, levels, radius, bwd_workspace=None, want1=True,
                      want2=True):
    """corr_ondemand_backward: (dfmap1, dfmap2) [B, D, H, W] of one prepared workspace and its lookups
    (coords_list[t] [B, 2, H, W], grad_list[t] [B, levels*K, H, W], in order).  A side that is not
    wanted is skipped and returned as None."""
    if len(coords_list) != len(grad_list) or not coords_list:
        raise ValueError("coords_list and grad_list must hold the same number (>= 1) of lookups")
    if not (want1 or want2):
        raise ValueError("at least one of dfmap1 / dfmap2 must be wanted")
    B, _, H, W = coords_list[0].shape
    K = (2 * radius + 1) ** 2
    for c, g in zip(coords_list, grad_list):
        if tuple(c.shape) != (B, 2, H, W) or tuple(g.shape) != (B, levels * K, H, W):
            raise ValueError(f"lookup shapes {tuple(c.shape)} / {tuple(g.shape)} do not match "
                             f"[{B}, 2, {H}, {W}] / [{B}, {levels * K}, {H}, {W}]")
    lib = load()
    fws = _dev(fwd_workspace, "fwd_workspace")
    if fwd_workspace.numel() * 4 < lib.corr_ondemand_workspace(B, D, H, W, levels):
        raise ValueError("fwd_workspace is smaller than corr_ondemand_workspace for these sizes")
    if bwd_workspace is None:
        bwd_workspace = ondemand_bwd_workspace(B, D, H, W, levels, radius, fwd_workspace.device)
    bws = _dev(bwd_workspace, "bwd_workspace")
    need = lib.corr_ondemand_bwd_workspace(B, D, H, W, levels, radius)
    if need == 0 or bwd_workspace.numel() * 4 < need:
        raise ValueError("bwd_workspace is smaller than corr_ondemand_bwd_workspace for these sizes")
    cp, gp = _ptrs(coords_list, "coords"), _ptrs(grad_list, "grads")
    dev = fwd_workspace.device
    df1 = torch.empty((B, D, H, W), dtype=torch.float32, device=dev) if want1 else None
    df2 = torch.empty((B, D, H, W), dtype=torch.float32, device=dev) if want2 else None
    with torch.cuda.device(dev):
        _check(lib.corr_ondemand_backward(fws, cp, gp, len(coords_list), B, D, H, W, levels, radius, bws,
                                          bwd_workspace.numel() * 4, None if df1 is None else df1.data_ptr(),
                                          None if df2 is None else df2.data_ptr(), _stream(fwd_workspace)))
    return df1, df2


def gru_pack_weights(wz, wr, wq):
    """corr_gru_pack_weights: the three gate weights [hidden, C, 1, 5] or [hidden, C, 5, 1] (each
    [hidden][C][5] when contiguous) -> the packed split (an opaque buffer)."""
    ws = [w.detach().contiguous().float() for w in (wz, wr, wq)]
    hidden, C = ws[0].shape[0], ws[0].shape[1]
    for w in ws:
        if w.dim() != 4 or w.shape[0] != hidden or w.shape[1] != C or w.shape[2] * w.shape[3] != 5:
            raise ValueError(f"GRU gate weights must be [hidden, C, 1, 5] or [hidden, C, 5, 1] "
                             f"(got {[tuple(v.shape) for v in ws]})")
    return _pack_weights(dict(zip(("wz", "wr", "wq"), ws)), "corr_gru_weights_bytes", "corr_gru_pack_weights",
                         (hidden, C - hidden), f"hidden = {hidden}, C = {C}")


def gru_half_step(h, x, direction, packed, bz, br, bq, workspace=None, precision=0):
    """corr_gru_half_step_prec: h [B, hidden, H, W], x [B, input, H, W] -> the new h (allocated
    here).  direction 0 = the 1x5 gates, 1 = the 5x1 ones; packed from gru_pack_weights; precision
    a CORR_PREC_* value (precision.py; 0 = bf16x6 is corr_gru_half_step itself, bit for bit)."""
    B, hidden, H, W = h.shape
    if x.dim() != 4 or x.shape[0] != B or tuple(x.shape[2:]) != (H, W):
        raise ValueError(f"x {tuple(x.shape)} does not match h {tuple(h.shape)}")
    lib = load()
    hp, xp, pk = _dev(h, "h"), _dev(x, "x"), _dev(packed, "packed")
    need = lib.corr_gru_workspace(B, hidden, H, W)
    if workspace is None:
        workspace = torch.empty((need + 3) // 4, dtype=torch.float32, device=h.device)
    out = torch.empty_like(h)
    with torch.cuda.device(h.device):
        _check(lib.corr_gru_half_step_prec(hp, xp, B, hidden, x.shape[1], H, W, direction, pk, _dev(bz, "bz"),
                                           _dev(br, "br"), _dev(bq, "bq"), _dev(workspace, "workspace"),
                                           workspace.numel() * 4, out.data_ptr(), int(precision), _stream(h)))
    return out


def conv_pack_weights(weights):
    """corr_conv_pack_weights: one Conv2d weight [cout, cin, 3, 3], or a list of them with equal
    cin that are stacked along cout (their convolutions then run as one launch) -> the packed
    split (an opaque buffer)."""
    ws = [weights] if isinstance(weights, torch.Tensor) else list(weights)
    if not ws:
        raise ValueError("conv_pack_weights needs at least one weight")
    for w in ws:
        if not isinstance(w, torch.Tensor):
            raise TypeError("conv weights must be torch.Tensors")
        if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[1] != ws[0].shape[1]:
            raise ValueError(f"conv weights must be [cout, cin, 3, 3] with equal cin "
                             f"(got {[tuple(v.shape) for v in ws]})")
    ws = [w.detach().float() for w in ws]
    w = (ws[0] if len(ws) == 1 else torch.cat(ws, dim=0)).contiguous()
    cout, cin = w.shape[0], w.shape[1]
    return _pack_weights(w, "corr_conv_weights_bytes", "corr_conv_pack_weights", (cout, cin),
                         f"cout = {cout}, cin = {cin}")


def conv_forward(in_a, in_b, packed, bias, cout, relu, out=None, out_offset=0, precision=0):
    """corr_conv_forward_prec: the 3x3 convolution (+ bias, + ReLU) of cat([in_a, in_b]) (in_b may
    be None) with the pack of conv_pack_weights, written into channels out_offset .. + cout - 1 of
    `out` [B, out_channels, H, W] (allocated as [B, cout, H, W] when None).  Returns `out`.
    precision is a CORR_PREC_* value (precision.py; 0 = bf16x6 is corr_conv_forward itself, bit for
    bit)."""
    ap = _dev(in_a, "in_a")
    if in_a.dim() != 4:
        raise ValueError(f"in_a must be [B, ca, H, W] (got {tuple(in_a.shape)})")
    B, ca, H, W = in_a.shape
    cb, bp = 0, None
    if in_b is not None:
        bp = _dev(in_b, "in_b")
        if in_b.dim() != 4 or in_b.shape[0] != B or tuple(in_b.shape[2:]) != (H, W):
            raise ValueError(f"in_b {tuple(in_b.shape)} does not match in_a {tuple(in_a.shape)}")
        if in_b.device != in_a.device:
            raise ValueError("in_a and in_b are on different devices")
        cb = in_b.shape[1]
    lib = load()
    need = lib.corr_conv_weights_bytes(cout, ca + cb)
    if need == 0:
        raise CorrError(CORR_EUNSUPPORTED, f"corr_conv_forward: unsupported cout = {cout}, ca = {ca}, cb = {cb}")
    pk = _pack_arg(packed, need, in_a.device, "the convolution")
    biasp = _bias_arg(bias, cout, in_a.device)
    if out is None:
        if out_offset != 0:
            raise ValueError("out_offset needs an out tensor")
        out = torch.empty((B, cout, H, W), dtype=torch.float32, device=in_a.device)
    op = _window_arg(out, "out", B, H, W, out_offset, cout, in_a.device)
    with torch.cuda.device(in_a.device):
        _check(lib.corr_conv_forward_prec(ap, ca, bp, cb, B, H, W, pk, biasp, cout, int(bool(relu)), op,
                                          out.shape[1], out_offset, int(precision), _stream(in_a)))
    return out


def mask_upsample_pack_weights(w):
    """corr_mask_upsample_pack_weights: the mask head's 1x1 Conv2d weight [576, 256, 1, 1] (or
    [576, 256]) -> the packed split (an opaque buffer)."""
    if not isinstance(w, torch.Tensor):
        raise TypeError("w must be a torch.Tensor")
    if tuple(w.shape) not in ((576, 256, 1, 1), (576, 256)):
        raise ValueError(f"w must be [576, 256, 1, 1] (got {tuple(w.shape)})")
    return _pack_weights(w.detach().float().contiguous(), "corr_mask_upsample_weights_bytes",
                         "corr_mask_upsample_pack_weights", (), "")


def mask_upsample_forward(hidden, hidden_offset, flow, packed, bias, scale, out=None, precision=0):
    """corr_mask_upsample_forward_prec: the convex upsampling of flow [B, 2, H, W] by the mask
    scale * (W hidden[:, hidden_offset:hidden_offset + 256] + bias), with the pack of
    mask_upsample_pack_weights and bias [576] -> out [B, 2, 8H, 8W] (allocated when None).  The
    mask itself is never stored.  precision is a CORR_PREC_* value (precision.py; 0 = bf16x6 is
    corr_mask_upsample_forward itself, bit for bit).  Returns `out`."""
    hp = _dev(hidden, "hidden")
    if hidden.dim() != 4:
        raise ValueError(f"hidden must be [B, C, H, W] (got {tuple(hidden.shape)})")
    B, hc, H, W = hidden.shape
    hidden_offset = int(hidden_offset)
    if hidden_offset < 0 or hidden_offset + 256 > hc:
        raise ValueError(f"hidden {tuple(hidden.shape)} does not hold channels {hidden_offset} .. "
                         f"{hidden_offset + 255}")
    fp = _dev(flow, "flow")
    if tuple(flow.shape) != (B, 2, H, W) or flow.device != hidden.device:
        raise ValueError(f"flow must be [{B}, 2, {H}, {W}] on {hidden.device} (got {tuple(flow.shape)} on "
                         f"{flow.device})")
    lib = load()
    need = lib.corr_mask_upsample_weights_bytes()
    pk = _pack_arg(packed, need, hidden.device, "the mask head")
    bp = _bias_arg(bias, 576, hidden.device, optional=False)
    if out is None:
        out = torch.empty((B, 2, 8 * H, 8 * W), dtype=torch.float32, device=hidden.device)
    op = _dev(out, "out")
    if tuple(out.shape) != (B, 2, 8 * H, 8 * W) or out.device != hidden.device:
        raise ValueError(f"out must be [{B}, 2, {8 * H}, {8 * W}] on {hidden.device} (got {tuple(out.shape)})")
    with torch.cuda.device(hidden.device):
        _check(lib.corr_mask_upsample_forward_prec(hp, hc, hidden_offset, fp, pk, bp, float(scale), B, H, W, op,
                                                   int(precision), _stream(hidden)))
    return out


def _mask_loss_args(name, hidden, hidden_offset, flow, packed, bias, gt, valid):
    """The sizes and pointers that corr_mask_upsample_loss and its backward share."""
    if not isinstance(hidden, torch.Tensor) or hidden.dim() != 4:
        raise ValueError(f"{name}: hidden must be a tensor [N, C, h, w]")
    N, hc, h, w = hidden.shape
    hidden_offset = int(hidden_offset)
    hp = _window_arg(hidden, "hidden", N, h, w, hidden_offset, 256, hidden.device)
    fp = _dev(flow, "flow")
    if tuple(flow.shape) != (N, 2, h, w) or flow.device != hidden.device:
        raise ValueError(f"{name}: flow must be [{N}, 2, {h}, {w}] on {hidden.device} (got {tuple(flow.shape)} on "
                         f"{flow.device})")
    H, W = _loss_frame(name, gt, valid, N)
    if not (0 < H <= 8 * h and 0 < W <= 8 * w):
        raise ValueError(f"{name}: a {H}x{W} loss frame does not lie in the {8 * h}x{8 * w} prediction")
    lib = load()
    pk = _pack_arg(packed, lib.corr_mask_upsample_weights_bytes(), hidden.device, "the mask head")
    bp = _bias_arg(bias, 576, hidden.device, optional=False)
    ws = torch.empty((lib.corr_mask_upsample_loss_workspace(N, h, w) + 7) // 8, dtype=torch.float64,
                     device=hidden.device)
    return lib, (hp, hc, hidden_offset, fp, pk, bp), (_dev(gt, "gt"), _dev(valid, "valid")), (N, h, w, H, W), ws


def mask_upsample_loss(hidden, hidden_offset, flow, packed, bias, scale, gt, valid, max_flow, want_metrics):
    """corr_mask_upsample_loss: the six fp64 words (include/corr_mi355x_train.h) of the prediction
    that mask_upsample_forward would store for the same inputs, cropped to gt's H x W."""
    lib, head, frame, dims, ws = _mask_loss_args("mask_upsample_loss", hidden, hidden_offset, flow, packed, bias, gt,
                                                 valid)
    out = torch.empty(6, dtype=torch.float64, device=hidden.device)
    with torch.cuda.device(hidden.device):
        _check(lib.corr_mask_upsample_loss(*head, float(scale), *frame, *dims, float(max_flow),
                                           int(bool(want_metrics)), out.data_ptr(), ws.data_ptr(), ws.numel() * 8,
                                           _stream(hidden)))
    return out


def mask_upsample_loss_bwd(hidden, hidden_offset, flow, packed, bias, scale, gt, valid, grad_scale, max_flow):
    """corr_mask_upsample_loss_bwd: grad_scale is a one-element fp32 device tensor -> (dflow, dz),
    dz [N, 576, h, w] the gradient of the head's convolution output."""
    lib, head, frame, dims, ws = _mask_loss_args("mask_upsample_loss_bwd", hidden, hidden_offset, flow, packed, bias,
                                                 gt, valid)
    if grad_scale.numel() != 1:
        raise ValueError(f"mask_upsample_loss_bwd: scale must hold one float (got {tuple(grad_scale.shape)})")
    N, h, w = dims[:3]
    dflow = torch.empty_like(flow)
    dz = torch.empty((N, 576, h, w), dtype=torch.float32, device=hidden.device)
    with torch.cuda.device(hidden.device):
        _check(lib.corr_mask_upsample_loss_bwd(*head, float(scale), *frame, _dev(grad_scale, "scale"), *dims,
                                               float(max_flow), _dev(dflow, "dflow"), _dev(dz, "dz"), ws.data_ptr(),
                                               ws.numel() * 8, _stream(hidden)))
    return dflow, dz


def flow_enc_pack_weights(w):
    """corr_flow_enc_pack_weights: a Conv2d weight [cout, 2, 7, 7] -> the packed split (an opaque
    buffer)."""
    if not isinstance(w, torch.Tensor):
        raise TypeError("w must be a torch.Tensor")
    if w.dim() != 4 or tuple(w.shape[1:]) != (2, 7, 7):
        raise ValueError(f"w must be [cout, 2, 7, 7] (got {tuple(w.shape)})")
    return _pack_weights(w.detach().float().contiguous(), "corr_flow_enc_weights_bytes",
                         "corr_flow_enc_pack_weights", (w.shape[0],), f"cout = {w.shape[0]}")


def flow_enc_forward(flow, packed, bias, cout, relu, out=None, out_offset=0, flow_copy=None, copy_offset=0):
    """corr_flow_enc_forward: the 7x7 convolution (+ bias, + ReLU) of flow [B, 2, H, W] with the
    pack of flow_enc_pack_weights, written into channels out_offset .. + cout - 1 of `out`
    [B, out_channels, H, W] (allocated as [B, cout, H, W] when None).  With `flow_copy`
    [B, copy_channels, H, W] the flow is also copied into its channels copy_offset, + 1.
    Returns `out`."""
    fp = _dev(flow, "flow")
    if flow.dim() != 4 or flow.shape[1] != 2:
        raise ValueError(f"flow must be [B, 2, H, W] (got {tuple(flow.shape)})")
    B, _, H, W = flow.shape
    lib = load()
    need = lib.corr_flow_enc_weights_bytes(cout)
    if need == 0:
        raise CorrError(CORR_EUNSUPPORTED, f"corr_flow_enc_forward: unsupported cout = {cout}")
    pk = _pack_arg(packed, need, flow.device, "the convolution")
    biasp = _bias_arg(bias, cout, flow.device)
    if out is None:
        if out_offset != 0:
            raise ValueError("out_offset needs an out tensor")
        out = torch.empty((B, cout, H, W), dtype=torch.float32, device=flow.device)
    op = _window_arg(out, "out", B, H, W, out_offset, cout, flow.device)
    cp, cc = None, 0
    if flow_copy is not None:
        cp, cc = _window_arg(flow_copy, "flow_copy", B, H, W, copy_offset, 2, flow.device), flow_copy.shape[1]
    elif copy_offset != 0:
        raise ValueError("copy_offset needs a flow_copy tensor")
    with torch.cuda.device(flow.device):
        _check(lib.corr_flow_enc_forward(fp, B, H, W, pk, biasp, cout, int(bool(relu)), op, out.shape[1], out_offset,
                                         cp, cc, copy_offset, _stream(flow)))
    return out


def flow_head_pack_weights(w):
    """corr_flow_head_pack_weights: the flow head's second Conv2d weight [2, 256, 3, 3] -> the packed
    split (an opaque buffer)."""
    if not isinstance(w, torch.Tensor):
        raise TypeError("w must be a torch.Tensor")
    if tuple(w.shape) != (2, 256, 3, 3):
        raise ValueError(f"w must be [2, 256, 3, 3] (got {tuple(w.shape)})")
    return _pack_weights(w.detach().float().contiguous(), "corr_flow_head_weights_bytes",
                         "corr_flow_head_pack_weights", (), "")


def flow_head_forward(hidden, hidden_offset, packed, bias, coords_in=None, coords0=None, delta=None,
                      coords_out=None, flow_out=None):
    """corr_flow_head_forward: delta = the 3x3 convolution (+ bias) of hidden[:, hidden_offset:
    hidden_offset + 256] (read in place) with the pack of flow_head_pack_weights; with `coords_in`
    also coords_out = coords_in + delta, and with `coords0` as well flow_out = coords_out - coords0.
    All of these are [B, 2, H, W]; the outputs are allocated when None and must not alias an
    input.  Returns (delta, coords_out, flow_out), None for what was not asked for."""
    hp = _dev(hidden, "hidden")
    if hidden.dim() != 4:
        raise ValueError(f"hidden must be [B, C, H, W] (got {tuple(hidden.shape)})")
    B, hc, H, W = hidden.shape
    hidden_offset = int(hidden_offset)
    if hidden_offset < 0 or hidden_offset + 256 > hc:
        raise ValueError(f"hidden {tuple(hidden.shape)} does not hold channels {hidden_offset} .. "
                         f"{hidden_offset + 255}")
    lib = load()
    need = lib.corr_flow_head_weights_bytes()
    pk = _pack_arg(packed, need, hidden.device, "the flow head")
    bp = _bias_arg(bias, 2, hidden.device, optional=False)
    if coords0 is not None and coords_in is None:
        raise ValueError("coords0 needs coords_in")

    def two(t, name, make):
        if t is None:
            if not make:
                return None, None
            t = torch.empty((B, 2, H, W), dtype=torch.float32, device=hidden.device)
        p = _dev(t, name)
        if tuple(t.shape) != (B, 2, H, W) or t.device != hidden.device:
            raise ValueError(f"{name} must be [{B}, 2, {H}, {W}] on {hidden.device} (got {tuple(t.shape)} on "
                             f"{t.device})")
        return t, p

    _, cip = two(coords_in, "coords_in", False)
    _, c0p = two(coords0, "coords0", False)
    delta, dp = two(delta, "delta", True)
    coords_out, cop = two(coords_out, "coords_out", coords_in is not None)
    flow_out, fop = two(flow_out, "flow_out", coords0 is not None)
    # (an output whose input is missing is passed on as it is: the library leaves it untouched)
    with torch.cuda.device(hidden.device):
        _check(lib.corr_flow_head_forward(hp, hc, hidden_offset, B, H, W, pk, bp, cip, c0p, dp, cop, fop,
                                          _stream(hidden)))
    return delta, coords_out if coords_in is not None else None, flow_out if coords0 is not None else None


def _enc_norm(scale, shift, B, C, device, name):
    """(scale ptr, shift ptr, norm_per_batch) of a [B, C] (per batch item) or [C] (per channel)
    pair of fp32 tensors."""
    sp, hp = _dev(scale, f"{name}_scale"), _dev(shift, f"{name}_shift")
    if scale.shape != shift.shape or tuple(scale.shape) not in ((B, C), (C,)) or scale.device != device \
            or shift.device != device:
        raise ValueError(f"{name}_scale / {name}_shift must both be [{B}, {C}] or [{C}] on {device} "
                         f"(got {tuple(scale.shape)}, {tuple(shift.shape)})")
    return sp, hp, int(scale.dim() == 2)


def enc_conv_forward(x, packed, bias, cout, stride=1, in_scale=None, in_shift=None, stats=False, precision=0):
    """corr_enc_conv_forward_prec: the 3x3 convolution (padding 1, stride 1 or 2, + bias, no ReLU) of
    x [B, cin, H, W], or of relu(x * in_scale + in_shift) when the pair ([B, cin] or [cin]) is
    given, with the pack of conv_pack_weights.  Returns out [B, cout, Ho, Wo], or (out, stats) with
    the per-tile statistics buffer for enc_norm_finalize when `stats`.  precision is a CORR_PREC_*
    value (precision.py; 0 = bf16x6 is corr_enc_conv_forward itself, bit for bit)."""
    xp = _dev(x, "x")
    if x.dim() != 4:
        raise ValueError(f"x must be [B, cin, H, W] (got {tuple(x.shape)})")
    B, cin, H, W = x.shape
    lib = load()
    need = lib.corr_conv_weights_bytes(cout, cin)
    if need == 0 or stride not in (1, 2):
        raise CorrError(CORR_EUNSUPPORTED,
                        f"corr_enc_conv_forward: unsupported cout = {cout}, cin = {cin}, stride = {stride}")
    pk = _pack_arg(packed, need, x.device, "the convolution")
    biasp = _bias_arg(bias, cout, x.device)
    if (in_scale is None) != (in_shift is None):
        raise ValueError("in_scale and in_shift must both be given or both be None")
    sp, hp, nb = (None, None, 0) if in_scale is None else _enc_norm(in_scale, in_shift, B, cin, x.device, "in")
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    st, nst = None, 0
    if stats:
        nst = lib.corr_enc_stats_bytes(B, cout, Ho, Wo)
        st = torch.empty(nst // 4, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _check(lib.corr_enc_conv_forward_prec(xp, cin, B, H, W, stride, sp, hp, nb, pk, biasp, cout, out.data_ptr(),
                                              None if st is None else st.data_ptr(), nst, int(precision),
                                              _stream(x)))
    return (out, st) if stats else out


def enc_norm_finalize(stats, B, C, Ho, Wo, eps=1e-5):
    """corr_enc_norm_finalize: the statistics of enc_conv_forward -> (scale, shift), [B, C] each:
    scale = 1 / sqrt(var + eps) (biased variance over Ho x Wo), shift = -mean * scale."""
    sp = _dev(stats, "stats")
    lib = load()
    if stats.numel() * 4 < lib.corr_enc_stats_bytes(B, C, Ho, Wo) or lib.corr_enc_stats_bytes(B, C, Ho, Wo) == 0:
        raise ValueError(f"stats holds {stats.numel() * 4} bytes, [{B}, {C}, {Ho}, {Wo}] needs "
                         f"{lib.corr_enc_stats_bytes(B, C, Ho, Wo)}")
    scale = torch.empty((B, C), dtype=torch.float32, device=stats.device)
    shift = torch.empty((B, C), dtype=torch.float32, device=stats.device)
    with torch.cuda.device(stats.device):
        _check(lib.corr_enc_norm_finalize(sp, B, C, Ho, Wo, eps, scale.data_ptr(), shift.data_ptr(), _stream(stats)))
    return scale, shift


def enc_join(y, scale, shift, skip, out=None):
    """corr_enc_join: relu(skip + relu(y * scale + shift)) for y, skip [B, C, H, W] and scale,
    shift [B, C] or [C]; into `out` (which may be y; allocated when None)."""
    yp, kp = _dev(y, "y"), _dev(skip, "skip")
    if y.dim() != 4 or skip.shape != y.shape or skip.device != y.device:
        raise ValueError(f"y and skip must be equal [B, C, H, W] tensors on one device "
                         f"(got {tuple(y.shape)}, {tuple(skip.shape)})")
    B, C, H, W = y.shape
    sp, hp, nb = _enc_norm(scale, shift, B, C, y.device, "norm")
    if out is None:
        out = torch.empty_like(y)
    op = _dev(out, "out")
    if out.shape != y.shape or out.device != y.device:
        raise ValueError(f"out {tuple(out.shape)} does not match y {tuple(y.shape)}")
    with torch.cuda.device(y.device):
        _check(load().corr_enc_join(yp, sp, hp, nb, kp, B, C, H, W, op, _stream(y)))
    return out


def _enc_front_pack(w, k, name):
    """A [cout, cin, k, k] (k = 1: or [cout, cin]) weight -> its packed split."""
    if not isinstance(w, torch.Tensor):
        raise TypeError("w must be a torch.Tensor")
    if not (w.dim() == 4 and tuple(w.shape[2:]) == (k, k)) and not (k == 1 and w.dim() == 2):
        raise ValueError(f"w must be [cout, cin, {k}, {k}] (got {tuple(w.shape)})")
    cout, cin = w.shape[0], w.shape[1]
    return _pack_weights(w.detach().float().contiguous(), f"corr_enc_{name}_weights_bytes",
                         f"corr_enc_{name}_pack_weights", (cout, cin), f"cout = {cout}, cin = {cin}")


def enc_stem_pack_weights(w):
    """corr_enc_stem_pack_weights: the stem's Conv2d weight [cout, cin, 7, 7], cin <= 16 -> the
    packed split (an opaque buffer)."""
    return _enc_front_pack(w, 7, "stem")


def enc_pw_pack_weights(w):
    """corr_enc_pw_pack_weights: a 1x1 Conv2d weight [cout, cin, 1, 1] (or [cout, cin]) -> the
    packed split (an opaque buffer)."""
    return _enc_front_pack(w, 1, "pw")


def _enc_front_forward(name, x, packed, bias, cout, stride, stats, precision):
    xp = _dev(x, "x")
    if x.dim() != 4:
        raise ValueError(f"x must be [B, cin, H, W] (got {tuple(x.shape)})")
    B, cin, H, W = x.shape
    lib = load()
    need = getattr(lib, f"corr_enc_{name}_weights_bytes")(cout, cin)
    if need == 0 or stride not in (1, 2):
        raise CorrError(CORR_EUNSUPPORTED,
                        f"corr_enc_{name}_forward: unsupported cout = {cout}, cin = {cin}, stride = {stride}")
    pk = _pack_arg(packed, need, x.device, "the convolution")
    biasp = _bias_arg(bias, cout, x.device)
    Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
    out = torch.empty((B, cout, Ho, Wo), dtype=torch.float32, device=x.device)
    st, nst = None, 0
    if stats:
        nst = lib.corr_enc_stats_bytes(B, cout, Ho, Wo)
        st = torch.empty(nst // 4, dtype=torch.float32, device=x.device)
    stp = None if st is None else st.data_ptr()
    with torch.cuda.device(x.device):
        if name == "stem":
            _check(lib.corr_enc_stem_forward_prec(xp, cin, B, H, W, pk, biasp, cout, out.data_ptr(), stp, nst,
                                                  int(precision), _stream(x)))
        else:
            _check(lib.corr_enc_pw_forward_prec(xp, cin, B, H, W, stride, pk, biasp, cout, out.data_ptr(), stp, nst,
                                                int(precision), _stream(x)))
    return (out, st) if stats else out


def enc_stem_forward(x, packed, bias, cout, stats=False, precision=0):
    """corr_enc_stem_forward_prec: the 7x7 convolution (stride 2, padding 3, + bias, no ReLU) of
    x [B, cin, H, W], cin <= 16, with the pack of enc_stem_pack_weights.  Returns out
    [B, cout, Ho, Wo], or (out, stats) with the per-tile statistics for enc_norm_finalize.
    precision: a CORR_PREC_* value (0 = bf16x6 is corr_enc_stem_forward itself, bit for bit)."""
    return _enc_front_forward("stem", x, packed, bias, cout, 2, stats, precision)


def enc_pw_forward(x, packed, bias, cout, stride=1, stats=False, precision=0):
    """corr_enc_pw_forward_prec: the 1x1 convolution (stride 1 or 2, + bias, no ReLU) of
    x [B, cin, H, W] with the pack of enc_pw_pack_weights.  Returns out [B, cout, Ho, Wo], or
    (out, stats) with the per-tile statistics for enc_norm_finalize.
    precision: a CORR_PREC_* value (0 = bf16x6 is corr_enc_pw_forward itself, bit for bit)."""
    return _enc_front_forward("pw", x, packed, bias, cout, stride, stats, precision)


def enc_join_affine(y, scale, shift, skip, skip_scale=None, skip_shift=None, skip_relu=False, out=None):
    """corr_enc_join_affine: relu(s(skip) + relu(y * scale + shift)) with s(v) = v * skip_scale +
    skip_shift (v itself when the pair is None), followed by a ReLU when `skip_relu`; y, skip
    [B, C, H, W], each pair [B, C] or [C]; into `out` (which may be y; allocated when None)."""
    yp, kp = _dev(y, "y"), _dev(skip, "skip")
    if y.dim() != 4 or skip.shape != y.shape or skip.device != y.device:
        raise ValueError(f"y and skip must be equal [B, C, H, W] tensors on one device "
                         f"(got {tuple(y.shape)}, {tuple(skip.shape)})")
    B, C, H, W = y.shape
    sp, hp, nb = _enc_norm(scale, shift, B, C, y.device, "norm")
    if (skip_scale is None) != (skip_shift is None):
        raise ValueError("skip_scale and skip_shift must both be given or both be None")
    ksp, khp, knb = (None, None, 0) if skip_scale is None else _enc_norm(skip_scale, skip_shift, B, C, y.device, "skip")
    if out is None:
        out = torch.empty_like(y)
    op = _dev(out, "out")
    if out.shape != y.shape or out.device != y.device:
        raise ValueError(f"out {tuple(out.shape)} does not match y {tuple(y.shape)}")
    with torch.cuda.device(y.device):
        _check(load().corr_enc_join_affine(yp, sp, hp, nb, kp, ksp, khp, knb, int(bool(skip_relu)), B, C, H, W, op,
                                           _stream(y)))
    return out
