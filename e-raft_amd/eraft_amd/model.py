"""Host-side E-RAFT forward around the MI355X CorrBlock (the caller of the hot path).

A restatement, in plain PyTorch, of the reference model that calls CorrBlock
(AhmedHumais/E-RAFT model/eraft.py:37-146, model/extractor.py, model/update.py,
utils/image_utils.py:85-123).  The dense convolutions stay on PyTorch-ROCm/MIOpen (out of
scope); only the correlation build and lookups go through libcorr_mi355x.so.

Module and parameter names follow the reference so that a reference checkpoint's
``state_dict`` loads unchanged (main.py:116-117: ``model.load_state_dict(ckpt['model'])``).
It exists to run the north_star's end-to-end check (flow EPE vs the reference model on
identical random weights, tests/test_e2e.py) and as the integration example.
"""
from __future__ import annotations

import os

import torch
import torch.nn as nn
import torch.nn.functional as F

from .corr import CorrBlock
from .ondemand import OnDemandConvCorrBlock, OnDemandCorrBlock
from .precision import (DEFAULT as _PRECISION, resolve as _resolve_precision, resolve_corr as _resolve_corr_precision,
                        resolve_encoder as _resolve_encoder_precision,
                        resolve_pointwise as _resolve_pointwise_precision)
from .utils import coords_grid


def _norm(kind: str, ch: int, groups: int = 8):
    if kind == "group":
        return nn.GroupNorm(num_groups=groups, num_channels=ch)
    if kind == "batch":
        return nn.BatchNorm2d(ch)
    if kind == "instance":
        return nn.InstanceNorm2d(ch)
    return nn.Sequential()


class ResidualBlock(nn.Module):
    """3x3-3x3 residual unit with an optional strided 1x1 projection (extractor.py:7-52)."""

    def __init__(self, cin, cout, norm_fn="group", stride=1):
        super().__init__()
        self.conv1 = nn.Conv2d(cin, cout, 3, padding=1, stride=stride)
        self.conv2 = nn.Conv2d(cout, cout, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)
        g = cout // 8
        self.norm1 = _norm(norm_fn, cout, g)
        self.norm2 = _norm(norm_fn, cout, g)
        if stride != 1:
            self.norm3 = _norm(norm_fn, cout, g)
            self.downsample = nn.Sequential(nn.Conv2d(cin, cout, 1, stride=stride), self.norm3)
        else:
            self.downsample = None

    def forward(self, x):
        y = self.relu(self.norm1(self.conv1(x)))
        y = self.relu(self.norm2(self.conv2(y)))
        skip = x if self.downsample is None else self.downsample(x)
        return self.relu(skip + y)


class BasicEncoder(nn.Module):
    """7x7/2 stem + three residual stages (64, 96/2, 128/2) + 1x1 head (extractor.py:137-189)."""

    def __init__(self, output_dim=128, norm_fn="batch", dropout=0.0, n_first_channels=1):
        super().__init__()
        self.norm_fn = norm_fn
        self.norm1 = _norm(norm_fn, 64)
        self.conv1 = nn.Conv2d(n_first_channels, 64, 7, stride=2, padding=3)
        self.relu1 = nn.ReLU(inplace=True)
        stages, cin = [], 64
        for cout, stride in ((64, 1), (96, 2), (128, 2)):
            stages.append(nn.Sequential(ResidualBlock(cin, cout, norm_fn, stride),
                                        ResidualBlock(cout, cout, norm_fn, 1)))
            cin = cout
        self.layer1, self.layer2, self.layer3 = stages
        self.conv2 = nn.Conv2d(128, output_dim, 1)
        self.dropout = nn.Dropout2d(p=dropout) if dropout > 0 else None
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, (nn.BatchNorm2d, nn.InstanceNorm2d, nn.GroupNorm)):
                if m.weight is not None:
                    nn.init.constant_(m.weight, 1)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ERAFT_AMD_FUSE_ENCODER=1: at inference on the MI355X the whole encoder runs on the project's
    # kernels (encoder.py): the 7x7 stem, the residual stages' 3x3 convolutions, the strided blocks'
    # 1x1 projections and the 1x1 head on the bf16x6 MFMA, every norm applied on load or in the
    # block's join, instead of MIOpen / rocBLAS convolutions and torch norm / ReLU / add kernels.
    # Default off (DESIGN §16 and §18 have the measurements); training always runs the torch code.
    fused = os.environ.get("ERAFT_AMD_FUSE_ENCODER", "0") == "1"
    # The fused convolutions' precision mode (precision.py); ERAFT sets it on its two encoders.  The
    # torch path ignores it.
    precision = _PRECISION

    def _fusable(self, x):
        """encoder.encoder_forward is built for an fp32 GPU tensor, instance norm or eval-mode
        batch norm, the reference's shapes (stem 7x7 / 2 with padding 3 to 64 channels, 3x3 stages
        of 64, 96, 128 channels, 1x1 projections and head, every convolution with a bias), and has
        no backward."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            return False
        if not (self.norm_fn == "instance" or (self.norm_fn == "batch" and not self.training)):
            return False
        if self.training and self.dropout is not None:
            return False

        def conv_is(c, shape, stride, padding):
            return (tuple(c.weight.shape) == shape and c.stride == (stride, stride) and c.padding == (padding, padding)
                    and c.dilation == (1, 1) and c.groups == 1 and c.bias is not None)

        def norm_ok(n):
            if self.norm_fn == "instance":
                return isinstance(n, nn.InstanceNorm2d) and not n.affine and not n.track_running_stats
            return isinstance(n, nn.BatchNorm2d) and n.running_mean is not None and n.running_var is not None

        if not (conv_is(self.conv1, (64, x.shape[1], 7, 7), 2, 3) and norm_ok(self.norm1)
                and conv_is(self.conv2, (self.conv2.out_channels, 128, 1, 1), 1, 0)):
            return False
        cin = 64
        for layer, cout, stride in ((self.layer1, 64, 1), (self.layer2, 96, 2), (self.layer3, 128, 2)):
            for k, blk in enumerate(layer):
                s = stride if k == 0 else 1
                if not (conv_is(blk.conv1, (cout, cin, 3, 3), s, 1) and conv_is(blk.conv2, (cout, cout, 3, 3), 1, 1)
                        and norm_ok(blk.norm1) and norm_ok(blk.norm2) and (blk.downsample is None) == (s == 1)):
                    return False
                if s != 1 and not (len(blk.downsample) == 2 and isinstance(blk.downsample[0], nn.Conv2d)
                                   and conv_is(blk.downsample[0], (cout, cin, 1, 1), s, 0)
                                   and norm_ok(blk.downsample[1])):
                    return False
                cin = cout
        ts = list(self.parameters()) + list(self.buffers())
        if any(t.device != x.device or (t.is_floating_point() and t.dtype != torch.float32) for t in ts):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in (x, *self.parameters())))

    def forward(self, x):
        pair = isinstance(x, (list, tuple))
        if pair:
            n = x[0].shape[0]
            x = torch.cat(x, dim=0)
        if self.fused and self._fusable(x):
            from .encoder import encoder_forward
            x = encoder_forward(self, x)
        else:
            x = self.relu1(self.norm1(self.conv1(x)))
            x = self.layer3(self.layer2(self.layer1(x)))
            x = self.conv2(x)
        if self.training and self.dropout is not None:
            x = self.dropout(x)
        return torch.split(x, [n, n], dim=0) if pair else x


class BasicMotionEncoder(nn.Module):
    """Consumes the lookup output: convc1 is the 324 -> 256 1x1 (update.py:63-82)."""

    def __init__(self, corr_levels=4, corr_radius=4):
        super().__init__()
        planes = corr_levels * (2 * corr_radius + 1) ** 2
        self.convc1 = nn.Conv2d(planes, 256, 1)
        self.convc2 = nn.Conv2d(256, 192, 3, padding=1)
        self.convf1 = nn.Conv2d(2, 128, 7, padding=3)
        self.convf2 = nn.Conv2d(128, 64, 3, padding=1)
        self.conv = nn.Conv2d(64 + 192, 128 - 2, 3, padding=1)

    def forward(self, flow, corr, fused=False):
        # fused: corr already is relu(convc1(lookup)) (CorrBlock.lookup_conv)
        c = F.relu(self.convc2(corr if fused else F.relu(self.convc1(corr))))
        f = F.relu(self.convf2(F.relu(self.convf1(flow))))
        return torch.cat([F.relu(self.conv(torch.cat([c, f], dim=1))), flow], dim=1)


class SepConvGRU(nn.Module):
    """Horizontal (1x5) then vertical (5x1) convolutional GRU (update.py:34-61)."""

    # ERAFT_AMD_FUSE_GRU=1: at inference on the MI355X each half step is corr_gru_half_step (two
    # HIP launches on the bf16 MFMA, gru.py) instead of the torch / MIOpen chain below.  Default
    # off (DESIGN §14 has the measurements); training always runs the torch code.
    fused = os.environ.get("ERAFT_AMD_FUSE_GRU", "0") == "1"
    # The fused half steps' precision mode (precision.py); ERAFT sets it on its instances.  The
    # torch path and training are fp32 and ignore it.
    precision = _PRECISION

    def __init__(self, hidden_dim=128, input_dim=192 + 128):
        super().__init__()
        c = hidden_dim + input_dim
        for tag, k, p in (("1", (1, 5), (0, 2)), ("2", (5, 1), (2, 0))):
            for gate in "zrq":
                setattr(self, f"conv{gate}{tag}", nn.Conv2d(c, hidden_dim, k, padding=p))

    def _step(self, h, x, tag):
        hx = torch.cat([h, x], dim=1)
        z = torch.sigmoid(getattr(self, f"convz{tag}")(hx))
        r = torch.sigmoid(getattr(self, f"convr{tag}")(hx))
        q = torch.tanh(getattr(self, f"convq{tag}")(torch.cat([r * h, x], dim=1)))
        return (1 - z) * h + z * q

    def _fusable(self, h, x):
        """The fused half steps (gru.sepconv_gru) are built for fp32 GPU tensors, hidden = 128 and
        C a multiple of 32 (<= 1024), and have no backward."""
        if not (h.is_cuda and x.is_cuda and h.dtype == x.dtype == torch.float32 and h.dim() == x.dim() == 4):
            return False
        hidden, c = h.shape[1], h.shape[1] + x.shape[1]
        if hidden != 128 or c % 32 or c > 1024 or tuple(self.convz1.weight.shape) != (hidden, c, 1, 5):
            return False
        ps = list(self.parameters())
        if len(ps) != 12 or any(p.dtype != torch.float32 or p.device != h.device for p in ps):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in (h, x, *ps)))

    def forward(self, h, x):
        if self.fused and self._fusable(h, x):
            from .gru import sepconv_gru
            return sepconv_gru(self, h, x)
        return self._step(self._step(h, x, "1"), x, "2")


class FlowHead(nn.Module):
    def __init__(self, input_dim=128, hidden_dim=256):
        super().__init__()
        self.conv1 = nn.Conv2d(input_dim, hidden_dim, 3, padding=1)
        self.conv2 = nn.Conv2d(hidden_dim, 2, 3, padding=1)
        self.relu = nn.ReLU(inplace=True)

    def forward(self, x):
        return self.conv2(self.relu(self.conv1(x)))


class BasicUpdateBlock(nn.Module):
    """Motion encoder + SepConvGRU + flow head + convex-upsampling mask (update.py:85-107)."""

    # ERAFT_AMD_FUSE_UPDATE=1: at inference on the MI355X the block's 3x3 convolutions are
    # corr_conv_forward launches that write into shared buffers (update.py: no cat, bias and ReLU
    # in the kernel) instead of MIOpen convolutions and torch glue; the flow's 7x7 convolution and
    # the flow head's 3x3 to 2 channels, with the coordinate update, are corr_flow_enc_forward and
    # corr_flow_head_forward launches.  Default off (DESIGN §15 and §19 have the measurements);
    # training always runs the torch code.
    fused = os.environ.get("ERAFT_AMD_FUSE_UPDATE", "0") == "1"
    # The fused 3x3 convolutions' precision mode (precision.py); ERAFT sets it on its instances.
    # The torch path and training are fp32 and ignore it.
    precision = _PRECISION

    def __init__(self, corr_levels=4, corr_radius=4, hidden_dim=128):
        super().__init__()
        self.encoder = BasicMotionEncoder(corr_levels, corr_radius)
        self.gru = SepConvGRU(hidden_dim=hidden_dim, input_dim=128 + hidden_dim)
        self.flow_head = FlowHead(hidden_dim, hidden_dim=256)
        self.mask = nn.Sequential(nn.Conv2d(128, 256, 3, padding=1), nn.ReLU(inplace=True),
                                  nn.Conv2d(256, 64 * 9, 1))

    def _fusable(self, net, inp, corr, flow, fused):
        """update.update_block is built for fp32 GPU tensors and the reference's channel counts,
        and has no backward."""
        ts = (net, inp, corr, flow)
        if not all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 4 and t.device == net.device for t in ts):
            return False
        enc = self.encoder
        if (net.shape[1], inp.shape[1], flow.shape[1]) != (128, 128, 2) or corr.shape[1] != (256 if fused else 324):
            return False
        shapes = ((enc.convc1, (256, 324, 1, 1)), (enc.convc2, (192, 256, 3, 3)), (enc.convf1, (128, 2, 7, 7)),
                  (enc.convf2, (64, 128, 3, 3)), (enc.conv, (126, 256, 3, 3)), (self.flow_head.conv1, (256, 128, 3, 3)),
                  (self.mask[0], (256, 128, 3, 3)))
        if any(tuple(c.weight.shape) != s or c.bias is None for c, s in shapes):
            return False
        # the flow's 7x7 and the flow head's 3x3 to 2 channels have kernels of their own (corr_flow.hip)
        for c, s, pad in ((enc.convf1, (128, 2, 7, 7), 3), (self.flow_head.conv2, (2, 256, 3, 3), 1)):
            if (tuple(c.weight.shape) != s or c.bias is None or c.padding != (pad, pad) or c.stride != (1, 1)
                    or c.dilation != (1, 1) or c.groups != 1):
                return False
        ps = list(self.parameters())
        if any(p.dtype != torch.float32 or p.device != net.device for p in ps):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in (*ts, *ps)))

    def forward(self, net, inp, corr, flow, fused=False, defer_mask=False, workspace=None, coords1=None,
                coords0=None):
        """Returns (net, mask, delta_flow).  With `defer_mask`: (net, hidden, delta_flow), hidden =
        relu(mask[0](net)) [B, 256, H, W], and mask[2] with its 0.25 is left to the caller
        (upsample.mask_upsample).  With `coords1` the refinement loop's coordinate update is part
        of the call: the result is (net, mask, delta_flow, coords1 + delta_flow, that - coords0),
        the last None without `coords0`; on the fused path the flow head's kernel writes both.
        `workspace` (update.UpdateWorkspace) keeps the fused path's buffers across iterations."""
        if self.fused and self._fusable(net, inp, corr, flow, fused):
            from .update import update_block
            return update_block(self, net, inp, corr, flow, fused, defer_mask=defer_mask, workspace=workspace,
                                coords1=coords1, coords0=coords0)
        motion = self.encoder(flow, corr, fused)
        net = self.gru(net, torch.cat([inp, motion], dim=1))
        mask = self.mask[1](self.mask[0](net)) if defer_mask else 0.25 * self.mask(net)
        delta = self.flow_head(net)
        if coords1 is None:
            return net, mask, delta
        coords1 = coords1 + delta
        return net, mask, delta, coords1, None if coords0 is None else coords1 - coords0


class ImagePadder:
    """Zero-pads top/left to a multiple of min_size (utils/image_utils.py:85-123)."""

    def __init__(self, min_size=64):
        self.min_size = min_size
        self.pad_height = self.pad_width = None

    def pad(self, image):
        h, w = image.shape[-2:]
        ph = (self.min_size - h % self.min_size) % self.min_size
        pw = (self.min_size - w % self.min_size) % self.min_size
        if self.pad_width is None:
            self.pad_height, self.pad_width = ph, pw
        elif (ph, pw) != (self.pad_height, self.pad_width):
            raise RuntimeError("ImagePadder: image size changed between calls")
        return F.pad(image, (self.pad_width, 0, self.pad_height, 0))

    def unpad(self, image):
        return image[..., self.pad_height:, self.pad_width:]


class _ConvexUpsampleFn(torch.autograd.Function):
    """ERAFT.upsample_flow on the MI355X: forward corr_convex_upsample, backward
    corr_convex_upsample_bwd (softmax and unfold backward fused; the 9x-expanded product of
    the torch composition is never materialised in either direction)."""

    @staticmethod
    def forward(ctx, flow, mask):
        from . import _lib
        n, _, h, w = flow.shape
        out = torch.empty((n, 2, 8 * h, 8 * w), dtype=torch.float32, device=flow.device)
        _lib.convex_upsample(flow, mask, out)
        ctx.save_for_backward(flow, mask)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        from . import _lib
        flow, mask = ctx.saved_tensors
        dflow, dmask = _lib.convex_upsample_bwd(flow, mask, grad_out.contiguous())
        return dflow, dmask


class ERAFT(nn.Module):
    """E-RAFT (model/eraft.py:37-146) with the MI355X CorrBlock on its hot path."""

    hidden_dim = 128
    context_dim = 128
    corr_levels = 4
    corr_radius = 4
    # lookup fused with convc1 (corr_lookup_conv, bf16x6 MFMA; in training its backward is
    # corr_lookup_conv_bwd); ERAFT_AMD_FUSE_CONV=0 keeps lookup + MIOpen convc1.  DSEC: 20.1 vs
    # 38.9 us per GRU iteration (profiles/r04k_conv_fwd_bwd_timing.jsonl)
    fuse_lookup_conv = os.environ.get("ERAFT_AMD_FUSE_CONV", "1") == "1"
    # ERAFT_AMD_FUSE_UPSAMPLE=1: at inference on the MI355X the mask head's 1x1 convolution, its
    # 0.25, the softmax over the taps and the convex combination are one corr_mask_upsample_forward
    # launch per iteration (upsample.py) and the 576-channel mask is never stored.  Default off
    # (DESIGN §17 has the measurements); training always runs the torch code.
    fuse_mask_upsample = os.environ.get("ERAFT_AMD_FUSE_UPSAMPLE", "0") == "1"
    # ERAFT_AMD_ONDEMAND_FUSE_CONV=1: with alternate_corr the block is OnDemandConvCorrBlock, whose
    # lookup_conv is one corr_ondemand_lookup_conv launch at inference (no 324-channel lookup in
    # HBM, no torch convc1); under autograd it is the unfused composition.  Default off (DESIGN §21
    # has the measurements).
    fuse_ondemand_conv = os.environ.get("ERAFT_AMD_ONDEMAND_FUSE_CONV", "0") == "1"
    # ERAFT_AMD_FUSE_MASK_LOSS=1: with a sequence_loss criterion the mask head's 1x1 convolution and
    # its 0.25 run inside the fused upsampling loss (SequenceLoss.add_hidden: corr_mask_upsample_loss
    # forward, corr_mask_upsample_loss_bwd + the convolution's backward over dz), so the 576-channel
    # mask is neither stored nor saved for backward.  Default off (DESIGN §32 has the measurements).
    fuse_mask_loss = os.environ.get("ERAFT_AMD_FUSE_MASK_LOSS", "0") == "1"
    # The precision mode of the GRU and the update block's 3x3 convolutions ("bf16x6", "bf16x3" or
    # "bf16": precision.py), that of the two encoders' convolutions, that of the correlation
    # build and that of the two fused 1x1 convolutions (lookup + convc1, the mask head); an
    # instance takes each from its config (below).
    precision = _PRECISION
    encoder_precision = _PRECISION
    corr_precision = _PRECISION
    pointwise_precision = _PRECISION

    def __init__(self, config, n_first_channels):
        super().__init__()
        self.subtype = config["subtype"].lower()
        if self.subtype not in ("standard", "warm_start"):
            raise ValueError(f"unknown subtype {self.subtype}")
        # RAFT's switch: lookups computed from the feature maps (OnDemandCorrBlock; no all-pairs
        # volume; its backward works without one too) instead of CorrBlock.  Config key, default off;
        # ERAFT_AMD_ONDEMAND=1 / =0 overrides it.
        alt = bool(config.get("alternate_corr", False)) if hasattr(config, "get") else False
        env = os.environ.get("ERAFT_AMD_ONDEMAND")
        self.alternate_corr = alt if env is None else env == "1"
        self.image_padder = ImagePadder(min_size=32)
        hdim, cdim = self.hidden_dim, self.context_dim
        self.fnet = BasicEncoder(output_dim=256, norm_fn="instance", dropout=0,
                                 n_first_channels=n_first_channels)
        self.cnet = BasicEncoder(output_dim=hdim + cdim, norm_fn="batch", dropout=0,
                                 n_first_channels=n_first_channels)
        self.update_block = BasicUpdateBlock(self.corr_levels, self.corr_radius, hidden_dim=hdim)
        # The reference's switch (model/eraft.py:102-133 puts fnet, cnet and the update block under
        # one autocast) is three knobs here, and setting all three corresponds to it:
        #   `mixed_precision` (absent / False: "bf16x6", every product exact as before; True:
        #   "bf16x3"; or a mode's name), overridden by ERAFT_AMD_PRECISION=<name>, reaches the GRU's
        #   eight convolutions and the update block's convc2, convf2, conv and the two heads' first
        #   convolutions, where their fused kernels run (ERAFT_AMD_FUSE_GRU=1 / ERAFT_AMD_FUSE_UPDATE=1);
        #   `encoder_precision` (the same values), overridden by ERAFT_AMD_ENCODER_PRECISION=<name>,
        #   reaches the 16 convolutions of fnet and the 16 of cnet (stem, 3x3 stages, 1x1 projections
        #   and head), where encoder.encoder_forward runs (ERAFT_AMD_FUSE_ENCODER=1);
        #   `pointwise_precision` (the same values), overridden by ERAFT_AMD_POINTWISE_PRECISION=<name>,
        #   reaches convc1 inside CorrBlock.lookup_conv (ERAFT_AMD_FUSE_CONV) and the mask head's 1x1
        #   convolution inside upsample.mask_upsample (ERAFT_AMD_FUSE_UPSAMPLE=1); `mixed_precision`
        #   does not set it, and the on-demand blocks never get it.
        # All act at inference only; the torch paths and training stay fp32.  convf1 and the flow
        # head's second convolution stay "bf16x6": the flow enters and leaves through them.
        # A fourth knob is the correlation build's own:
        #   `corr_precision` (the same values), overridden by ERAFT_AMD_CORR_PRECISION=<name>, reaches
        #   CorrBlock's all-pairs build (the lookups read whatever values it left in the pyramid).
        # The reference casts the feature maps to fp32 before its CorrBlock, outside the autocast, so
        # `mixed_precision` does not set it.  Inference only: a build recorded for autograd runs
        # "bf16x6" (CorrBlock.precision tells).  With `alternate_corr` the on-demand blocks compute
        # their windows on the fp32 MFMA and ignore it.
        self.precision = _resolve_precision(config)
        self.update_block.precision = self.update_block.gru.precision = self.precision
        self.encoder_precision = _resolve_encoder_precision(config)
        self.fnet.precision = self.cnet.precision = self.encoder_precision
        self.corr_precision = _resolve_corr_precision(config)
        self.pointwise_precision = _resolve_pointwise_precision(config)

    def freeze_bn(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eval()

    @staticmethod
    def upsample_flow(flow, mask):
        """Convex combination of 3x3 neighbours, x8 (eraft.py:75-86).  On the MI355X: the
        one-pass HIP kernel (corr_convex_upsample), with its HIP backward under autograd
        (_ConvexUpsampleFn); on the CPU the torch composition below (what bench.py's CPU
        baseline runs)."""
        if flow.is_cuda:
            return _ConvexUpsampleFn.apply(flow.float().contiguous(), mask.float().contiguous())
        n, _, h, w = flow.shape
        mask = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
        up = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
        up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3)
        return up.reshape(n, 2, 8 * h, 8 * w)

    def _mask_fusable(self, *ts):
        """upsample.mask_upsample is built for fp32 GPU tensors and the reference's mask head
        (256 -> 576, 1x1, with a bias), and has no backward."""
        head = self.update_block.mask[2]
        if not all(t.is_cuda and t.dtype == torch.float32 and t.device == ts[0].device for t in ts):
            return False
        if tuple(head.weight.shape) != (576, 256, 1, 1) or head.bias is None:
            return False
        ps = list(self.update_block.parameters())
        if any(p.dtype != torch.float32 or p.device != ts[0].device for p in ps):
            return False
        return not (torch.is_grad_enabled() and any(t.requires_grad for t in (*ts, *self.parameters())))

    def forward(self, image1, image2, iters=12, flow_init=None, upsample=True, sequence_loss=None):
        """`sequence_loss`: a loss.SequenceLoss.  Each iteration then hands it the 1/8-resolution
        flow and the mask (add_upsampled: on the MI355X the loss fused with the upsampling, no
        full-resolution prediction stored; the torch composition elsewhere) instead of calling
        upsample_flow; the returned list of predictions is empty and the caller reads
        sequence_loss.result().  Works under no_grad for validation.  With `fuse_mask_loss` the
        criterion gets relu(mask[0](net)) and the head mask[2] instead of the mask (add_hidden)."""
        image1 = self.image_padder.pad(image1).contiguous()
        image2 = self.image_padder.pad(image2).contiguous()
        fmap1, fmap2 = self.fnet([image1, image2])
        if self.alternate_corr:
            block = OnDemandConvCorrBlock if self.fuse_ondemand_conv else OnDemandCorrBlock
            corr_fn = block(fmap1.float(), fmap2.float(), num_levels=self.corr_levels, radius=self.corr_radius,
                            train=torch.is_grad_enabled())
        else:
            # (the default mode is passed by omission: a drop-in class with the reference's signature works)
            mode = {} if self.corr_precision == _PRECISION else {"precision": self.corr_precision}
            corr_fn = CorrBlock(fmap1.float(), fmap2.float(), num_levels=self.corr_levels, radius=self.corr_radius,
                                **mode)
        net, inp = torch.split(self.cnet(image2), [self.hidden_dim, self.context_dim], dim=1)
        net, inp = torch.tanh(net), torch.relu(inp)
        n, _, h, w = image1.shape
        coords0 = coords_grid(n, h // 8, w // 8, device=image1.device)
        coords1 = coords0.clone()
        if flow_init is not None:
            coords1 = coords1 + flow_init
        predictions = []
        # on the MI355X the lookup feeds convc1 on-chip (corr_lookup_conv), at inference and, with
        # its autograd backward (corr._LookupConvFn), in training
        fuse = (self.fuse_lookup_conv and image1.is_cuda and self.corr_radius == 4
                and hasattr(corr_fn, "lookup_conv"))
        # with ERAFT_AMD_FUSE_UPDATE=1 at inference the update block keeps its buffers in a workspace
        # made once per forward and its flow head's kernel also does the coordinate update: the loop
        # then issues no coords1 + delta and no coords1 - coords0 (flow is the kernel's flow_out)
        ub, ws, flow = self.update_block, None, None
        # (the default mode is passed by omission, as the build's; the on-demand blocks have no modes)
        pw_mask = {} if self.pointwise_precision == _PRECISION else {"precision": self.pointwise_precision}
        pw = {} if self.alternate_corr else pw_mask
        for it in range(iters):
            coords1 = coords1.detach()
            if fuse:
                enc = ub.encoder
                corr = corr_fn.lookup_conv(coords1, enc.convc1.weight, enc.convc1.bias, **pw)
            else:
                corr = corr_fn(coords1)
            if flow is None:
                flow = coords1 - coords0
            tail = ub.fused and ub._fusable(net, inp, corr, flow, fuse)
            kw = {}
            if tail:
                if ws is None:
                    from .update import UpdateWorkspace
                    ws = UpdateWorkspace(inp.detach())
                kw = {"workspace": ws, "coords1": coords1, "coords0": coords0}
            pad = (self.image_padder.pad_height, self.image_padder.pad_width)
            if sequence_loss is not None and self.fuse_mask_loss:
                # the criterion runs the mask head itself (add_hidden takes the torch composition
                # for tensors its kernels are not built for)
                net, hidden, delta, *upd = ub(net, inp, corr, flow, fuse, defer_mask=True, **kw)
                coords1, flow = upd if tail else (coords1 + delta, None)
                sequence_loss.add_hidden(ub.mask[2], hidden, flow if tail else coords1 - coords0, it, iters, pad)
                continue
            if sequence_loss is not None:
                # the criterion needs the mask itself: the inference-only mask head fusion is not taken
                net, up_mask, delta, *upd = ub(net, inp, corr, flow, fuse, **kw)
                coords1, flow = upd if tail else (coords1 + delta, None)
                sequence_loss.add_upsampled(flow if tail else coords1 - coords0, up_mask, it, iters, pad)
                continue
            if self.fuse_mask_upsample and self._mask_fusable(net, inp, corr, coords1):
                from .upsample import channel_window, mask_upsample
                net, hidden, delta, *upd = ub(net, inp, corr, flow, fuse, defer_mask=True, **kw)
                coords1, flow = upd if tail else (coords1 + delta, None)
                hidden, off = channel_window(hidden)
                up = mask_upsample(ub.mask[2], hidden, off, flow if tail else coords1 - coords0, **pw_mask)
            else:
                net, up_mask, delta, *upd = ub(net, inp, corr, flow, fuse, **kw)
                coords1, flow = upd if tail else (coords1 + delta, None)
                up = self.upsample_flow(flow if tail else coords1 - coords0, up_mask)
            predictions.append(self.image_padder.unpad(up))
        return (flow if flow is not None else coords1 - coords0), predictions
