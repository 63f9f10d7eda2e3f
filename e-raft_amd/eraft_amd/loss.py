"""The reference's training loss (train.py:47-75 sequence_loss; the same function in
eraft_train.py and train_dsec.py): the gamma-weighted L1 over every prediction of the refinement
loop, masked by `valid` and |gt| < max_flow, plus the EPE / 1px / 3px / 5px metrics of the last.

On the MI355X it runs on the kernels of csrc/corr_loss.hip, in two forms:
  sequence_loss(preds, gt, valid)      over stored predictions (corr_sequence_loss / _bwd);
  SequenceLoss(gt, valid)              a criterion the model feeds per iteration: add_upsampled
                                       takes the 1/8-resolution flow and the 576-channel mask and
                                       is one fused launch pair forward (corr_upsample_loss) and
                                       one backward (corr_upsample_loss_bwd), so neither the
                                       full-resolution prediction nor its gradient is ever stored
                                       (ERAFT.forward(..., sequence_loss=crit)); add_hidden takes
                                       relu(mask[0](net)) and the head mask[2] instead of the mask
                                       and runs the head inside the launches (csrc/corr_mask_loss.hip:
                                       corr_mask_upsample_loss forward, corr_mask_upsample_loss_bwd
                                       and the convolution's backward over dz), so no mask is stored
                                       or saved either (ERAFT.fuse_mask_loss).
Anything that is not an fp32 GPU tensor goes through the plain torch composition below.  Nothing
here synchronises: the metrics are 0-dim tensors, float(m["epe"]) is the reference's .item().
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch.autograd.function import once_differentiable

__all__ = ["SequenceLoss", "sequence_loss"]


def _valid_plane(valid, gt):
    """valid as [B, H, W] (a [B, 1, H, W] mask loses its channel)."""
    if valid.dim() == 4 and valid.shape[1] == 1:
        valid = valid[:, 0]
    if valid.dim() != 3 or gt.dim() != 4 or gt.shape[1] != 2 or tuple(valid.shape) != (gt.shape[0], *gt.shape[2:]):
        raise ValueError(f"sequence_loss: flow_gt {tuple(gt.shape)} needs valid [B, H, W] or [B, 1, H, W] "
                         f"(got {tuple(valid.shape)})")
    return valid


def _on_hip(*ts):
    return all(isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 for t in ts)


def _torch_upsample(flow, mask):
    """The convex upsampling as the reference composes it (eraft.py:75-86)."""
    n, _, h, w = flow.shape
    mask = torch.softmax(mask.view(n, 1, 9, 8, 8, h, w), dim=2)
    up = F.unfold(8 * flow, [3, 3], padding=1).view(n, 2, 9, 1, 1, h, w)
    up = torch.sum(mask * up, dim=2).permute(0, 1, 4, 2, 5, 3)
    return up.reshape(n, 2, 8 * h, 8 * w)


def _torch_mask(gt, valid, max_flow):
    mag = torch.sum(gt ** 2, dim=1).sqrt()
    return (valid >= 0.5) & (mag < max_flow)


def _torch_metrics(pred, gt, v):
    epe = torch.sum((pred - gt) ** 2, dim=1).sqrt()
    epe = epe.reshape(-1)[v.reshape(-1)]
    return {"epe": epe.mean(), "1px": (epe < 1).float().mean(), "3px": (epe < 3).float().mean(),
            "5px": (epe < 5).float().mean()}


def _metrics(stats):
    """The six words of the last term -> the reference's metrics (NaN with no valid pixel: 0 / 0)."""
    return {"epe": stats[2] / stats[1], "1px": stats[3] / stats[1], "3px": stats[4] / stats[1],
            "5px": stats[5] / stats[1]}


def _scale(grad, coef):
    """The backward kernels' device scalar: upstream gradient * weight / numel, no host sync."""
    return (grad.detach().to(torch.float32) * coef).reshape(1).contiguous()


class _SequenceLossFn(torch.autograd.Function):
    """One term over a stored prediction: (weight * mean(v |pred - gt|), the six fp64 words)."""

    @staticmethod
    def forward(ctx, pred, gt, valid, max_flow, weight, want_metrics):
        from . import _lib
        stats = _lib.sequence_loss(pred, gt, valid, max_flow, want_metrics)
        ctx.save_for_backward(pred, gt, valid)
        ctx.max_flow, ctx.coef = max_flow, weight / pred.numel()
        ctx.mark_non_differentiable(stats)
        return (stats[0] * ctx.coef).float(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _grad_stats):
        from . import _lib
        pred, gt, valid = ctx.saved_tensors
        return _lib.sequence_loss_bwd(pred, gt, valid, _scale(grad, ctx.coef), ctx.max_flow), None, None, None, None, None


class _UpsampleLossFn(torch.autograd.Function):
    """One term of the prediction upsample_flow(flow, mask)[..., pad_h:, pad_w:], which is never
    stored: saves flow and mask, and its backward forms the prediction's gradient in registers."""

    @staticmethod
    def forward(ctx, flow, mask, gt, valid, max_flow, weight, want_metrics):
        from . import _lib
        stats = _lib.upsample_loss(flow, mask, gt, valid, max_flow, want_metrics)
        ctx.save_for_backward(flow, mask, gt, valid)
        ctx.max_flow, ctx.coef = max_flow, weight / gt.numel()
        ctx.mark_non_differentiable(stats)
        return (stats[0] * ctx.coef).float(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _grad_stats):
        from . import _lib
        flow, mask, gt, valid = ctx.saved_tensors
        dflow, dmask = _lib.upsample_loss_bwd(flow, mask, gt, valid, _scale(grad, ctx.coef), ctx.max_flow)
        return dflow, dmask, None, None, None, None, None


class _MaskHeadLossFn(torch.autograd.Function):
    """One term of the prediction upsample_flow(flow, scale * conv(hidden))[..., pad_h:, pad_w:] for
    the 1x1 mask head `conv`: saves hidden, flow and the parameters, never a mask; its backward
    recomputes the logits, and the head's own gradients are aten's convolution_backward over dz."""

    @staticmethod
    def forward(ctx, hidden, flow, weight, bias, gt, valid, conv, mask_scale, max_flow, coef, want_metrics):
        from . import _lib
        from .upsample import _mask_pack, channel_window
        packed, pbias = _mask_pack(conv)
        buf, off = channel_window(hidden)
        stats = _lib.mask_upsample_loss(buf, off, flow, packed, pbias, mask_scale, gt, valid, max_flow, want_metrics)
        ctx.save_for_backward(hidden, flow, weight, bias, gt, valid)
        ctx.conv, ctx.mask_scale, ctx.max_flow, ctx.coef = conv, mask_scale, max_flow, coef
        ctx.mark_non_differentiable(stats)
        return (stats[0] * coef).float(), stats

    @staticmethod
    @once_differentiable
    def backward(ctx, grad, _grad_stats):
        from . import _lib
        from .upsample import _mask_pack, channel_window
        hidden, flow, weight, bias, gt, valid = ctx.saved_tensors
        packed, pbias = _mask_pack(ctx.conv)
        buf, off = channel_window(hidden)
        dflow, dz = _lib.mask_upsample_loss_bwd(buf, off, flow, packed, pbias, ctx.mask_scale, gt, valid,
                                                _scale(grad, ctx.coef), ctx.max_flow)
        need = (ctx.needs_input_grad[0], ctx.needs_input_grad[2], ctx.needs_input_grad[3])
        dhidden = dweight = dbias = None
        if any(need):
            dhidden, dweight, dbias = torch.ops.aten.convolution_backward(
                dz, hidden, weight, [576], [1, 1], [0, 0], [1, 1], False, [0, 0], 1, list(need))
        return dhidden, dflow, dweight, dbias, None, None, None, None, None, None, None


def _is_mask_head(conv):
    return (isinstance(conv, torch.nn.Conv2d) and tuple(conv.weight.shape) == (576, 256, 1, 1)
            and conv.bias is not None and conv.stride == (1, 1) and conv.padding == (0, 0)
            and conv.weight.is_cuda and conv.weight.dtype == conv.bias.dtype == torch.float32)


class SequenceLoss:
    """The sequence loss as a criterion that takes its predictions one at a time.

        crit = SequenceLoss(flow_gt, valid)
        model(image1, image2, iters=12, sequence_loss=crit)     # add_upsampled per iteration
        loss, metrics = crit.result(); loss.backward()

    `index` / `total` give a term its weight gamma^(total - 1 - index); the term with index ==
    total - 1 also yields the metrics.  result() sums the terms in iteration order."""

    def __init__(self, flow_gt, valid, gamma=0.8, max_flow=400.0):
        valid = _valid_plane(valid, flow_gt)
        self.hip = flow_gt.is_cuda and flow_gt.dtype == torch.float32
        if self.hip:
            flow_gt, valid = flow_gt.detach().contiguous(), valid.detach().to(torch.float32).contiguous()
        self.flow_gt, self.valid = flow_gt, valid
        self.gamma, self.max_flow = float(gamma), float(max_flow)
        self._terms, self._metrics = {}, None

    def _record(self, index, total, term, metrics):
        if not 0 <= index < total:
            raise ValueError(f"SequenceLoss: index {index} of {total} predictions")
        if index in self._terms:
            raise ValueError(f"SequenceLoss: prediction {index} was added twice")
        self._terms[index] = term
        if index == total - 1:
            self._metrics = metrics()

    def _weight(self, index, total):
        return self.gamma ** (total - index - 1)

    def add(self, pred, index, total):
        """A stored prediction [B, 2, H, W]."""
        if pred.shape != self.flow_gt.shape:
            raise ValueError(f"SequenceLoss: prediction {tuple(pred.shape)}, flow_gt {tuple(self.flow_gt.shape)}")
        last = index == total - 1
        if self.hip and _on_hip(pred):
            term, stats = _SequenceLossFn.apply(pred.contiguous(), self.flow_gt, self.valid, self.max_flow,
                                                self._weight(index, total), last)
            self._record(index, total, term, lambda: _metrics(stats))
        else:
            v = _torch_mask(self.flow_gt, self.valid, self.max_flow)
            term = self._weight(index, total) * (v[:, None] * (pred - self.flow_gt).abs()).mean()
            self._record(index, total, term, lambda: _torch_metrics(pred.detach(), self.flow_gt, v))

    def add_upsampled(self, flow, mask, index, total, pad=(0, 0)):
        """The prediction upsample_flow(flow, mask) without its first pad = (pad_h, pad_w) rows and
        columns (ImagePadder pads at the top and left), from flow [B, 2, h, w] and mask
        [B, 576, h, w]."""
        ph, pw = int(pad[0]), int(pad[1])
        H, W = self.flow_gt.shape[2:]
        if flow.dim() != 4 or (8 * flow.shape[2] - ph, 8 * flow.shape[3] - pw) != (H, W) or ph < 0 or pw < 0:
            raise ValueError(f"SequenceLoss: flow {tuple(flow.shape)} with pad {(ph, pw)} does not upsample to "
                             f"flow_gt's {H}x{W}")
        if self.hip and _on_hip(flow, mask):
            term, stats = _UpsampleLossFn.apply(flow.contiguous(), mask.contiguous(), self.flow_gt, self.valid,
                                                self.max_flow, self._weight(index, total), index == total - 1)
            self._record(index, total, term, lambda: _metrics(stats))
        else:
            self.add(_torch_upsample(flow, mask)[..., ph:, pw:], index, total)

    def add_hidden(self, conv, hidden, flow, index, total, pad=(0, 0), scale=0.25):
        """The same term as add_upsampled(flow, scale * conv(hidden), ...) from hidden =
        relu(mask[0](net)) [B, 256, h, w] (a channel slice of a wider contiguous buffer is read in
        place) and the mask head `conv`.  With fp32 GPU tensors and a 256 -> 576 1x1 `conv` with a
        bias the head runs inside the fused launches and no mask is stored or saved for backward."""
        ph, pw = int(pad[0]), int(pad[1])
        H, W = self.flow_gt.shape[2:]
        if (flow.dim() != 4 or hidden.dim() != 4 or (8 * flow.shape[2] - ph, 8 * flow.shape[3] - pw) != (H, W)
                or ph < 0 or pw < 0 or hidden.shape[0] != flow.shape[0] or hidden.shape[2:] != flow.shape[2:]):
            raise ValueError(f"SequenceLoss: hidden {tuple(hidden.shape)}, flow {tuple(flow.shape)} with pad "
                             f"{(ph, pw)} do not upsample to flow_gt's {H}x{W}")
        if (self.hip and _on_hip(hidden, flow) and _is_mask_head(conv) and hidden.shape[1] == 256
                and hidden.device == flow.device == conv.weight.device == self.flow_gt.device):
            term, stats = _MaskHeadLossFn.apply(hidden, flow.contiguous(), conv.weight, conv.bias, self.flow_gt,
                                                self.valid, conv, float(scale), self.max_flow,
                                                self._weight(index, total) / self.flow_gt.numel(),
                                                index == total - 1)
            self._record(index, total, term, lambda: _metrics(stats))
        else:
            self.add_upsampled(flow, scale * conv(hidden), index, total, pad)

    def result(self):
        """(loss, metrics) of the predictions added so far; metrics is None until the last one is."""
        if not self._terms:
            raise RuntimeError("SequenceLoss: no prediction was added")
        loss = None
        for index in sorted(self._terms):
            loss = self._terms[index] if loss is None else loss + self._terms[index]
        return loss, self._metrics


def sequence_loss(flow_preds, flow_gt, valid, gamma=0.8, max_flow=400.0):
    """The reference's sequence_loss(flow_preds, flow_gt, valid, gamma, max_flow) -> (loss, metrics),
    with valid [B, H, W] or [B, 1, H, W] and the metrics as 0-dim tensors (no .item(), no sync)."""
    crit = SequenceLoss(flow_gt, valid, gamma, max_flow)
    n = len(flow_preds)
    for i, pred in enumerate(flow_preds):
        crit.add(pred, i, n)
    return crit.result()
