"""Training objectives (models/loss/image_quality_v2.py) on the HIP kernels of csrc/objective.hip, and the
description of a training step's loss that training.DBSRTrainer(objective=...) builds into its plan.

PixelWiseError, PSNR and AlignedL2 have the reference's signatures.  On device tensors ([B, 3, H, W]; a single
[3, H, W] image too) they run dbsr_objective_forward / dbsr_psnr_from_stats -- there is no torch fall-back on the
device: a shape the kernels do not serve is an error -- and PixelWiseError / AlignedL2 carry autograd to `pred`.  CPU
tensors run evaluation.PixelWiseError / evaluation.PSNR, the torch restatement of the reference (the scoring paths'
numbers; untouched).

One deviation from torch autograd: 'l2_sqrt' has gradient 0 at a pixel whose three differences are all zero, where
autograd through sqrt gives NaN ('Objectives on the fused step').
"""
import torch
import torch.nn as nn

from . import evaluation

METRICS = ('l1', 'l2', 'l2_sqrt', 'charbonnier')


def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError('unknown metric %r (one of %s)' % (metric, ', '.join(METRICS)))


def _refuse_mask(metric, valid):
    if valid is not None and metric not in ('l1', 'l2'):
        # the reference's own closures take no `reduction` argument: TypeError there (image_quality_v2.py:36-43,60)
        raise ValueError('PixelWiseError(%r) does not take a valid mask (l1 and l2 do)' % (metric,))


def _as_batch(pred, gt, valid=None):
    if pred.dim() == 3:
        pred, gt = pred.unsqueeze(0), gt.unsqueeze(0)
        if valid is not None and valid.dim() == 3:
            valid = valid.unsqueeze(0)
    if pred.dim() != 4 or pred.shape[1] != 3 or gt.shape != pred.shape:
        raise ValueError('objectives: device tensors must be [B, 3, H, W] (or [3, H, W]) of one shape, got %s and %s'
                         % (tuple(pred.shape), tuple(gt.shape)))
    return pred, gt, valid


class _PixelWiseHip(torch.autograd.Function):
    """PixelWiseError on dbsr_objective_forward with autograd to pred: the kernel leaves the unnormalised gradient
    and the scale 1 / denominator on the device (with a mask the denominator is known only after the reduction)."""

    @staticmethod
    def forward(ctx, pred, gt, valid, bi, metric):
        from . import ops
        ctx.in_dtype = pred.dtype
        loss, g, _ = ops.objective_forward(pred.detach(), gt.detach(), bi, metric, 1.0, valid,
                                           want_grad=ctx.needs_input_grad[0])
        if g is not None:
            ctx.save_for_backward(g, loss)
        return loss[0].clone()

    @staticmethod
    def backward(ctx, gloss):
        g, loss = ctx.saved_tensors
        return (g * (loss[2] * gloss.float())).to(ctx.in_dtype), None, None, None, None


class PixelWiseError(nn.Module):
    """models/loss/image_quality_v2.py:24-66: metric in 'l1', 'l2', 'l2_sqrt', 'charbonnier' over the
    boundary_ignore crop; `valid` ([B, 1, H, W]) with 'l1' and 'l2' only."""

    def __init__(self, metric='l1', boundary_ignore=None):
        super().__init__()
        _check_metric(metric)
        self.metric, self.boundary_ignore = metric, boundary_ignore
        self._cpu = evaluation.PixelWiseError(metric=metric, boundary_ignore=boundary_ignore or None)

    def forward(self, pred, gt, valid=None):
        _refuse_mask(self.metric, valid)
        if not pred.is_cuda:
            return self._cpu(pred, gt, valid=valid)
        pred, gt, valid = _as_batch(pred, gt, valid)
        return _PixelWiseHip.apply(pred, gt, valid, self.boundary_ignore or 0, self.metric)


class PSNR(nn.Module):
    """models/loss/image_quality_v2.py:69-101: per-image PSNR over the crop, images whose value is inf or NaN
    dropped, the mean of the rest (0 if none is left).  max_value=None takes each image's gt.max().  On the device
    the result is a 0-dim tensor (no gradient: a statistic) and nothing is read back."""

    def __init__(self, boundary_ignore=None, max_value=1.0):
        super().__init__()
        self.boundary_ignore, self.max_value = boundary_ignore, max_value
        self._cpu = evaluation.PSNR(boundary_ignore=boundary_ignore or None, max_value=max_value)

    def forward(self, pred, gt, valid=None):
        if not pred.is_cuda:
            return self._cpu(pred, gt, valid=valid)
        from . import ops
        pred, gt, valid = _as_batch(pred, gt, valid)
        with torch.no_grad():
            _, _, stats = ops.objective_forward(pred, gt, self.boundary_ignore or 0, 'l2', 1.0, valid, want_grad=False)
            maxes = gt.float().amax(dim=(1, 2, 3)) if self.max_value is None else None
            value, _ = ops.psnr_from_stats(stats, self.max_value, maxes, masked=valid is not None)
        return value[0]


class AlignedL2(nn.Module):
    """models/loss/image_quality_v2.py:166-191: burstsr.SpatialColorAlignment, then the masked MSE over the crop
    (device tensors only, as the alignment)."""

    def __init__(self, alignment_net, sr_factor=4, boundary_ignore=None):
        super().__init__()
        from .burstsr import SpatialColorAlignment
        self.sca = SpatialColorAlignment(alignment_net, sr_factor)
        self.boundary_ignore = boundary_ignore

    def forward(self, pred, gt, burst_input):
        pred_warped_m, valid = self.sca(pred, gt, burst_input)
        return masked_mse(pred_warped_m, gt, valid, self.boundary_ignore)


def masked_mse(pred, gt, valid, boundary_ignore=None):
    """AlignedL2's tail (:176-191): sum(valid (pred - gt)^2) / (3 sum(valid) + 1e-12) over the crop."""
    if not pred.is_cuda:
        return evaluation.PixelWiseError('l2', boundary_ignore or None)(pred, gt, valid=valid)
    pred, gt, valid = _as_batch(pred, gt, valid)
    return _PixelWiseHip.apply(pred, gt, valid, boundary_ignore or 0, 'l2')


class Objective:
    """A training step's loss: weight * PixelWiseError(metric) + ssim * (1 - SSIM) + extra(pred, gt), every term
    with the same boundary_ignore crop.

    metric / weight: the pixel-wise term.  ssim: the weight of image_quality_v2.SSIM(use_for_loss=True) with the
    fixed dynamic range ssim_val_range (the reference's data-dependent rule would read the prediction back), or None.
    extra: a callable (pred, gt) -> scalar tensor differentiable w.r.t. pred (evaluation.LPIPS(differentiable=True)
    times a weight, or any torch objective; it crops for itself), or None.  psnr: keep Stat/psnr.

    DBSRTrainer(objective=...) runs the first two inside its plan; `extra` runs eagerly between the plan's forward
    and backward.  Calling the object evaluates the same loss through the modules of this file (autograd to pred)."""

    def __init__(self, metric='l1', weight=1.0, ssim=None, extra=None, psnr=True, boundary_ignore=40,
                 ssim_val_range=1.0):
        _check_metric(metric)
        if extra is not None and not callable(extra):
            raise ValueError('Objective: extra must be a callable (pred, gt) -> scalar tensor')
        if ssim is not None and not float(ssim_val_range) > 0.0:
            raise ValueError('Objective: ssim_val_range must be > 0')
        self.metric, self.weight = metric, float(weight)
        self.ssim = None if ssim is None else float(ssim)
        self.extra, self.psnr = extra, bool(psnr)
        self.boundary_ignore = int(boundary_ignore or 0)
        self.ssim_val_range = float(ssim_val_range)

    @staticmethod
    def of(spec, boundary_ignore=40):
        """An Objective from a metric name (with the caller's boundary_ignore) or an Objective as it is."""
        if isinstance(spec, Objective):
            return spec
        if isinstance(spec, str):
            return Objective(metric=spec, boundary_ignore=boundary_ignore)
        raise ValueError('objective: a metric name or an objectives.Objective, got %r' % (spec,))

    def __call__(self, pred, gt):
        bi = self.boundary_ignore or None
        total = self.weight * PixelWiseError(self.metric, bi)(pred, gt)
        if self.ssim is not None:
            total = total + self.ssim * evaluation.SSIM(bi, use_for_loss=True, val_range=self.ssim_val_range)(pred, gt)
        if self.extra is not None:
            total = total + self.extra(pred, gt)
        return total
