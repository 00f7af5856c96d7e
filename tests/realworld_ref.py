"""Torch-CPU restatement of the real-world objective (actors/dbsr_actors.py:68-80), shared by the real-world
tests: warp (oracle.warp) -> im_test^T C (spatial_color_alignment.py:64-66) -> PixelWiseError('l1',
boundary_ignore) with the validity mask (image_quality_v2.py:47-66) -> x weight, with autograd to the
prediction.  test_realworld_oracle.py pins it to the reference's own loss and gradient."""
import torch

from oracle import dbsr_oracle as orc


def masked_l1(out, gt, valid, bi, weight):
    """weight * PixelWiseError('l1', boundary_ignore=bi)(out, gt, valid=valid); bi 0 = no crop."""
    if bi:
        out, gt = out[..., bi:-bi, bi:-bi], gt[..., bi:-bi, bi:-bi]
        valid = valid[..., bi:-bi, bi:-bi] if valid is not None else None
    err = (out - gt).abs()
    if valid is None:
        return weight * err.mean()
    v = valid.float()
    return weight * (err * v).sum() / (v.sum() * (err.numel() / v.numel()) + 1e-12)


def aligned_l1(pred, gt, flow, c_mat, valid, bi, weight=1.0):
    """(loss, dL/dpred, the colour-matched warped prediction) for fixed flow / c_mat / valid (each may be None)."""
    pred = pred.detach().clone().requires_grad_(True)
    pw = orc.warp(pred, flow) if flow is not None else pred
    m = torch.einsum('bchw,bck->bkhw', pw, c_mat) if c_mat is not None else pw
    loss = masked_l1(m, gt, valid, bi, weight)
    loss.backward()
    return loss.detach(), pred.grad, m.detach()


def sca_objective(pred, gt, burst, sd, bi=40, weight=10.0, sr_factor=4):
    """The reference's training use of SpatialColorAlignment on the oracle: the flow under no_grad from
    pred.detach() (spatial_color_alignment.py:89-90), autograd through oracle.warp + oracle.match_colors.
    Returns (loss, dL/dpred, (flow, c_mat, valid))."""
    import torch.nn.functional as F
    pred = pred.detach().clone().requires_grad_(True)
    with torch.no_grad():
        flow = orc.pwcnet(pred.detach() / (pred.max() + 1e-6), gt / (gt.max() + 1e-6), sd, 'encoder.alignment_net.net')
    pred_warped = orc.warp(pred, flow)
    ds = 1.0 / float(2.0 * sr_factor)
    flow_ds = F.interpolate(flow, scale_factor=ds, mode='bilinear') * ds
    burst_0_warped = orc.warp(burst[:, 0, [0, 1, 3]].contiguous(), flow_ds)
    gt_ds = F.interpolate(gt, scale_factor=ds, mode='bilinear')
    K, ksz = orc.gaussian_kernel_2d(1.5)
    out, valid, c_mat = orc.match_colors(gt_ds, burst_0_warped, pred_warped, ksz, K)
    loss = masked_l1(out, gt, valid, bi, weight)
    loss.backward()
    return loss.detach(), pred.grad, (flow, c_mat.detach(), valid)
