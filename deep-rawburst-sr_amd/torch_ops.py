"""torch.ops.dbsr.* -- the HIP kernels as PyTorch operators.

Loading this module loads libdbsr_torch.so (TORCH_LIBRARY(dbsr, m) over the C ABI of libdbsr_hip.so,
csrc/torch/torch_ops.cpp) and registers autograd formulas, so the ops compose with torch autograd the
way the reference's _FunctionCorrelation does (external/pwcnet/correlation/correlation.py:278-383):

    torch.ops.dbsr.correlation(first, second, leaky=False)      FunctionCorrelation (+ the callers'
                                                                leaky_relu with leaky=True)
    torch.ops.dbsr.backwarp(input, flow)                        pwcnet.py:16-38
    torch.ops.dbsr.warp_bilinear(feat, flow)                    warp.py:19-46
    torch.ops.dbsr.warp_bilinear_flow_backward(grad, feat, flow)   warp's gradient w.r.t. the flow
    torch.ops.dbsr.backwarp_backward(grad, input, flow)         backwarp's gradients -> (dinput, dflow)
    torch.ops.dbsr.fuse_softmax(logits, feats, want_weights)    merging.py:116-126 -> (fused, weights)
    torch.ops.dbsr.conv2d_fused(x, w, b, stride, padding, dilation, act, residual, post_act)
    torch.ops.dbsr.conv_transpose2d_k4s2(x, w, b)               nn.ConvTranspose2d(k4, s2, p1), pwcnet.py:119-120
    torch.ops.dbsr.flow_finalize(flow, H, W)                    pwcnet.py:274-279
    torch.ops.dbsr.resize_bilinear(x, Hp, Wp)                   pwcnet.py:266-271 (forward only)

Gradients: correlation w.r.t. both inputs (K3/K4), backwarp and warp w.r.t. the sampled tensor and the flow
(csrc/flow_grad.hip; backwarp's in-place thresholded mask takes none, pwcnet.py:33-38), fusion w.r.t. the
features / logits, conv2d_fused (act none / relu / lrelu, no residual or post-activation), conv_transpose2d_k4s2
and flow_finalize w.r.t. their tensor inputs (csrc/pwc_grad.hip: PWC-Net training).  Only the gradients autograd
asks for are computed.  No CPU kernels: like the reference's correlation (correlation.py:324-325) the ops raise on
CPU tensors.
"""
import os

import torch

from . import _lib

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, 'libdbsr_torch.so')
_loaded = False


def load():
    """Load the operator library once (raises if it is missing: build with `make`)."""
    global _loaded
    if _loaded:
        return torch.ops.dbsr
    _lib.lib()                               # the C-ABI library it links against (ABI version check)
    if not os.path.exists(LIB_PATH):
        raise _lib.DBSRLibError('libdbsr_torch.so not found at %s: build it with `make`' % LIB_PATH)
    torch.ops.load_library(LIB_PATH)
    _register_autograd()
    _loaded = True
    return torch.ops.dbsr


def _register_autograd():
    lib = torch.library

    def corr_setup(ctx, inputs, output):
        first, second, leaky = inputs
        ctx.save_for_backward(first, second, output)
        ctx.leaky = leaky

    def corr_bwd(ctx, grad):
        first, second, out = ctx.saved_tensors
        d1, d2 = torch.ops.dbsr.correlation_backward(grad.contiguous(), first, second, out, ctx.leaky)
        return d1, d2, None

    lib.register_autograd('dbsr::correlation', corr_bwd, setup_context=corr_setup)

    def warp_setup(ctx, inputs, output):
        feat, flow = inputs
        # the features are needed only for the flow's gradient
        ctx.save_for_backward(flow, feat if ctx.needs_input_grad[1] else None)

    def warp_bwd(ctx, grad):
        flow, feat = ctx.saved_tensors
        grad = grad.contiguous()
        dfeat = torch.ops.dbsr.warp_bilinear_backward(grad, flow) if ctx.needs_input_grad[0] else None
        dflow = torch.ops.dbsr.warp_bilinear_flow_backward(grad, feat, flow) \
            if ctx.needs_input_grad[1] and feat is not None else None
        return dfeat, dflow

    lib.register_autograd('dbsr::warp_bilinear', warp_bwd, setup_context=warp_setup)

    def backwarp_setup(ctx, inputs, output):
        inp, flow = inputs
        ctx.save_for_backward(inp if ctx.needs_input_grad[1] else None, flow)

    def backwarp_bwd(ctx, grad):
        inp, flow = ctx.saved_tensors
        need_in, need_fl = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and inp is not None
        if inp is None:                       # only d/d(input): the kernel does not read the input then
            inp = grad
        din, dfl = torch.ops.dbsr.backwarp_backward(grad.contiguous(), inp, flow, need_in, need_fl)
        return (din if need_in else None), (dfl if need_fl else None)

    lib.register_autograd('dbsr::backwarp', backwarp_bwd, setup_context=backwarp_setup)

    def fuse_setup(ctx, inputs, output):
        logits, feats, want = inputs
        if feats.shape[2] % 8:
            # the forward kernel takes C % 4, the backward C % 8: fail while recording, not in backward()
            raise RuntimeError('dbsr::fuse_softmax: autograd needs C % 8 == 0 (got C = %d)' % feats.shape[2])
        fused, weights = output
        if weights.numel() == 0:           # weights are needed for the backward: recompute them
            _, weights = torch.ops.dbsr.fuse_softmax(logits, feats, True)
        ctx.save_for_backward(weights, feats, fused)

    def fuse_bwd(ctx, dfused, dweights):
        weights, feats, fused = ctx.saved_tensors
        if dweights is not None and dweights.numel() and bool(dweights.abs().sum() != 0):
            raise NotImplementedError('dbsr::fuse_softmax: gradient through the returned weights is not '
                                      'supported (the reference discards them, dbsrnet.py:38)')
        dl, df = torch.ops.dbsr.fuse_backward(weights, feats, fused, dfused.contiguous())
        return dl, df, None

    lib.register_autograd('dbsr::fuse_softmax', fuse_bwd, setup_context=fuse_setup)

    # conv2d_fused: act none / ReLU / LeakyReLU without a residual or post-activation (csrc/pwc_grad.hip and the
    # stride-1 kernels of train_ops.hip, chosen by dbsr::conv2d_backward)
    def conv_setup(ctx, inputs, output):
        x, weight, bias, stride, padding, dilation, act, residual, post_act = inputs
        if residual is not None or post_act != 0:
            # the inner activation's output is not kept, so its gradient cannot be formed: fail while recording
            raise RuntimeError('dbsr::conv2d_fused: autograd needs residual=None and post_act=0')
        if act not in (_lib.ACT_NONE, _lib.ACT_RELU, _lib.ACT_LRELU):
            raise RuntimeError('dbsr::conv2d_fused: autograd needs act in {none, relu, lrelu} (got %d)' % act)
        need_w = ctx.needs_input_grad[1]
        ctx.save_for_backward(x if need_w else None, weight, output if act != _lib.ACT_NONE else None)
        ctx.conv = (stride, padding, dilation, act)
        ctx.x_meta = (x.shape, x.dtype)

    def conv_bwd(ctx, grad):
        x, weight, out = ctx.saved_tensors
        stride, padding, dilation, act = ctx.conv
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        if x is None:                         # only d/d(input): the kernels read the input's shape and dtype alone
            x = torch.empty(ctx.x_meta[0], dtype=ctx.x_meta[1], device=grad.device)
        if out is None:
            out = grad
        dx, dw, db = torch.ops.dbsr.conv2d_backward(grad.contiguous(), x, weight, out, stride, padding, dilation, act,
                                                    need_x, need_w, need_b)
        return (dx if need_x else None, dw if need_w else None, db if need_b else None,
                None, None, None, None, None, None)

    lib.register_autograd('dbsr::conv2d_fused', conv_bwd, setup_context=conv_setup)

    def convt_setup(ctx, inputs, output):
        x, weight, bias = inputs
        ctx.save_for_backward(x, weight)

    def convt_bwd(ctx, grad):
        x, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        dx, dw, db = torch.ops.dbsr.conv_transpose2d_k4s2_backward(grad.contiguous(), x, weight, need_x, need_w, need_b)
        return dx if need_x else None, dw if need_w else None, db if need_b else None

    lib.register_autograd('dbsr::conv_transpose2d_k4s2', convt_bwd, setup_context=convt_setup)

    def ff_setup(ctx, inputs, output):
        flow, H, W, Hp, Wp = inputs
        ctx.ff = (flow.shape[2], flow.shape[3], Hp or 4 * flow.shape[2], Wp or 4 * flow.shape[3])

    def ff_bwd(ctx, grad):
        hf, wf, Hp, Wp = ctx.ff
        return torch.ops.dbsr.flow_finalize_backward(grad.contiguous(), hf, wf, Hp, Wp), None, None, None, None

    lib.register_autograd('dbsr::flow_finalize', ff_bwd, setup_context=ff_setup)


def FunctionCorrelation(tenFirst, tenSecond):
    """Drop-in for external/pwcnet/correlation/correlation.py:385-387 (differentiable)."""
    return load().correlation(tenFirst, tenSecond, False)


class ModuleCorrelation(torch.nn.Module):
    """correlation.py:391-396."""
    def forward(self, tenFirst, tenSecond):
        return FunctionCorrelation(tenFirst, tenSecond)
