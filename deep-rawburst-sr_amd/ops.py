"""Op-level mirror of the reference's functional sub-seams, NCHW in / NCHW out like the reference:

  FunctionCorrelation(tenFirst, tenSecond)      external/pwcnet/correlation/correlation.py:385-387
  backwarp(tenInput, tenFlow)                   models/alignment/pwcnet.py:16-38
  warp(feat, flow, mode, padding_mode)          models/layers/warp.py:19-46
  conv2d(...)                                   nn.Conv2d (+ fused activation / residual) via dbsr_conv2d

Each runs the HIP kernel of libdbsr_hip.so; the NCHW<->NHWC permutes around the call are torch
device copies (layout plumbing for callers that hold NCHW tensors; the engine never uses them).
Errors mirror the reference: non-contiguous input to the correlation raises (correlation.py:286-287),
a CPU tensor raises (correlation.py:324-325 raises NotImplementedError on CPU).
"""
import collections

import torch

from . import _lib as L


def _nhwc(x, dtype=None):
    t = x.permute(0, 2, 3, 1)
    if dtype is not None:
        t = t.to(dtype)
    c = t.shape[-1]
    ld = (c + 7) // 8 * 8 if c <= 16 else (c + 31) // 32 * 32     # dbsr_conv2d channel padding
    out = torch.zeros(*t.shape[:-1], ld, dtype=t.dtype, device=t.device)
    out[..., :c] = t
    return out, ld


def _need_cuda(*ts):
    for t in ts:
        if not t.is_cuda:
            raise NotImplementedError('dbsr_amd ops run on the HIP device only (no CPU implementation, as '
                                      'correlation.py:324-325)')


def FunctionCorrelation(tenFirst, tenSecond, leaky=False):
    """81-channel cost volume / C (K2).  leaky=True fuses the callers' leaky_relu(0.1)."""
    _need_cuda(tenFirst, tenSecond)
    if not (tenFirst.is_contiguous() and tenSecond.is_contiguous()):
        raise AssertionError('correlation inputs must be contiguous (correlation.py:286-287)')
    N, C, H, W = tenFirst.shape
    dt = tenFirst.dtype
    a, lda = _nhwc(tenFirst)
    b, ldb = _nhwc(tenSecond)
    out = torch.zeros(N, H, W, 88, dtype=dt, device=tenFirst.device)
    L.check(L.lib().dbsr_correlation(N, H, W, C, L.tensor_desc(a, lda), L.tensor_desc(b, ldb),
                                     L.tensor_desc(out, 88), 1 if leaky else 0, L.stream_ptr(tenFirst.device)),
            'dbsr_correlation')
    return out[..., :81].permute(0, 3, 1, 2).contiguous()


class ModuleCorrelation(torch.nn.Module):
    def forward(self, tenFirst, tenSecond):
        return FunctionCorrelation(tenFirst, tenSecond)


def backwarp(tenInput, tenFlow):
    _need_cuda(tenInput, tenFlow)
    N, C, H, W = tenInput.shape
    x, ldx = _nhwc(tenInput)
    fl = tenFlow.permute(0, 2, 3, 1).to(torch.float32).contiguous()
    out = torch.zeros_like(x)
    L.check(L.lib().dbsr_backwarp(N, H, W, C, L.tensor_desc(x, ldx), L.tensor_desc(fl, 2), 1.0,
                                  L.tensor_desc(out, ldx), L.stream_ptr(tenInput.device)), 'dbsr_backwarp')
    return out[..., :C].permute(0, 3, 1, 2).contiguous()


def warp(feat, flow, mode='bilinear', padding_mode='zeros'):
    if mode != 'bilinear' or padding_mode != 'zeros':
        raise NotImplementedError('only bilinear / zeros is on the hot path (encoders.py:80)')
    _need_cuda(feat, flow)
    N, C, H, W = feat.shape
    x, ld = _nhwc(feat)
    fl = flow.to(torch.float32).contiguous()
    out = torch.zeros_like(x)
    L.check(L.lib().dbsr_warp_bilinear(N, H, W, ld, L.tensor_desc(x, ld), fl.data_ptr(), 2 * H * W,
                                       L.tensor_desc(out, ld), L.stream_ptr(feat.device)), 'dbsr_warp_bilinear')
    return out[..., :C].permute(0, 3, 1, 2).contiguous()


_PACKED = collections.OrderedDict()    # (weight, bias, version, dtype, shuffle) -> packed MFMA weights
_PACKED_MAX = 64


def _packed(weight, bias, compute_dtype, shuffle, stream):
    """Packed weights (dbsr_conv_pack_weights) of a parameter, cached while the tensor is unchanged (same
    storage and autograd version counter), so a repeated op-level call does not repack."""
    key = (weight.data_ptr(), weight._version, tuple(weight.shape),
           bias.data_ptr() if bias is not None else 0, bias._version if bias is not None else 0,
           compute_dtype, shuffle, weight.device)
    hit = _PACKED.get(key)
    if hit is not None:
        _PACKED.move_to_end(key)
        return hit[0], hit[1]
    Cout, Cin, kh, kw = weight.shape
    dev = weight.device
    n = L.lib().dbsr_conv_packed_elems(Cout, Cin, kh, kw)
    wp = torch.empty(n, dtype=compute_dtype, device=dev)
    bp = torch.empty(Cout, dtype=torch.float32, device=dev) if bias is not None else None
    w32 = weight.detach().to(torch.float32).contiguous()
    b32 = bias.detach().to(torch.float32).contiguous() if bias is not None else None
    L.check(L.lib().dbsr_conv_pack_weights(w32.data_ptr(), b32.data_ptr() if b32 is not None else None, Cout, Cin,
                                           kh, kw, L.dtype_code(compute_dtype), shuffle, wp.data_ptr(),
                                           bp.data_ptr() if bp is not None else None, stream), 'pack')
    # the cache keeps the source tensors alive so their storage (the key) cannot be reused meanwhile
    _PACKED[key] = (wp, bp, weight, bias, w32, b32)
    while len(_PACKED) > _PACKED_MAX:
        _PACKED.popitem(last=False)
    return wp, bp


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, act=L.ACT_NONE, residual=None,
           post_act=L.ACT_NONE, compute_dtype=torch.float32, out_f32=False, head=None, shuffle=1, max_blocks=0,
           workspace=True):
    """act(conv2d(x) + bias) (+ residual, then post_act); NCHW in/out, computed by dbsr_conv2d.
    max_blocks > 0 caps the workgroups of a persistent kernel (dbsr_conv_desc.max_blocks).
    workspace=False passes no split-K scratch (NULL, 0 bytes): a conv that would split K then runs unsplit.
    head = (w [hc, Cout, 1, 1], b [hc] | None): return ReLU(conv1x1(result, w, b)) as fp32 NCHW instead,
    computed by dbsr_conv2d_head (the conv's own result is not stored).
    shuffle = s > 1: return PixelShuffle(s) of the result (upsampling.py:51-66's conv + shuffle)."""
    _need_cuda(x, weight)
    N, Cin, H, W = x.shape
    Cout, _, kh, kw = weight.shape
    dev = x.device
    xs, ldx = _nhwc(x, compute_dtype)
    s = L.stream_ptr(dev)
    wp, bp = _packed(weight, bias, compute_dtype, shuffle, s)
    oh = (H + 2 * padding - dilation * (kh - 1) - 1) // stride + 1
    ow = (W + 2 * padding - dilation * (kw - 1) - 1) // stride + 1
    ody = torch.float32 if out_f32 else compute_dtype
    pc = Cout // (shuffle * shuffle)
    ldy = (pc + 7) // 8 * 8
    y = torch.zeros(N, oh * shuffle, ow * shuffle, ldy, dtype=ody, device=dev)
    d = L.ConvDesc()
    d.n_frames = N
    d.x = L.tensor_desc(xs, ldx)
    d.in_h, d.in_w, d.cin = H, W, Cin
    d.w = wp.data_ptr()
    d.bias = bp.data_ptr() if bp is not None else None
    d.cout, d.kh, d.kw, d.stride, d.pad, d.dil = Cout, kh, kw, stride, padding, dilation
    d.y = L.tensor_desc(y, ldy)
    d.out_h, d.out_w = oh, ow
    d.act = act
    if residual is not None:
        rr, ldr = _nhwc(residual, ody)
        d.res = L.tensor_desc(rr, ldr)
    else:
        d.res = L.NULL_TENSOR
    d.post_act = post_act
    d.max_blocks = max_blocks
    d.out_mode, d.shuffle = (L.OUT_SHUFFLE, shuffle) if shuffle > 1 else (L.OUT_NHWC, 0)
    need = L.lib().dbsr_conv_workspace_bytes(d)
    ws = torch.zeros(max(need // 4, 1), dtype=torch.float32, device=dev)
    d.workspace, d.workspace_bytes = (ws.data_ptr(), need) if workspace else (None, 0)
    if head is not None:
        hw, hb = head
        hc = hw.shape[0]
        hw32 = hw.reshape(hc, -1).to(device=dev, dtype=torch.float32).contiguous()
        hb32 = hb.to(device=dev, dtype=torch.float32).contiguous() if hb is not None else None
        out = torch.zeros(N, hc, oh, ow, dtype=torch.float32, device=dev)
        L.check(L.lib().dbsr_conv2d_head(d, hw32.data_ptr(), hb32.data_ptr() if hb32 is not None else None, hc,
                                         L.tensor_desc(out, 1, 0, img_stride=hc * oh * ow, dtype=torch.float32),
                                         s), 'dbsr_conv2d_head')
        return out
    conv2d.last_kernel = L.lib().dbsr_conv_kernel_for(d)     # which kernel family ran (tests)
    conv2d.last_variant = L.lib().dbsr_conv_dispatch_variant(d)
    L.check(L.lib().dbsr_conv2d(d, s), 'dbsr_conv2d')
    return y[..., :pc].permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------
# training-step kernels (backward of the ops above; dbsr_hip.h 'training step')
# ---------------------------------------------------------------------------------------------------
def conv2d_wgrad(x, dy, k, compute_dtype=torch.float32, with_bias=False):
    """dL/dW of nn.Conv2d(k x k, stride 1, pad k//2) for input x [N,Cin,H,W] and output gradient dy
    [N,Cout,H,W] (dbsr_conv_wgrad): fp32 [Cout,Cin,k,k].  with_bias: also dL/db = dy.sum((0, 2, 3)) from the
    same pass (dbsr_conv_wgrad_bias), returned as (dw, db)."""
    _need_cuda(x, dy)
    N, Cin, H, W = x.shape
    Cout = dy.shape[1]
    xs, ldx = _nhwc(x, compute_dtype)
    ds, ldd = _nhwc(dy, compute_dtype)
    dw = torch.zeros(Cout, Cin, k, k, dtype=torch.float32, device=x.device)
    need = L.lib().dbsr_conv_wgrad_workspace_bytes(N, H, W, Cin, Cout, k)
    ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=x.device)
    if not with_bias:
        L.check(L.lib().dbsr_conv_wgrad(N, H, W, L.tensor_desc(xs, ldx), Cin, L.tensor_desc(ds, ldd), Cout, k,
                                        dw.data_ptr(), 0, ws.data_ptr(), need, L.stream_ptr(x.device)),
                'dbsr_conv_wgrad')
        return dw
    db = torch.zeros(Cout, dtype=torch.float32, device=x.device)
    L.check(L.lib().dbsr_conv_wgrad_bias(N, H, W, L.tensor_desc(xs, ldx), Cin, L.tensor_desc(ds, ldd), Cout, k,
                                         dw.data_ptr(), db.data_ptr(), 0, ws.data_ptr(), need,
                                         L.stream_ptr(x.device)), 'dbsr_conv_wgrad_bias')
    return dw, db


def conv2d_dgrad(dy, weight, residual=None, gate=None, compute_dtype=torch.float32):
    """dL/dX of nn.Conv2d(weight, stride 1, pad k//2) for output gradient dy [N,Cout,H,W]: the forward conv
    kernel on dgrad-packed weights (dbsr_dgrad_weights + dbsr_conv_pack_weights), then + residual and
    * (gate > 0) in its epilogue (the ResBlock / ReLU backward).  NCHW fp32/bf16 out."""
    _need_cuda(dy, weight)
    Cout, Cin, kh, kw = weight.shape
    w32 = weight.to(torch.float32).contiguous()
    wt = torch.empty(Cin, Cout, kh, kw, dtype=torch.float32, device=dy.device)
    s = L.stream_ptr(dy.device)
    L.check(L.lib().dbsr_dgrad_weights(w32.data_ptr(), Cout, Cin, kh, kw, wt.data_ptr(), s), 'dbsr_dgrad_weights')
    N, _, H, W = dy.shape
    ds, ldd = _nhwc(dy, compute_dtype)
    n = L.lib().dbsr_conv_packed_elems(Cin, Cout, kh, kw)
    wp = torch.empty(n, dtype=compute_dtype, device=dy.device)
    L.check(L.lib().dbsr_conv_pack_weights(wt.data_ptr(), None, Cin, Cout, kh, kw, L.dtype_code(compute_dtype), 1,
                                           wp.data_ptr(), None, s), 'pack')
    ldy = (Cin + 7) // 8 * 8
    y = torch.zeros(N, H, W, ldy, dtype=compute_dtype, device=dy.device)
    d = L.ConvDesc()
    d.n_frames = N
    d.x = L.tensor_desc(ds, ldd)
    d.in_h, d.in_w, d.cin = H, W, Cout
    d.w, d.bias = wp.data_ptr(), None
    d.cout, d.kh, d.kw, d.stride, d.pad, d.dil = Cin, kh, kw, 1, kh // 2, 1
    d.y = L.tensor_desc(y, ldy)
    d.out_h, d.out_w = H, W
    d.act, d.post_act = L.ACT_NONE, L.ACT_NONE
    keep = []
    if residual is not None:
        rr, ldr = _nhwc(residual, compute_dtype)
        if ldr != ldy:
            rr = torch.nn.functional.pad(rr, (0, ldy - ldr)) if ldr < ldy else rr[..., :ldy].contiguous()
        d.res = L.tensor_desc(rr, ldy)
        keep.append(rr)
    if gate is not None:
        gg, ldg = _nhwc(gate, compute_dtype)
        if ldg != ldy:
            gg = torch.nn.functional.pad(gg, (0, ldy - ldg)) if ldg < ldy else gg[..., :ldy].contiguous()
        d.gate = L.tensor_desc(gg, ldy)
        keep.append(gg)
    d.out_mode, d.shuffle = L.OUT_NHWC, 0
    need = L.lib().dbsr_conv_workspace_bytes(d)
    ws = torch.zeros(max(need // 4, 1), dtype=torch.float32, device=dy.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), need
    conv2d_dgrad.last_kernel = L.lib().dbsr_conv_kernel_for(d)     # which kernel family ran (tests)
    L.check(L.lib().dbsr_conv2d(d, s), 'dbsr_conv2d (dgrad)')
    return y[..., :Cin].permute(0, 3, 1, 2).contiguous()


def fuse_backward(weights, all_feat, fused, dfused):
    """Softmax-fusion backward (merging.py:116-124): weights / all_feat [B,N,C,H,W], fused / dfused [B,C,H,W]
    -> (dlogits [B,N,C,H,W], dfeat [B,N,C,H,W])."""
    _need_cuda(weights, all_feat, fused, dfused)
    B, N, C, H, W = all_feat.shape
    dt = all_feat.dtype
    nh = lambda t: t.reshape(-1, C, H, W).permute(0, 2, 3, 1).contiguous()          # noqa: E731
    w, f = nh(weights.to(dt)), nh(all_feat)
    fu, dfu = nh(fused.to(dt)), nh(dfused.to(dt))
    dl = torch.empty_like(w)
    df = torch.empty_like(f)
    img = H * W * C
    L.check(L.lib().dbsr_fuse_backward(B, N, H * W, C, L.tensor_desc(w, C, img_stride=img),
                                       L.tensor_desc(f, C, img_stride=img, fmap=(1, N, 0, 1)),
                                       L.tensor_desc(f, C, img_stride=img, fmap=(N - 1, N, 1, 1)),
                                       L.tensor_desc(fu, C, img_stride=img), L.tensor_desc(dfu, C, img_stride=img),
                                       L.tensor_desc(dl, C, img_stride=img),
                                       L.tensor_desc(df, C, img_stride=img, fmap=(1, N, 0, 1)),
                                       L.tensor_desc(df, C, img_stride=img, fmap=(N - 1, N, 1, 1)),
                                       L.stream_ptr(all_feat.device)), 'dbsr_fuse_backward')
    back = lambda t: t.view(B, N, H, W, C).permute(0, 1, 4, 2, 3).contiguous()        # noqa: E731
    return back(dl), back(df)


def warp_backward(dout, flow):
    """dL/dfeat of warp(feat, flow) (warp.py:19-46): dout [N,C,H,W], flow [N,2,H,W] -> fp32 [N,C,H,W]."""
    _need_cuda(dout, flow)
    N, C, H, W = dout.shape
    d = dout.permute(0, 2, 3, 1).contiguous()
    fl = flow.to(torch.float32).contiguous()
    out = torch.zeros(N, H, W, C, dtype=torch.float32, device=dout.device)
    L.check(L.lib().dbsr_warp_backward(N, H, W, C, L.tensor_desc(d, C), fl.data_ptr(), 2 * H * W, out.data_ptr(),
                                       L.FrameMap(1, 1, 0, 1), H * W * C, L.stream_ptr(dout.device)),
            'dbsr_warp_backward')
    return out.permute(0, 3, 1, 2).contiguous()


def warp_backward_gather(dout, flow, gate=None):
    """dL/dfeat of warp(feat, flow) (warp.py:19-46) by the owner-computes gather kernel, optionally times
    [gate > 0] (the encoder's ReLU): dout [N,C,H,W] (fp32 / bf16 / fp16), flow [N,2,H,W], gate like dout ->
    [N,C,H,W] in dout's dtype."""
    _need_cuda(dout, flow)
    N, C, H, W = dout.shape
    dev = dout.device
    d = dout.permute(0, 2, 3, 1).contiguous()
    fl = flow.to(torch.float32).contiguous()
    out = torch.empty_like(d)
    g = gate.to(dout.dtype).permute(0, 2, 3, 1).contiguous() if gate is not None else None
    need = L.lib().dbsr_warp_backward_gather_workspace_bytes(N, H, W)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    L.check(L.lib().dbsr_warp_backward_gather(N, H, W, C, L.tensor_desc(d, C), fl.data_ptr(), 2 * H * W,
                                              L.tensor_desc(g, C) if g is not None else L.NULL_TENSOR,
                                              L.tensor_desc(out, C), ws.data_ptr(), need, L.stream_ptr(dev)),
            'dbsr_warp_backward_gather')
    return out.permute(0, 3, 1, 2).contiguous()


def warp_flow_backward(feat, dout, flow):
    """dL/dflow of warp(feat, flow) (warp.py:19-46): feat, dout [N,C,H,W] of one dtype (fp32 / bf16 / fp16),
    flow [N,2,H,W] -> fp32 [N,2,H,W]."""
    _need_cuda(feat, dout, flow)
    N, C, H, W = feat.shape
    ld = (C + 7) // 8 * 8
    x = torch.zeros(N, H, W, ld, dtype=feat.dtype, device=feat.device)
    x[..., :C] = feat.permute(0, 2, 3, 1)
    d = torch.zeros_like(x)
    d[..., :C] = dout.permute(0, 2, 3, 1)
    fl = flow.to(torch.float32).contiguous()
    out = torch.empty(N, 2, H, W, dtype=torch.float32, device=feat.device)
    L.check(L.lib().dbsr_warp_flow_backward(N, H, W, ld, L.tensor_desc(x, ld), L.tensor_desc(d, ld), fl.data_ptr(),
                                            2 * H * W, out.data_ptr(), 2 * H * W, 0, L.stream_ptr(feat.device)),
            'dbsr_warp_flow_backward')
    return out


def backwarp_backward(inp, flow, dout, scale=1.0, need_input=True, need_flow=True):
    """(dL/dinput, dL/dflow) of backwarp(input, flow * scale) (pwcnet.py:16-38; the mask carries no gradient):
    inp, dout [N,C,H,W], flow [N,2,H,W] -> (fp32 [N,C,H,W], fp32 [N,2,H,W]); an unwanted one is None and costs
    nothing."""
    _need_cuda(inp, flow, dout)
    if not (need_input or need_flow):
        return None, None
    N, C, H, W = inp.shape
    x, ldx = _nhwc(inp)
    d, _ = _nhwc(dout, inp.dtype)
    fl = flow.permute(0, 2, 3, 1).to(torch.float32).contiguous()
    din = torch.empty(N, H, W, ldx, dtype=torch.float32, device=inp.device) if need_input else None
    dfl = torch.empty(N, H, W, 2, dtype=torch.float32, device=inp.device) if need_flow else None
    L.check(L.lib().dbsr_backwarp_backward(N, H, W, C, L.tensor_desc(x, ldx), L.tensor_desc(fl, 2), float(scale),
                                           L.tensor_desc(d, ldx),
                                           L.tensor_desc(din, ldx) if need_input else L.NULL_TENSOR,
                                           L.tensor_desc(dfl, 2) if need_flow else L.NULL_TENSOR,
                                           L.stream_ptr(inp.device)), 'dbsr_backwarp_backward')
    return (din[..., :C].permute(0, 3, 1, 2).contiguous() if need_input else None,
            dfl.permute(0, 3, 1, 2).contiguous() if need_flow else None)


def chan_sum(t):
    """Per-channel sum over batch and pixels (the conv bias gradient) of t [N,C,H,W] -> fp32 [C]."""
    _need_cuda(t)
    N, C, H, W = t.shape
    ld = (C + 7) // 8 * 8
    x = torch.zeros(N, H, W, ld, dtype=t.dtype, device=t.device)
    x[..., :C] = t.permute(0, 2, 3, 1)
    out = torch.empty(C, dtype=torch.float32, device=t.device)
    need = L.lib().dbsr_chan_sum_workspace_bytes(N, H * W, C)
    ws = torch.empty(max(need // 4, 1), dtype=torch.float32, device=t.device)
    L.check(L.lib().dbsr_chan_sum(N, H * W, C, L.tensor_desc(x, ld), out.data_ptr(), 0, ws.data_ptr(), need,
                                  L.stream_ptr(t.device)), 'dbsr_chan_sum')
    return out


# The ops below take the NHWC buffers the training plan passes ([images, ..., ld] device tensors, channels last,
# `c` channels used from c0) and write their output buffer in place, so a caller chooses ld / c0 / padding itself.
def _hw(t):
    return t[0].numel() // t.shape[-1]


def unshuffle_gate(ds, gate, du, s, c):
    """dbsr_unshuffle_gate: ds / gate [B, H*s, W*s, ld] (c channels), du [B, H, W, ldu >= c*s*s] written in torch's
    pixel_unshuffle channel order, du = unshuffle([gate > 0] * ds).  Returns du."""
    _need_cuda(ds, gate, du)
    B, H, W = du.shape[:3]
    L.check(L.lib().dbsr_unshuffle_gate(B, H, W, s, c, L.tensor_desc(ds, ds.shape[-1]),
                                        L.tensor_desc(gate, gate.shape[-1]), L.tensor_desc(du, du.shape[-1]),
                                        L.stream_ptr(ds.device)), 'dbsr_unshuffle_gate')
    return du


def merge_prep_backward(dwp, proj, dproj, N, c):
    """dbsr_merge_prep_backward: dwp [B*N, ..., ld >= 2c] (channels [0,c) d base, [c,2c) d diff), proj / dproj
    [B*N, ..., ld >= c].  Returns dproj."""
    _need_cuda(dwp, proj, dproj)
    L.check(L.lib().dbsr_merge_prep_backward(dwp.shape[0] // N, N, _hw(dwp), c, L.tensor_desc(dwp, dwp.shape[-1]),
                                             L.tensor_desc(proj, proj.shape[-1]),
                                             L.tensor_desc(dproj, dproj.shape[-1]), L.stream_ptr(dwp.device)),
            'dbsr_merge_prep_backward')
    return dproj


def gate_copy(inp, gate, out, c, out_c0=0, gate_map=L.IDENTITY):
    """dbsr_gate_copy: out[f][.., out_c0 : out_c0 + c] = [gate[gate_map(f)] > 0] * inp[f] over inp's images.
    Returns out."""
    _need_cuda(inp, gate, out)
    L.check(L.lib().dbsr_gate_copy(inp.shape[0], _hw(inp), c, L.tensor_desc(inp, inp.shape[-1]),
                                   L.tensor_desc(gate, gate.shape[-1], fmap=gate_map),
                                   L.tensor_desc(out, out.shape[-1], out_c0), L.stream_ptr(inp.device)),
            'dbsr_gate_copy')
    return out


def enc_grad_gate(dref, dsrc32, e, de, N, c):
    """dbsr_enc_grad_gate: dref [B, ..., ld], dsrc32 fp32 [B*N, ..., c] (dense), e / de [B*N, ..., ld]:
    de[b*N+n] = [e > 0] * (n == 0 ? dref[b] : dsrc32[b*N+n]).  Returns de."""
    _need_cuda(dref, dsrc32, e, de)
    if dsrc32.dtype != torch.float32 or not dsrc32.is_contiguous() or dsrc32.shape[-1] != c:
        raise ValueError('enc_grad_gate: dsrc32 must be a contiguous fp32 [B*N, ..., c] tensor')
    L.check(L.lib().dbsr_enc_grad_gate(dref.shape[0], N, _hw(e), c, L.tensor_desc(dref, dref.shape[-1]),
                                       dsrc32.data_ptr(), L.tensor_desc(e, e.shape[-1]),
                                       L.tensor_desc(de, de.shape[-1]), L.stream_ptr(e.device)),
            'dbsr_enc_grad_gate')
    return de


def relu_grad(pred, gout, dpre):
    """dbsr_relu_grad: pred / gout fp32 NCHW [B,C,H,W] -> dpre [B,H,W,ld >= C] = [pred > 0] * gout in dpre's dtype
    (channels C.. of dpre are left as they are).  Returns dpre."""
    _need_cuda(pred, gout, dpre)
    B, C, H, W = pred.shape
    pred, gout = _f32c(pred), _f32c(gout)
    L.check(L.lib().dbsr_relu_grad(B, C, H, W, pred.data_ptr(), gout.data_ptr(), L.tensor_desc(dpre, dpre.shape[-1]),
                                   L.stream_ptr(pred.device)), 'dbsr_relu_grad')
    return dpre


def head_backward(h, dp, w, hc, dh):
    """dbsr_head_backward: h / dh [n, ..., ld >= 32], dp [n, ..., 8] (hc channels used), w fp32 [hc, 32]: dh (in
    place) = [h > 0] * (w^T . dp).  Returns (dh, dw fp32 [hc, 32], db fp32 [hc])."""
    _need_cuda(h, dp, w, dh)
    dev = h.device
    n, hw = h.shape[0], _hw(h)
    wd = w.reshape(hc, 32).to(torch.float32).contiguous()
    dw = torch.zeros(hc, 32, dtype=torch.float32, device=dev)
    db = torch.zeros(hc, dtype=torch.float32, device=dev)
    need = L.lib().dbsr_head_backward_workspace_bytes(n, hw, 32, hc)
    ws = torch.empty(need // 4 + 1, dtype=torch.float32, device=dev)
    L.check(L.lib().dbsr_head_backward(n, hw, L.tensor_desc(h, h.shape[-1]), 32, L.tensor_desc(dp, dp.shape[-1]),
                                       wd.data_ptr(), hc, L.tensor_desc(dh, dh.shape[-1]), dw.data_ptr(),
                                       db.data_ptr(), 0, ws.data_ptr(), need, L.stream_ptr(dev)),
            'dbsr_head_backward')
    return dh, dw, db


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0, n=None):
    """dbsr_adam_step on the first n (default: all) elements of flat contiguous fp32 device tensors, in place."""
    _need_cuda(param, grad, exp_avg, exp_avg_sq)
    n = param.numel() if n is None else int(n)
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise ValueError('adam_step: contiguous fp32 tensors of at least n elements')
    L.check(L.lib().dbsr_adam_step(n, param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                                   float(lr), float(betas[0]), float(betas[1]), float(eps), int(step),
                                   float(grad_scale), L.stream_ptr(param.device)), 'dbsr_adam_step')


def dgrad_weights(weight):
    """dbsr_dgrad_weights: fp32 [cout, cin, kh, kw] -> [cin, cout, kh, kw], transposed and spatially flipped."""
    _need_cuda(weight)
    cout, cin, kh, kw = weight.shape
    w32 = weight.to(torch.float32).contiguous()
    wt = torch.empty(cin, cout, kh, kw, dtype=torch.float32, device=weight.device)
    L.check(L.lib().dbsr_dgrad_weights(w32.data_ptr(), cout, cin, kh, kw, wt.data_ptr(), L.stream_ptr(weight.device)),
            'dbsr_dgrad_weights')
    return wt


# ---------------------------------------------------------------------------------------------------
# real-world fine-tuning objective (csrc/sca_train.hip; dbsr_hip.h 'real-world fine-tuning objective')
# ---------------------------------------------------------------------------------------------------
def _f32c(t):
    return None if t is None else t.to(torch.float32).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def aligned_l1_forward(pred, gt, flow, c_mat, valid, boundary_ignore, weight=1.0):
    """dbsr_aligned_l1_forward on fp32 NCHW device tensors: returns (loss2 [2] = {loss, gradient scale}, g_pw
    [B,3,H,W] the unnormalised dL/dwarp(pred), stats [B,2] = {masked squared-error sum, valid count} per image)."""
    _need_cuda(pred, gt)
    B, C, H, W = pred.shape
    if C != 3 or gt.shape != pred.shape:
        raise ValueError('aligned_l1: pred and gt must be [B, 3, H, W]')
    dev = pred.device
    pred, gt, flow, c_mat = _f32c(pred), _f32c(gt), _f32c(flow), _f32c(c_mat)
    v8 = None if valid is None else valid.to(torch.uint8).contiguous()
    need = L.lib().dbsr_aligned_l1_workspace_bytes(B, H, W)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    g_pw = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev)
    loss2 = torch.empty(2, dtype=torch.float32, device=dev)
    stats = torch.empty(B, 2, dtype=torch.float32, device=dev)
    L.check(L.lib().dbsr_aligned_l1_forward(B, H, W, int(boundary_ignore), pred.data_ptr(), _ptr(flow), _ptr(c_mat),
                                            _ptr(v8), gt.data_ptr(), float(weight), g_pw.data_ptr(),
                                            loss2.data_ptr(), stats.data_ptr(), ws.data_ptr(), need,
                                            L.stream_ptr(dev)), 'dbsr_aligned_l1_forward')
    return loss2, g_pw, stats


def aligned_l1_backward(g_pw, flow, pred=None, c_mat=None, scale=None, want_gpred=True, dpre_dtype=None):
    """dbsr_aligned_l1_backward: dpred = scale * warp^T(c_mat g_pw) (scale: a 1-element device tensor or None;
    c_mat None: g_pw as it is).  Returns (gpred fp32 [B,3,H,W] or None, dpre [B,H,W,8] of dpre_dtype = the
    ReLU-gated NHWC copy for the predictor's backward, or None)."""
    _need_cuda(g_pw)
    B, _, H, W = g_pw.shape
    dev = g_pw.device
    g_pw, flow, c_mat, pred = _f32c(g_pw), _f32c(flow), _f32c(c_mat), _f32c(pred)
    need = L.lib().dbsr_aligned_l1_workspace_bytes(B, H, W)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    gpred = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if want_gpred else None
    dpre = torch.zeros(B, H, W, 8, dtype=dpre_dtype, device=dev) if dpre_dtype is not None else None
    L.check(L.lib().dbsr_aligned_l1_backward(B, H, W, _ptr(pred), _ptr(flow), g_pw.data_ptr(), _ptr(c_mat),
                                             _ptr(scale), _ptr(gpred),
                                             L.tensor_desc(dpre, 8) if dpre is not None else L.NULL_TENSOR,
                                             ws.data_ptr(), need, L.stream_ptr(dev)), 'dbsr_aligned_l1_backward')
    return gpred, dpre


def aligned_l1(pred, gt, flow, c_mat, valid, boundary_ignore, weight=1.0):
    """The aligned L1 objective of the real-world recipe (actors/dbsr_actors.py:68-80) and its gradient:
    loss = weight * sum(valid |warp(pred, flow)^T c_mat - gt|) / (3 sum(valid) + 1e-12) over the
    boundary_ignore crop (flow [B,2,H,W] px, c_mat [B,3,3], valid [B,1,H,W]; each may be None).  Returns
    (loss [1], dpred [B,3,H,W]) as device tensors; nothing is read back."""
    loss2, g_pw, _ = aligned_l1_forward(pred, gt, flow, c_mat, valid, boundary_ignore, weight)
    gpred, _ = aligned_l1_backward(g_pw, flow, scale=loss2[1:])
    return loss2[:1], gpred


# ---------------------------------------------------------------------------------------------------
# image-quality metrics (csrc/metrics.hip; dbsr_hip.h 'image-quality metrics')
# ---------------------------------------------------------------------------------------------------
def _ssim_args(pred, gt, valid, boundary_ignore):
    _need_cuda(pred, gt)
    if pred.dim() != 4 or gt.shape != pred.shape:
        raise ValueError('ssim: pred and gt must be [B, C, H, W] of one shape')
    if pred.dtype != torch.float32 or gt.dtype != torch.float32:
        raise ValueError('ssim: pred and gt must be float32')
    B, _, H, W = pred.shape
    v8 = None
    if valid is not None:
        if valid.numel() != B * H * W:
            raise ValueError('ssim: valid must be [B, 1, H, W]')
        v8 = valid.to(torch.uint8).contiguous()
    return pred.contiguous(), gt.contiguous(), v8, int(boundary_ignore or 0)


def ssim_forward(pred, gt, valid=None, boundary_ignore=0, val_range=1.0, want_map=False):
    """dbsr_ssim_forward on fp32 NCHW device tensors: returns (result [2] = {masked mean SSIM, gradient scale},
    sums [B,2] = {masked SSIM sum, valid window count} per image, map [B,C,H-2bi-10,W-2bi-10] or None)."""
    pred, gt, v8, bi = _ssim_args(pred, gt, valid, boundary_ignore)
    B, C, H, W = pred.shape
    dev = pred.device
    need = L.lib().dbsr_ssim_workspace_bytes(B, C, H, W, bi)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    smap = torch.empty(B, C, max(H - 2 * bi - 10, 0), max(W - 2 * bi - 10, 0), dtype=torch.float32,
                       device=dev) if want_map else None
    sums = torch.empty(B, 2, dtype=torch.float32, device=dev)
    result = torch.empty(2, dtype=torch.float32, device=dev)
    L.check(L.lib().dbsr_ssim_forward(B, C, H, W, bi, pred.data_ptr(), gt.data_ptr(), _ptr(v8), float(val_range),
                                      _ptr(smap), sums.data_ptr(), result.data_ptr(), ws.data_ptr(), need,
                                      L.stream_ptr(dev)), 'dbsr_ssim_forward')
    return result, sums, smap


def ssim_backward(pred, gt, valid=None, boundary_ignore=0, val_range=1.0, scale=None):
    """dbsr_ssim_backward: scale * d(sum valid * S)/dpred as fp32 [B,C,H,W], zero outside the crop (scale: a
    1-element device tensor, e.g. ssim_forward's result[1:]; None: 1)."""
    pred, gt, v8, bi = _ssim_args(pred, gt, valid, boundary_ignore)
    B, C, H, W = pred.shape
    dev = pred.device
    if scale is None:
        scale = torch.ones(1, dtype=torch.float32, device=dev)
    scale = scale.to(torch.float32).contiguous()
    gpred = torch.empty_like(pred)
    L.check(L.lib().dbsr_ssim_backward(B, C, H, W, bi, pred.data_ptr(), gt.data_ptr(), _ptr(v8), float(val_range),
                                       scale.data_ptr(), gpred.data_ptr(), None, 0, L.stream_ptr(dev)),
            'dbsr_ssim_backward')
    return gpred


def ssim(pred, gt, valid=None, boundary_ignore=0, val_range=1.0):
    """Masked mean SSIM (image_quality_v2.SSIM with use_for_loss=False) and its gradient: returns (ssim [1],
    dssim/dpred [B,C,H,W]) as device tensors; nothing is read back."""
    result, _, _ = ssim_forward(pred, gt, valid, boundary_ignore, val_range)
    return result[:1], ssim_backward(pred, gt, valid, boundary_ignore, val_range, scale=result[1:])


# ---------------------------------------------------------------------------------------------------
# LPIPS (csrc/lpips.hip around dbsr_conv2d in fp32; dbsr_hip.h 'image-quality metrics')
# ---------------------------------------------------------------------------------------------------
LPIPS_NET_CODE = {'alex': 0, 'vgg': 1}


def _f32_dev(what, *ts):
    _need_cuda(*ts)
    for t in ts:
        if t.dtype != torch.float32:
            raise ValueError('%s: tensors must be float32' % what)


def lpips_prep(pred, gt, boundary_ignore=0, net='alex', bgr2rgb=False, normalize=False, out=None):
    """dbsr_lpips_prep: pred, gt [B,3,H,W] fp32 NCHW -> [2B,Hc,Wc,8] fp32 NHWC (pred images first): crop, optional
    channel flip, optional 2x - 1, (x - shift) / scale; channels 3..7 zero."""
    _f32_dev('lpips_prep', pred, gt)
    if pred.dim() != 4 or pred.shape[1] != 3 or gt.shape != pred.shape:
        raise ValueError('lpips_prep: pred and gt must be [B, 3, H, W] of one shape')
    B, _, H, W = pred.shape
    bi = int(boundary_ignore or 0)
    pred, gt = pred.contiguous(), gt.contiguous()
    if out is None:
        out = torch.empty(2 * B, max(H - 2 * bi, 0), max(W - 2 * bi, 0), 8, dtype=torch.float32, device=pred.device)
    L.check(L.lib().dbsr_lpips_prep(B, H, W, bi, LPIPS_NET_CODE[net], int(bool(bgr2rgb)), int(bool(normalize)),
                                    pred.data_ptr(), gt.data_ptr(), out.data_ptr(), L.stream_ptr(pred.device)),
            'dbsr_lpips_prep')
    return out


def maxpool2d(x, k, s, out=None):
    """dbsr_maxpool2d on an fp32 NHWC device tensor [N,H,W,C] (contiguous, C % 4 == 0): k x k / stride s, floor mode,
    no padding -> [N,(H-k)//s+1,(W-k)//s+1,C]."""
    _f32_dev('maxpool2d', x)
    if x.dim() != 4 or not x.is_contiguous():
        raise ValueError('maxpool2d: x must be a contiguous [N, H, W, C] tensor')
    N, H, W, C = x.shape
    if out is None:
        out = torch.empty(N, max((H - k) // s + 1, 0), max((W - k) // s + 1, 0), C, dtype=torch.float32,
                          device=x.device)
    L.check(L.lib().dbsr_maxpool2d(N, H, W, C, int(k), int(s), x.data_ptr(), C, out.data_ptr(), C,
                                   L.stream_ptr(x.device)), 'dbsr_maxpool2d')
    return out


def lpips_layer(feat, lin, layer=0, want_map=False, per_layer=None, value=None, ws=None, dmap=None):
    """dbsr_lpips_layer on one tapped feature tensor [2B,h,w,C] fp32 NHWC (pred images first) and lin [C]: returns
    (value [B], per_layer [B,5], map [B,h,w] or None).  per_layer[:, layer] is this layer's mean distance; value is
    set to it for layer 0 and has it added for layers 1..4 (pass the same per_layer / value for all five)."""
    _f32_dev('lpips_layer', feat, lin)
    if feat.dim() != 4 or feat.shape[0] % 2 or not feat.is_contiguous():
        raise ValueError('lpips_layer: feat must be a contiguous [2B, h, w, C] tensor')
    N, h, w, C = feat.shape
    B = N // 2
    if lin.numel() != C:
        raise ValueError('lpips_layer: lin must hold C = %d weights' % C)
    dev = feat.device
    lin = lin.contiguous()
    need = L.lib().dbsr_lpips_layer_workspace_bytes(B, h, w, C)
    if ws is None:
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    if per_layer is None:
        per_layer = torch.zeros(B, 5, dtype=torch.float32, device=dev)
    if value is None:
        value = torch.zeros(B, dtype=torch.float32, device=dev)
    if want_map and dmap is None:
        dmap = torch.empty(B, h, w, dtype=torch.float32, device=dev)
    L.check(L.lib().dbsr_lpips_layer(B, h, w, C, int(layer), feat.data_ptr(), lin.data_ptr(),
                                     _ptr(dmap if want_map else None), per_layer.data_ptr(), value.data_ptr(),
                                     ws.data_ptr(), need, L.stream_ptr(dev)), 'dbsr_lpips_layer')
    return value, per_layer, (dmap if want_map else None)


def lpips_layer_backward(feat, lin, gvalue=None, out=None, accumulate=False):
    """dbsr_lpips_layer_backward: feat [2B,h,w,C] and lin as for lpips_layer, gvalue [B] the upstream gradient of
    value (None: ones) -> d(sum_b gvalue[b] per_layer[b]) / d feat[:B] as [B,h,w,C], written to `out` or, with
    accumulate, added to it.  At an all-zero pred vector it is the limit g / 1e-10 (finite), not autograd's NaN."""
    _f32_dev('lpips_layer_backward', feat, lin)
    if feat.dim() != 4 or feat.shape[0] % 2 or not feat.is_contiguous():
        raise ValueError('lpips_layer_backward: feat must be a contiguous [2B, h, w, C] tensor')
    N, h, w, C = feat.shape
    B = N // 2
    if lin.numel() != C:
        raise ValueError('lpips_layer_backward: lin must hold C = %d weights' % C)
    dev = feat.device
    if gvalue is None:
        gvalue = torch.ones(B, dtype=torch.float32, device=dev)
    _f32_dev('lpips_layer_backward', gvalue)
    if gvalue.numel() != B:
        raise ValueError('lpips_layer_backward: gvalue must hold B = %d values' % B)
    if out is None:
        if accumulate:
            raise ValueError('lpips_layer_backward: accumulate needs `out`')
        out = torch.empty(B, h, w, C, dtype=torch.float32, device=dev)
    _f32_dev('lpips_layer_backward', out)
    if tuple(out.shape) != (B, h, w, C) or not out.is_contiguous():
        raise ValueError('lpips_layer_backward: out must be a contiguous [B, h, w, C] tensor')
    L.check(L.lib().dbsr_lpips_layer_backward(B, h, w, C, feat.data_ptr(), lin.contiguous().data_ptr(),
                                              gvalue.contiguous().data_ptr(), out.data_ptr(), int(bool(accumulate)),
                                              L.stream_ptr(dev)), 'dbsr_lpips_layer_backward')
    return out


def maxpool2d_backward(x, dy, k, s, out=None):
    """dbsr_maxpool2d_backward: x [N,H,W,C] the pool's input, dy [N,oh,ow,C] -> dx [N,H,W,C], each element the sum of
    dy over the windows whose first maximum it is; every element is written (k / s: 3 / 2 or 2 / 2)."""
    _f32_dev('maxpool2d_backward', x, dy)
    if x.dim() != 4 or not x.is_contiguous() or not dy.is_contiguous():
        raise ValueError('maxpool2d_backward: x and dy must be contiguous [N, H, W, C] tensors')
    N, H, W, C = x.shape
    if tuple(dy.shape) != (N, (H - k) // s + 1, (W - k) // s + 1, C):
        raise ValueError('maxpool2d_backward: dy %s does not belong to x %s' % (tuple(dy.shape), tuple(x.shape)))
    if out is None:
        out = torch.empty_like(x)
    L.check(L.lib().dbsr_maxpool2d_backward(N, H, W, C, int(k), int(s), x.data_ptr(), dy.data_ptr(), out.data_ptr(),
                                            L.stream_ptr(x.device)), 'dbsr_maxpool2d_backward')
    return out


def lpips_stem_backward(dy, w, shape, boundary_ignore=0, net='alex', bgr2rgb=False, normalize=False, out=None):
    """dbsr_lpips_stem_backward: dy [B,oh,ow,64] (the gradient of the first conv's pre-activation) and that conv's
    weights w [64,3,k,k] -> gpred of `shape` [B,3,H,W]: the conv's transpose and dbsr_lpips_prep's, every element
    written (zeros in the boundary_ignore frame)."""
    _f32_dev('lpips_stem_backward', dy, w)
    B, _, H, W = shape
    bi = int(boundary_ignore or 0)
    k, s, p = (11, 4, 2) if net == 'alex' else (3, 1, 1)
    oh, ow = (H - 2 * bi + 2 * p - k) // s + 1, (W - 2 * bi + 2 * p - k) // s + 1
    if tuple(dy.shape) != (B, oh, ow, 64) or not dy.is_contiguous() or tuple(w.shape) != (64, 3, k, k):
        raise ValueError('lpips_stem_backward (%s): dy must be [%d, %d, %d, 64] and w [64, 3, %d, %d]'
                         % (net, B, oh, ow, k, k))
    if out is None:
        out = torch.empty(B, 3, H, W, dtype=torch.float32, device=dy.device)
    L.check(L.lib().dbsr_lpips_stem_backward(B, H, W, bi, LPIPS_NET_CODE[net], int(bool(bgr2rgb)), int(bool(normalize)),
                                             dy.data_ptr(), w.contiguous().data_ptr(), out.data_ptr(),
                                             L.stream_ptr(dy.device)), 'dbsr_lpips_stem_backward')
    return out


def _lpips_dgrad_pack(w, k_channels):
    """A stride-1 backbone conv's weights [cout,cin,k,k] (fp32, device) -> the packed slices of its input-gradient
    conv, which reads dy's cout channels in blocks of k_channels: [(c0, n, packed weights), ...].  The dgrad conv's
    weights are the flipped transpose, wd[ci][co][ky][kx] = w[co][ci][k-1-ky][k-1-kx]."""
    cout, cin, k, _ = w.shape
    wd = w.detach().float().flip(2, 3).transpose(0, 1).contiguous()
    s = L.stream_ptr(w.device)
    slices = []
    for c0 in range(0, cout, k_channels):
        n = min(k_channels, cout - c0)
        ws = wd[:, c0:c0 + n].contiguous()
        wp = torch.empty(L.lib().dbsr_conv_packed_elems(cin, n, k, k), dtype=torch.float32, device=w.device)
        L.check(L.lib().dbsr_conv_pack_weights(ws.data_ptr(), None, cin, n, k, k, L.DBSR_F32, 1, wp.data_ptr(), None,
                                               s), 'pack (lpips dgrad)')
        slices.append((c0, n, wp))
    torch.cuda.current_stream(w.device).synchronize()                 # the slices' host copies go out of scope
    return slices


def _lpips_dgrad_descs(slices, dy, dx, part, B, h, w, cin, cout, k, p):
    """The dbsr_conv2d launches of one stride-1 input gradient: dy [B,h,w,cout] -> dx [B,h,w,cin], per image (the
    forward's rule: an image's rounding must not depend on its batch) and per block of dy's channels, each block's
    result riding in as the next one's residual through part[0] / part[1].  Returns (descs, workspace)."""
    descs = []
    for b in range(B):
        for i, (c0, n, wp) in enumerate(slices):
            last = i == len(slices) - 1
            d = L.ConvDesc()
            d.n_frames = 1
            d.x = L.tensor_desc(dy, cout, c0=c0, fmap=(1, 1, b, 1))
            d.in_h, d.in_w, d.cin = h, w, n
            d.w, d.bias = wp.data_ptr(), None
            d.cout, d.kh, d.kw, d.stride, d.pad, d.dil = cin, k, k, 1, k - 1 - p, 1
            d.y = L.tensor_desc(dx if last else part[i % 2], cin, fmap=(1, 1, b, 1))
            d.out_h, d.out_w = h, w
            d.res = L.tensor_desc(part[(i - 1) % 2], cin, fmap=(1, 1, b, 1)) if i else L.NULL_TENSOR
            d.act, d.post_act = L.ACT_NONE, L.ACT_NONE
            d.out_mode, d.shuffle = L.OUT_NHWC, 0
            d.workspace_bytes = L.lib().dbsr_conv_workspace_bytes(d)
            descs.append(d)
    ws = torch.zeros(max(max(d.workspace_bytes for d in descs) // 4, 1), dtype=torch.float32, device=dy.device)
    for d in descs:
        d.workspace = ws.data_ptr()
    return descs, ws


def lpips_conv_dgrad(dy, w, padding, k_channels=None):
    """The input gradient of a stride-1 backbone conv exactly as LPIPSPlan.backward launches it: dy [B,h,w,cout]
    fp32 NHWC and the conv's weights w [cout,cin,k,k] -> dx [B,h,w,cin] (2 * padding == k - 1)."""
    _f32_dev('lpips_conv_dgrad', dy, w)
    B, h, wd_, cout = dy.shape
    cin, k = w.shape[1], w.shape[2]
    if w.shape[0] != cout or 2 * padding != k - 1 or not dy.is_contiguous():
        raise ValueError('lpips_conv_dgrad: dy [B,h,w,cout] contiguous, w [cout,cin,k,k], 2 * padding == k - 1')
    slices = _lpips_dgrad_pack(w, k_channels or LPIPSPlan.K_CHANNELS)
    dx = torch.empty(B, h, wd_, cin, dtype=torch.float32, device=dy.device)
    part = [torch.empty_like(dx) for _ in range(min(2, len(slices) - 1))]
    descs, ws = _lpips_dgrad_descs(slices, dy, dx, part, B, h, wd_, cin, cout, k, padding)
    s = L.stream_ptr(dy.device)
    for d in descs:
        L.check(L.lib().dbsr_conv2d(d, s), 'dbsr_conv2d (lpips dgrad)')
    torch.cuda.current_stream(dy.device).synchronize()                # ws and part go out of scope
    return dx


class LPIPSPlan:
    """The whole LPIPS forward on the device for one set of weights (evaluation.load_lpips_weights' dict, tensors on
    the HIP device): prep -> fp32 dbsr_conv2d with ReLU in the epilogue / dbsr_maxpool2d, NHWC with ld = C
    throughout -> dbsr_lpips_layer at each of the five taps.  Weights are packed once; activations, workspaces
    and results are allocated at the first call for a shape (B, H, W, boundary_ignore, want_maps) and reused, so
    later calls for that shape allocate nothing and the sequence can be captured in a graph.  forward() returns
    (value [B], per_layer [B,5], maps or None): views of the plan's buffers, overwritten by the next call.
    backward() is the gradient of the last forward's value with respect to pred (csrc/lpips_grad.hip and the
    convs' input gradients through dbsr_conv2d; DESIGN.md, 'LPIPS as a training objective'); its weights and
    buffers are made at the first backward, so a plan that only scores pays nothing for it.

    Each conv runs per image pair and per block of K_CHANNELS input channels (see _build).  32 is where the
    device's distance maps are as close to float64 as the float32 CPU restatement's ('LPIPS': at the
    384 x 384 scoring shape VGG's deepest map is 5.8x the restatement's error unblocked, 3.3x at 128, 1.6x at 64,
    1.2x at 32, for 2.9 / 3.4 / 4.0 / 5.5 ms)."""
    K_CHANNELS = 32

    def __init__(self, weights):
        from .evaluation import LPIPS_NETS
        self.net = weights['net']
        self.spec = LPIPS_NETS[self.net]
        self.device = weights['lin'][0].device
        _need_cuda(*weights['conv_w'], *weights['conv_b'], *weights['lin'])
        s = L.stream_ptr(self.device)
        self.packed = []                                    # per conv: [(c0, n, packed weights, bias | None), ...]
        for (cin, cout, k, _, _), w, b in zip(self.spec['convs'], weights['conv_w'], weights['conv_b']):
            if tuple(w.shape) != (cout, cin, k, k) or tuple(b.shape) != (cout,):
                raise ValueError('LPIPSPlan: conv %d -> %d has weights %s / bias %s' % (cin, cout, tuple(w.shape),
                                                                                      tuple(b.shape)))
            w32, b32 = w.detach().float().contiguous(), b.detach().float().contiguous()
            slices = []
            for c0 in range(0, cin, self.K_CHANNELS):
                n = min(self.K_CHANNELS, cin - c0)
                ws = w32[:, c0:c0 + n].contiguous()
                wp = torch.empty(L.lib().dbsr_conv_packed_elems(cout, n, k, k), dtype=torch.float32, device=self.device)
                bp = torch.empty(cout, dtype=torch.float32, device=self.device) if c0 == 0 else None
                L.check(L.lib().dbsr_conv_pack_weights(ws.data_ptr(), b32.data_ptr() if c0 == 0 else None, cout, n, k,
                                                       k, L.DBSR_F32, 1, wp.data_ptr(), _ptr(bp), s), 'pack')
                slices.append((c0, n, wp, bp))
            torch.cuda.current_stream(self.device).synchronize()      # the slices' host copies go out of scope
            self.packed.append(slices)
        self.lins = [v.detach().float().reshape(-1).contiguous() for v in weights['lin']]
        self._shapes = {}
        # backward(): the convs' fp32 weights, from which the input-gradient convs are packed at the first backward
        self._w32 = [w.detach().float().contiguous() for w in weights['conv_w']]
        self._dgrad = None
        self._last_key = None

    def _build(self, B, H, W, bi, want_maps):
        """Buffers and the launch list for one shape."""
        dev, f32 = self.device, torch.float32
        h, w, c = H - 2 * bi, W - 2 * bi, 8
        x = torch.empty(2 * B, h, w, c, dtype=f32, device=dev)
        st = {'x0': x, 'steps': [], 'per_layer': torch.zeros(B, 5, dtype=f32, device=dev),
              'value': torch.zeros(B, dtype=f32, device=dev), 'maps': [] if want_maps else None}
        layer = 0
        for op in self.spec['program']:
            if isinstance(op, int):
                cin, cout, k, s, p = self.spec['convs'][op]
                oh, ow = (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1
                y = torch.empty(2 * B, oh, ow, cout, dtype=f32, device=dev)
                # One launch per image pair (frames b and B + b through the frame map): dbsr_conv2d picks its tile
                # and split-K from the total pixel count, so a conv over the whole batch would round an image's
                # features differently at B = 3 than at B = 1.  Two frames per launch is the B = 1 dispatch.
                # K is summed in blocks of K_CHANNELS input channels, one launch per block, each block's result
                # riding in as the next one's residual (bias in the first, ReLU after the last): the kernels'
                # K-ordered fp32 chain over all of 9 x 512 non-negative products drifts several times further from
                # the float64 value than a blocked sum does ('LPIPS').
                slices = self.packed[op]
                part = [torch.empty_like(y) for _ in range(min(2, len(slices) - 1))]
                descs = []
                for b in range(B):
                    for i, (c0, n, wp, bp) in enumerate(slices):
                        last = i == len(slices) - 1
                        d = L.ConvDesc()
                        d.n_frames = 2
                        d.x = L.tensor_desc(x, c, c0=c0, fmap=(1, B, b, 1))
                        d.in_h, d.in_w, d.cin = h, w, n
                        d.w, d.bias = wp.data_ptr(), _ptr(bp)
                        d.cout, d.kh, d.kw, d.stride, d.pad, d.dil = cout, k, k, s, p, 1
                        d.y = L.tensor_desc(y if last else part[i % 2], cout, fmap=(1, B, b, 1))
                        d.out_h, d.out_w = oh, ow
                        d.res = L.tensor_desc(part[(i - 1) % 2], cout, fmap=(1, B, b, 1)) if i else L.NULL_TENSOR
                        if len(slices) == 1:
                            d.act, d.post_act = L.ACT_RELU, L.ACT_NONE
                        else:
                            d.act, d.post_act = L.ACT_NONE, (L.ACT_RELU if last else L.ACT_NONE)
                        d.out_mode, d.shuffle = L.OUT_NHWC, 0
                        d.workspace_bytes = L.lib().dbsr_conv_workspace_bytes(d)
                        descs.append(d)
                # the launches run in stream order and share one split-K workspace
                ws = torch.zeros(max(max(d.workspace_bytes for d in descs) // 4, 1), dtype=f32, device=dev)
                for d in descs:
                    d.workspace = ws.data_ptr()
                st['steps'].append(('conv', descs, (x, y, ws, part, op)))
                x, h, w, c = y, oh, ow, cout
            elif op == 'tap':
                need = L.lib().dbsr_lpips_layer_workspace_bytes(B, h, w, c)
                if need == 0:
                    raise L.DBSRLibError('lpips: tap %d of shape [%d, %d, %d, %d] is refused' % (layer, 2 * B, h, w, c))
                ws = torch.empty(need, dtype=torch.uint8, device=dev)
                dmap = torch.empty(B, h, w, dtype=f32, device=dev) if want_maps else None
                if want_maps:
                    st['maps'].append(dmap)
                st['steps'].append(('tap', (B, h, w, c, layer, need), (x, ws, dmap)))
                layer += 1
            else:
                _, k, s = op
                y = torch.empty(2 * B, (h - k) // s + 1, (w - k) // s + 1, c, dtype=f32, device=dev)
                st['steps'].append(('pool', (2 * B, h, w, c, k, s), (x, y)))
                x, h, w = y, y.shape[1], y.shape[2]
        return st

    def forward(self, pred, gt, boundary_ignore=0, bgr2rgb=False, normalize=False, want_maps=False):
        _f32_dev('lpips', pred, gt)
        if pred.dim() != 4 or pred.shape[1] != 3 or gt.shape != pred.shape:
            raise ValueError('lpips: pred and gt must be [B, 3, H, W] of one shape')
        if pred.device != self.device or gt.device != self.device:
            raise ValueError('lpips: the images are on %s, the weights on %s' % (pred.device, self.device))
        B, _, H, W = pred.shape
        bi = int(boundary_ignore or 0)
        need = self.spec['min_side']
        if H - 2 * bi < need or W - 2 * bi < need:
            raise ValueError('lpips (%s): the crop %d x %d is smaller than %d x %d (the last pool needs a row)'
                             % (self.net, H - 2 * bi, W - 2 * bi, need, need))
        key = (B, H, W, bi, bool(want_maps))
        st = self._shapes.get(key)
        if st is None:
            st = self._shapes[key] = self._build(B, H, W, bi, want_maps)
        st['gen'] = st.get('gen', 0) + 1                    # backward() belongs to this forward of the shape
        st['args'] = (B, H, W, bi, bool(bgr2rgb), bool(normalize))
        self._last_key = key
        lib, s = L.lib(), L.stream_ptr(self.device)
        lpips_prep(pred, gt, bi, self.net, bgr2rgb, normalize, out=st['x0'])
        for kind, a, bufs in st['steps']:
            if kind == 'conv':
                for d in a:
                    L.check(lib.dbsr_conv2d(d, s), 'dbsr_conv2d (lpips)')
            elif kind == 'pool':
                N, h, w, c, k, ps = a
                L.check(lib.dbsr_maxpool2d(N, h, w, c, k, ps, bufs[0].data_ptr(), c, bufs[1].data_ptr(), c, s),
                        'dbsr_maxpool2d')
            else:
                Bn, h, w, c, layer, need = a
                L.check(lib.dbsr_lpips_layer(Bn, h, w, c, layer, bufs[0].data_ptr(), self.lins[layer].data_ptr(),
                                             _ptr(bufs[2]), st['per_layer'].data_ptr(), st['value'].data_ptr(),
                                             bufs[1].data_ptr(), need, s), 'dbsr_lpips_layer')
        return st['value'], st['per_layer'], st['maps']

    # ------------------------------------------------------------------------------------------ backward
    def token(self):
        """(shape key, generation) of the last forward: pass it to backward() to have a backward that no longer
        belongs to the shape's newest forward refused instead of run on overwritten activations."""
        if self._last_key is None:
            raise RuntimeError('LPIPSPlan: no forward has run')
        return self._last_key, self._shapes[self._last_key]['gen']

    def activations(self, shape_key=None):
        """The activations the last forward of `shape_key` (default: the last forward's) saved, in program order:
        ('relu', y) per conv and ('pool', x, y) per max-pool, [2B,h,w,C] NHWC views of the plan's buffers with the
        pred images first (what backward() gates and routes by)."""
        st = self._shapes[shape_key or self.token()[0]]
        out = []
        for kind, _, bufs in st['steps']:
            if kind == 'conv':
                out.append(('relu', bufs[1]))
            elif kind == 'pool':
                out.append(('pool', bufs[0], bufs[1]))
        return out

    def _build_backward(self, st):
        """Buffers and the launch list of the backward for one shape: the forward's steps in reverse.  Two flat
        gradient buffers alternate (a conv's or pool's input gradient goes to the other one; a tap adds into the
        one that holds its activation's gradient; the ReLU gate runs in place), two more carry the K blocks."""
        if self._dgrad is None:
            self._dgrad = [None] + [_lpips_dgrad_pack(w, self.K_CHANNELS) for w in self._w32[1:]]
        B, H, W, bi = st['args'][:4]
        dev, f32 = self.device, torch.float32
        sizes = [B * b[1].shape[1] * b[1].shape[2] * b[1].shape[3] for k, _, b in st['steps'] if k != 'tap']
        flat = [torch.empty(max(sizes), dtype=f32, device=dev) for _ in range(4)]
        view = lambda i, h, w, c: flat[i][:B * h * w * c].view(B, h, w, c)
        bw = {'gpred': torch.empty(B, 3, H, W, dtype=f32, device=dev), 'ones': torch.ones(B, dtype=f32, device=dev),
              'gvalue': torch.ones(B, dtype=f32, device=dev), 'flat': flat, 'launches': []}
        cur, have = 0, False                               # the buffer of the current activation's gradient
        for kind, a, bufs in reversed(st['steps']):
            if kind == 'tap':
                _, h, w, c, layer, _ = a
                bw['launches'].append(('layer', (B, h, w, c, layer, int(have)), (bufs[0], view(cur, h, w, c))))
                have = True
            elif kind == 'pool':
                _, h, w, c, k, s = a
                oh, ow = bufs[1].shape[1], bufs[1].shape[2]
                bw['launches'].append(('pool', (B, h, w, c, k, s), (bufs[0], view(cur, oh, ow, c),
                                                                   view(cur ^ 1, h, w, c))))
                cur ^= 1
            else:
                x, y, op = bufs[0], bufs[1], bufs[4]
                cin, cout, k, _, p = self.spec['convs'][op]
                oh, ow = y.shape[1], y.shape[2]
                dy = view(cur, oh, ow, cout)
                bw['launches'].append(('gate', (B, oh * ow, cout), (L.tensor_desc(dy, cout), L.tensor_desc(y, cout))))
                if op == 0:
                    bw['launches'].append(('stem', None, (dy,)))
                else:
                    h, w = x.shape[1], x.shape[2]
                    dx = view(cur ^ 1, h, w, cin)
                    part = [view(2, h, w, cin), view(3, h, w, cin)]
                    descs, ws = _lpips_dgrad_descs(self._dgrad[op], dy, dx, part, B, h, w, cin, cout, k, p)
                    bw['launches'].append(('conv', descs, (dy, dx, ws, part)))
                    cur ^= 1
        return bw

    def backward(self, gvalue=None, token=None):
        """d(sum_b gvalue[b] value[b]) / d pred of the last forward() (of `token`'s shape when given), fp32
        [B,3,H,W]: a view of the plan's buffer, overwritten by the next backward of that shape.  gvalue: [B] device
        tensor, None = ones.  With `token` (from token() right after the forward) a backward that no longer belongs
        to the shape's newest forward raises RuntimeError: the saved activations are gone."""
        key, gen = token if token is not None else self.token()
        st = self._shapes[key]
        if st['gen'] != gen:
            raise RuntimeError('LPIPSPlan: backward() after another forward of the same shape -- the saved '
                               'activations are gone (one forward per backward)')
        bw = st.get('bwd')
        if bw is None:
            bw = st['bwd'] = self._build_backward(st)
        B, H, W, bi, bgr2rgb, normalize = st['args']
        if gvalue is None:
            gv = bw['ones']
        else:
            if gvalue.device != self.device or gvalue.numel() != B:
                raise ValueError('lpips backward: gvalue must hold B = %d values on %s' % (B, self.device))
            gv = bw['gvalue']
            gv.copy_(gvalue.detach().reshape(-1))
        lib, s = L.lib(), L.stream_ptr(self.device)
        for kind, a, bufs in bw['launches']:
            if kind == 'layer':
                Bn, h, w, c, layer, acc = a
                L.check(lib.dbsr_lpips_layer_backward(Bn, h, w, c, bufs[0].data_ptr(), self.lins[layer].data_ptr(),
                                                      gv.data_ptr(), bufs[1].data_ptr(), acc, s),
                        'dbsr_lpips_layer_backward')
            elif kind == 'pool':
                Bn, h, w, c, k, ps = a
                L.check(lib.dbsr_maxpool2d_backward(Bn, h, w, c, k, ps, bufs[0].data_ptr(), bufs[1].data_ptr(),
                                                    bufs[2].data_ptr(), s), 'dbsr_maxpool2d_backward')
            elif kind == 'gate':
                Bn, hw, c = a
                L.check(lib.dbsr_act_backward(Bn, hw, c, L.ACT_RELU, bufs[0], bufs[1], bufs[0], s),
                        'dbsr_act_backward (lpips)')
            elif kind == 'conv':
                for d in a:
                    L.check(lib.dbsr_conv2d(d, s), 'dbsr_conv2d (lpips dgrad)')
            else:
                L.check(lib.dbsr_lpips_stem_backward(B, H, W, bi, LPIPS_NET_CODE[self.net], int(bgr2rgb),
                                                     int(normalize), bufs[0].data_ptr(), self._w32[0].data_ptr(),
                                                     bw['gpred'].data_ptr(), s), 'dbsr_lpips_stem_backward')
        return bw['gpred']


# ---------------------------------------------------------------------------------------------------
# synthetic training data (csrc/synth_ops.hip; dbsr_hip.h 'synthetic training data')
# ---------------------------------------------------------------------------------------------------
def _cam_params(params, B, what):
    if params.shape != (B, 16) or params.dtype != torch.float32 or not params.is_cuda:
        raise ValueError('%s: params must be a float32 device tensor [B, 16]' % what)
    return params.contiguous()


def unprocess_rgb(src, params):
    """dbsr_unprocess_rgb: src float32 [B,3,Hc,Wc] in [0,1] or uint8 [B,Hc,Wc,3] RGB (device), params [B,16]
    (rgb2cam, rgb / red / blue gain, smoothstep and gamma flags) -> linear sensor image float32 [B,3,Hc,Wc]."""
    _need_cuda(src, params)
    if src.dim() != 4:
        raise ValueError('unprocess_rgb: src must be [B,3,Hc,Wc] float32 or [B,Hc,Wc,3] uint8')
    if src.dtype == torch.uint8:
        B, Hc, Wc, C = src.shape
        fmt = L.SRC_U8_NHWC
    elif src.dtype == torch.float32:
        B, C, Hc, Wc = src.shape
        fmt = L.SRC_F32_NCHW
    else:
        raise ValueError('unprocess_rgb: src must be float32 or uint8, not %s' % src.dtype)
    if C != 3:
        raise ValueError('unprocess_rgb: src must have 3 channels')
    src, params = src.contiguous(), _cam_params(params, B, 'unprocess_rgb')
    lin = torch.empty(B, 3, Hc, Wc, dtype=torch.float32, device=src.device)
    L.check(L.lib().dbsr_unprocess_rgb(B, Hc, Wc, src.data_ptr(), fmt, params.data_ptr(), lin.data_ptr(),
                                       L.stream_ptr(src.device)), 'dbsr_unprocess_rgb')
    return lin


def burst_synth(lin, ainv, border_crop, downsample_factor, noise_levels=None, z=None, want_rgb=True, want_flow=True):
    """dbsr_burst_synth on the linear image lin float32 [B,3,Hc,Wc]: ainv [B,N,2,3] (transformed pixel -> source
    position), noise_levels [B,2] and z [B,N,4,H2/2,W2/2] (both None: no noise).  Returns (burst [B,N,4,H2/2,W2/2],
    burst_rgb [B,N,3,H2,W2] or None, flow [B,N,2,H2,W2] or None)."""
    _need_cuda(lin, ainv)
    if lin.dim() != 4 or lin.shape[1] != 3 or lin.dtype != torch.float32:
        raise ValueError('burst_synth: lin must be float32 [B,3,Hc,Wc]')
    B, _, Hc, Wc = lin.shape
    if ainv.dim() != 4 or ainv.shape[0] != B or tuple(ainv.shape[2:]) != (2, 3):
        raise ValueError('burst_synth: ainv must be [B,N,2,3]')
    N = ainv.shape[1]
    bc, f = int(border_crop or 0), int(downsample_factor)
    dev = lin.device
    lin, ainv = lin.contiguous(), _f32c(ainv)
    H2, W2 = (Hc - 2 * bc) // max(f, 1), (Wc - 2 * bc) // max(f, 1)
    if (z is None) != (noise_levels is None):
        raise ValueError('burst_synth: z and noise_levels go together')
    if z is not None:
        if tuple(z.shape) != (B, N, 4, H2 // 2, W2 // 2) or tuple(noise_levels.shape) != (B, 2):
            raise ValueError('burst_synth: z must be [B,N,4,H2/2,W2/2] and noise_levels [B,2]')
        z, noise_levels = _f32c(z), _f32c(noise_levels)
    shp = lambda c, h, w: (B, N, c, max(h, 0), max(w, 0))                                  # noqa: E731
    burst = torch.empty(shp(4, H2 // 2, W2 // 2), dtype=torch.float32, device=dev)
    rgb = torch.empty(shp(3, H2, W2), dtype=torch.float32, device=dev) if want_rgb else None
    flow = torch.empty(shp(2, H2, W2), dtype=torch.float32, device=dev) if want_flow else None
    L.check(L.lib().dbsr_burst_synth(B, N, Hc, Wc, bc, f, lin.data_ptr(), ainv.data_ptr(), _ptr(noise_levels), _ptr(z),
                                     burst.data_ptr(), _ptr(rgb), _ptr(flow), L.stream_ptr(dev)), 'dbsr_burst_synth')
    return burst, rgb, flow


def postprocess_rgb(img, params, gains=True, ccm=True, gamma=True, smoothstep=True, want_f32=True, want_u8=False):
    """dbsr_postprocess_rgb on img float32 [B,3,H,W] with params [B,16] (cam2rgb, rgb / red / blue gain, the
    meta smoothstep and gamma flags).  Returns (sRGB float32 [B,3,H,W] or None, uint8 [B,H,W,3] RGB or None)."""
    _need_cuda(img, params)
    if img.dim() != 4 or img.shape[1] != 3 or img.dtype != torch.float32:
        raise ValueError('postprocess_rgb: img must be float32 [B,3,H,W]')
    B, _, H, W = img.shape
    img, params = img.contiguous(), _cam_params(params, B, 'postprocess_rgb')
    flags = ((L.POST_GAINS if gains else 0) | (L.POST_CCM if ccm else 0) | (L.POST_GAMMA if gamma else 0) |
             (L.POST_SMOOTHSTEP if smoothstep else 0))
    out = torch.empty_like(img) if want_f32 else None
    u8 = torch.empty(B, H, W, 3, dtype=torch.uint8, device=img.device) if want_u8 else None
    L.check(L.lib().dbsr_postprocess_rgb(B, H, W, img.data_ptr(), params.data_ptr(), flags, _ptr(out), _ptr(u8),
                                         L.stream_ptr(img.device)), 'dbsr_postprocess_rgb')
    return out, u8


# ---------------------------------------------------------------------------------------------------
# dynamic loss scaling (csrc/loss_scale.hip; dbsr_hip.h 'dynamic loss scaling')
# ---------------------------------------------------------------------------------------------------
def loss_scale_state(scale, device):
    """A fresh scaler state buffer (DBSR_LS_WORDS int32 words on `device`; word 0 is the fp32 scale)."""
    st = torch.zeros(L.LS_WORDS, dtype=torch.int32, device=device)
    st.view(torch.float32)[L.LS_SCALE] = float(scale)
    return st


def _ls_check(state, *ts):
    _need_cuda(state, *ts)
    if state.dtype != torch.int32 or state.numel() < L.LS_WORDS or not state.is_contiguous():
        raise ValueError('loss-scale state: a contiguous int32 device tensor of %d words' % L.LS_WORDS)


def l1_loss_backward(pred, gt, boundary_ignore, dpre_dtype=torch.float32, ld=8, state=None):
    """dbsr_l1_loss_backward (state None) or dbsr_l1_loss_backward_scaled on fp32 NCHW device tensors: returns
    (loss [1], dpre [B,H,W,ld] of dpre_dtype)."""
    _need_cuda(pred, gt)
    B, C, H, W = pred.shape
    dev = pred.device
    pred, gt = _f32c(pred), _f32c(gt)
    dpre = torch.zeros(B, H, W, ld, dtype=dpre_dtype, device=dev)
    loss = torch.zeros(1, dtype=torch.float32, device=dev)
    nb = (B * H * W + 255) // 256
    ws = torch.zeros(nb, dtype=torch.float32, device=dev)
    if state is None:
        L.check(L.lib().dbsr_l1_loss_backward(B, C, H, W, int(boundary_ignore), pred.data_ptr(), gt.data_ptr(),
                                              L.tensor_desc(dpre, ld), loss.data_ptr(), ws.data_ptr(), 4 * nb,
                                              L.stream_ptr(dev)), 'dbsr_l1_loss_backward')
    else:
        _ls_check(state)
        L.check(L.lib().dbsr_l1_loss_backward_scaled(B, C, H, W, int(boundary_ignore), pred.data_ptr(), gt.data_ptr(),
                                                     state.data_ptr(), L.tensor_desc(dpre, ld), loss.data_ptr(),
                                                     ws.data_ptr(), 4 * nb, L.stream_ptr(dev)),
                'dbsr_l1_loss_backward_scaled')
    return loss, dpre


def grad_unscale_check(grad, state):
    """dbsr_grad_unscale_check: grad (flat fp32, contiguous; any 4-B aligned view) *= 1 / state.scale in place,
    state.found_inf set on an inf / NaN."""
    _ls_check(state, grad)
    if grad.dtype != torch.float32 or not grad.is_contiguous():
        raise ValueError('grad_unscale_check: a contiguous fp32 tensor')
    L.check(L.lib().dbsr_grad_unscale_check(grad.numel(), grad.data_ptr(), state.data_ptr(),
                                            L.stream_ptr(grad.device)), 'dbsr_grad_unscale_check')
    return grad


def adam_step_guarded(param, grad, exp_avg, exp_avg_sq, state, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0):
    """dbsr_adam_step_guarded on flat contiguous fp32 device tensors, in place."""
    _ls_check(state, param, grad, exp_avg, exp_avg_sq)
    for t in (param, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != param.numel():
            raise ValueError('adam_step_guarded: contiguous fp32 tensors of one size')
    L.check(L.lib().dbsr_adam_step_guarded(param.numel(), param.data_ptr(), grad.data_ptr(), exp_avg.data_ptr(),
                                           exp_avg_sq.data_ptr(), float(lr), float(betas[0]), float(betas[1]),
                                           float(eps), float(grad_scale), state.data_ptr(),
                                           L.stream_ptr(param.device)), 'dbsr_adam_step_guarded')


def loss_scale_update(state, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000):
    """dbsr_loss_scale_update: torch.amp.GradScaler.update on the device state."""
    _ls_check(state)
    L.check(L.lib().dbsr_loss_scale_update(state.data_ptr(), float(growth_factor), float(backoff_factor),
                                           int(growth_interval), L.stream_ptr(state.device)),
            'dbsr_loss_scale_update')


# ---------------------------------------------------------------------------------------------------
# objectives of the training step (csrc/objective.hip; dbsr_hip.h 'objectives of the training step')
# ---------------------------------------------------------------------------------------------------
def _objective_args(pred, gt, metric, boundary_ignore):
    _need_cuda(pred, gt)
    if pred.dim() != 4 or pred.shape[1] != 3 or gt.shape != pred.shape:
        raise ValueError('objective: pred and gt must be [B, 3, H, W] of one shape')
    if metric not in L.METRIC_CODES:
        raise ValueError('objective: unknown metric %r (one of %s)' % (metric, ', '.join(L.METRIC_CODES)))
    return _f32c(pred), _f32c(gt), L.METRIC_CODES[metric], int(boundary_ignore or 0)


def objective_step(pred, gt, boundary_ignore, metric='l1', weight=1.0, gextra=None, state=None,
                   dpre_dtype=torch.float32, ld=8):
    """dbsr_objective_step on fp32 NCHW device tensors [B,3,H,W]: returns (loss [3] = {metric, weight * metric,
    weight / count}, dpre [B,H,W,ld] of dpre_dtype = scale * [pred > 0] * (weight * dmetric/dpred + gextra) in the
    crop, stats [B,2] float64 = {sum (pred - gt)^2, elements} per image).  state: a loss-scale state or None."""
    pred, gt, code, bi = _objective_args(pred, gt, metric, boundary_ignore)
    B, _, H, W = pred.shape
    dev = pred.device
    if gextra is not None:
        _need_cuda(gextra)
        if gextra.shape != pred.shape:
            raise ValueError('objective_step: gextra must have pred\'s shape')
        gextra = _f32c(gextra)
    if state is not None:
        _ls_check(state)
    dpre = torch.zeros(B, H, W, ld, dtype=dpre_dtype, device=dev)
    loss = torch.zeros(3, dtype=torch.float32, device=dev)
    stats = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    need = L.lib().dbsr_objective_workspace_bytes(B, H, W)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    L.check(L.lib().dbsr_objective_step(B, H, W, bi, code, float(weight), pred.data_ptr(), gt.data_ptr(), _ptr(gextra),
                                        _ptr(state), L.tensor_desc(dpre, ld), loss.data_ptr(), stats.data_ptr(),
                                        ws.data_ptr(), need, L.stream_ptr(dev)), 'dbsr_objective_step')
    return loss, dpre, stats


def objective_forward(pred, gt, boundary_ignore, metric='l1', weight=1.0, valid=None, want_grad=True):
    """dbsr_objective_forward: returns (loss [3] = {metric, weight * metric, weight / denominator}, g [B,3,H,W] the
    unnormalised gradient (dloss/dpred = loss[2] / weight * g) or None, stats [B,2] float64).  valid: [B,1,H,W]
    mask, with 'l1' and 'l2' only (the reference's other two metrics cannot take one)."""
    pred, gt, code, bi = _objective_args(pred, gt, metric, boundary_ignore)
    B, _, H, W = pred.shape
    dev = pred.device
    v8 = None
    if valid is not None:
        if metric not in ('l1', 'l2'):
            raise ValueError('objective: metric %r does not take a valid mask (l1 and l2 do)' % (metric,))
        _need_cuda(valid)
        if valid.numel() != B * H * W:
            raise ValueError('objective: valid must be [B, 1, H, W]')
        v8 = valid.to(torch.uint8).contiguous()
    g = torch.empty(B, 3, H, W, dtype=torch.float32, device=dev) if want_grad else None
    loss = torch.zeros(3, dtype=torch.float32, device=dev)
    stats = torch.zeros(B, 2, dtype=torch.float64, device=dev)
    need = L.lib().dbsr_objective_workspace_bytes(B, H, W)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    L.check(L.lib().dbsr_objective_forward(B, H, W, bi, code, float(weight), pred.data_ptr(), gt.data_ptr(), _ptr(v8),
                                           _ptr(g), loss.data_ptr(), stats.data_ptr(), ws.data_ptr(), need,
                                           L.stream_ptr(dev)), 'dbsr_objective_forward')
    return loss, g, stats


def psnr_from_stats(stats, max_value=1.0, max_values=None, masked=False):
    """dbsr_psnr_from_stats: stats [B,2] float64 (objective_step / objective_forward) -> (psnr [1] = the mean over
    the images whose PSNR is finite, 0 if none; per_image [B]).  max_values: per-image maxima [B] (device) instead
    of the scalar max_value."""
    _need_cuda(stats)
    if stats.dtype != torch.float64 or stats.dim() != 2 or stats.shape[1] != 2 or not stats.is_contiguous():
        raise ValueError('psnr_from_stats: stats must be a contiguous float64 [B, 2] tensor')
    B = stats.shape[0]
    dev = stats.device
    if max_values is not None:
        _need_cuda(max_values)
        max_values = _f32c(max_values).reshape(-1)
        if max_values.numel() != B:
            raise ValueError('psnr_from_stats: max_values must hold B values')
    out = torch.zeros(1, dtype=torch.float32, device=dev)
    per = torch.zeros(B, dtype=torch.float32, device=dev)
    L.check(L.lib().dbsr_psnr_from_stats(B, stats.data_ptr(), int(bool(masked)),
                                         float(max_value if max_value is not None else 0.0), _ptr(max_values),
                                         out.data_ptr(), per.data_ptr(), L.stream_ptr(dev)), 'dbsr_psnr_from_stats')
    return out, per


def relu_grad_scaled(pred, gout, state, dpre):
    """dbsr_relu_grad_scaled: dpre [B,H,W,ld >= C] = state.scale * [pred > 0] * gout (pred / gout fp32 NCHW).
    Returns dpre."""
    _ls_check(state, pred, gout, dpre)
    B, C, H, W = pred.shape
    pred, gout = _f32c(pred), _f32c(gout)
    L.check(L.lib().dbsr_relu_grad_scaled(B, C, H, W, pred.data_ptr(), gout.data_ptr(), state.data_ptr(),
                                          L.tensor_desc(dpre, dpre.shape[-1]), L.stream_ptr(pred.device)),
            'dbsr_relu_grad_scaled')
    return dpre
