"""PWC-Net alignment network (models/alignment/pwcnet.py:234-281), MI355X engine-backed.

`PWCNet(source_img, target_img) -> flow[P,2,H,W]` is the reference's own sub-seam
(pwcnet.py:248); it runs the HIP PWC path of engine.py.  The reference loads
`pwcnet-network-default.pth` with `strKey.replace('module', 'net')` (pwcnet.py:244-246); same here.
"""
import torch
import torch.nn as nn

from .arch import PWCNetwork


class PWCNet(nn.Module):
    def __init__(self, load_pretrained=True, weights_path=None, rgb2bgr=False):
        super().__init__()
        self.net = PWCNetwork()
        self.rgb2bgr = rgb2bgr
        if load_pretrained:
            if weights_path is None:
                raise ValueError('load_pretrained=True needs weights_path (pwcnet.py:240-242)')
            weights_dict = torch.load(weights_path, map_location='cpu', weights_only=True)
            self.net.load_state_dict({k.replace('module', 'net'): v for k, v in weights_dict.items()})
        self.compute_dtype = torch.float32
        # True: in training mode with autograd on and a parameter that requires grad, the forward is a composition
        # of torch.ops.dbsr.* calls and back-propagates into the parameters (dbsrnet_cvpr2021(train_alignmentnet=
        # True) sets it).  False (default): always the engine, forward-only.
        self.differentiable = False
        self._engine = None

    def _trains(self):
        return (self.differentiable and self.training and torch.is_grad_enabled()
                and any(p.requires_grad for p in self.parameters()))

    def forward(self, source_img, target_img):
        if source_img.shape[-2:] != target_img.shape[-2:]:
            raise ValueError('source/target spatial sizes differ (pwcnet.py:249-250)')
        if self._trains():
            return self._forward_autograd(source_img, target_img)
        from .engine import PWCEngine
        if self._engine is None or not self._engine.matches(self):
            self._engine = PWCEngine(self)
        return self._engine.forward(source_img, target_img)

    # ------------------------------------------------------------------------------------------------
    # The differentiable forward: PWCNet.forward / Network.forward (pwcnet.py:221-281) as torch.ops.dbsr.* calls,
    # each with a HIP backward (csrc/pwc_grad.hip, flow_grad.hip, train_ops.hip).  The DenseNet concatenations and
    # the final flow + refiner add are torch ops (autograd slices the concat's gradient); accumulating the dense
    # convs' input gradients in place into channel slices of one buffer is later work.
    # ------------------------------------------------------------------------------------------------
    _BACKWARP = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}          # fltBackwarp, pwcnet.py:121

    def _forward_autograd(self, source_img, target_img):
        if self.compute_dtype != torch.float32:
            raise NotImplementedError('PWCNet(differentiable=True) trains in float32 only (flows are fp32 everywhere '
                                      'in this package); compute_dtype is %s' % self.compute_dtype)
        from . import _lib
        from .torch_ops import load
        ops = load()
        LRELU = _lib.ACT_LRELU
        H, W = source_img.shape[-2:]
        src = source_img.reshape(-1, 3, H, W).float()
        tgt = target_img.reshape(-1, 3, H, W).float()
        if self.rgb2bgr:
            src, tgt = src[:, [2, 1, 0]], tgt[:, [2, 1, 0]]
        P = src.shape[0]
        Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
        # the images are data: the resize is forward-only.  flow = net(target, source) (pwcnet.py:273); both pyramids
        # in one batch (the convs are per-image, the parameter gradients add up the same way)
        x = ops.resize_bilinear(torch.cat([tgt, src], 0).detach().contiguous(), Hp, Wp)

        def conv(seq, i, t, stride=1, pad=1, dil=1, act=LRELU):
            m = seq[i]
            return ops.conv2d_fused(t, m.weight, m.bias, stride, pad, dil, act, None, 0)

        net = self.net
        feats = []
        for name in ['netOne', 'netTwo', 'netThr', 'netFou', 'netFiv', 'netSix']:
            seq = getattr(net.netExtractor, name)
            x = conv(seq, 4, conv(seq, 2, conv(seq, 0, x, stride=2)))
            feats.append(x)
        est = None
        for level, name in [(6, 'netSix'), (5, 'netFiv'), (4, 'netFou'), (3, 'netThr'), (2, 'netTwo')]:
            dec = getattr(net, name)
            first, second = feats[level - 1][:P].contiguous(), feats[level - 1][P:].contiguous()
            if est is None:
                feat = ops.correlation(first, second, True)
            else:
                flow = ops.conv_transpose2d_k4s2(est[0], dec.netUpflow.weight, dec.netUpflow.bias)
                upfeat = ops.conv_transpose2d_k4s2(est[1], dec.netUpfeat.weight, dec.netUpfeat.bias)
                warped = ops.backwarp(second, flow * self._BACKWARP[level])
                feat = torch.cat([ops.correlation(first, warped, True), first, flow, upfeat], 1)
            for sub in ['netOne', 'netTwo', 'netThr', 'netFou', 'netFiv']:
                feat = torch.cat([conv(getattr(dec, sub), 0, feat), feat], 1)
            est = (conv(dec.netSix, 0, feat, act=_lib.ACT_NONE), feat)
        r = est[1]
        main = net.netRefiner.netMain
        for i, d in enumerate([1, 2, 4, 8, 16, 1, 1]):
            r = conv(main, 2 * i, r, pad=d, dil=d, act=LRELU if i < 6 else _lib.ACT_NONE)
        return ops.flow_finalize((est[0] + r).contiguous(), H, W, Hp, Wp)
