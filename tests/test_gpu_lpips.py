"""LPIPS on the HIP device (csrc/lpips.hip and the fp32 dbsr_conv2d, through ops.lpips_prep / maxpool2d /
lpips_layer / LPIPSPlan and evaluation.LPIPS) against values computed on the CPU.  No torch convolution runs on the
device here: every expected value comes from the host.

Bounds, none of them taken from the code under test:
  * prep and max-pool are bitwise: an IEEE subtraction and division, and a maximum.
  * a backbone conv is within 4e-7 * sum |a||b| of its float64 value: the measured bound of the K-ordered fp32 MFMA
    chain up to K = 4096 (3.5e-7), rounded up.
  * the layer kernel and the whole metric get 4x the float32 CPU restatement's own distance-map error against
    float64 on the same inputs (tests/golden/lpips.npz at the fixture shapes): the kernels' sequential fp32 sums
    lose up to about 3x what a blocked CPU sum does (3.5e-7 against ~1e-7 of sum |ab|).  A value is within
    max(4x its float32 error, 4 float32 ulps): five fp32 per-layer roundings and the final store.

Measured on MI355X (kernel error / yardstick; DESIGN.md, 'LPIPS'): convs 0.11 to 0.27 of their bound; the layer
kernel alone 0.15 to 1.53 on maps and at most 1.03 on per-layer values (bar 4); end to end, maps of layers 0..4:
alex 35x47 0.39 0.39 0.28 1.30 1.42, 51x39 0.60 0.80 1.46 1.52 0.40, 384 1.14 1.31 1.23 1.53 1.24; vgg 35x47 1.42
1.59 1.33 0.89 0.72, 51x39 1.30 1.17 1.44 1.80 3.21, 384 1.51 1.27 1.31 1.08 1.18 (bar 4); values within 2.7e-10
(bar 4.7e-10 to 9.3e-10).  With the convs' K summed in one chain instead of blocks of 32 channels, vgg's deepest
map reached 5.76 at 384 and 4.56 at 51x39 (a four-pixel map whose yardstick is 6.5 ulps where others have 20 to 26):
that is why LPIPSPlan blocks K."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips.npz')
WEIGHT_SEED = 11                                        # make_golden_lpips.WEIGHT_SEED
CASES = {'a': ((1, 3, 35, 47), 0, 101), 'b': ((2, 3, 51, 39), 4, 102)}     # make_golden_lpips.CASES


def images(shape, seed):
    """make_golden_lpips.images: gt = rand, pred = clamp(gt + 0.25 randn, 0, 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = rng.random(shape, dtype=np.float64).astype(np.float32)
    pred = np.clip(gt + np.float32(0.25) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(gt)


def ulp32(v):
    return float(np.spacing(np.float32(abs(float(v)))))


@pytest.fixture(scope='module')
def ops():
    from dbsr_amd import ops
    return ops


@pytest.fixture(scope='module')
def ev():
    from dbsr_amd import evaluation
    return evaluation


@functools.lru_cache(maxsize=None)
def _weights(net):
    from dbsr_amd import evaluation
    sd = evaluation.generate_lpips_state_dict(net, seed=WEIGHT_SEED)
    return sd, evaluation.load_lpips_weights(sd, net)


@functools.lru_cache(maxsize=None)
def _plan(net):
    from dbsr_amd import ops
    w = _weights(net)[1]
    return ops.LPIPSPlan({'net': net, 'conv_w': [t.to(DEV) for t in w['conv_w']],
                          'conv_b': [t.to(DEV) for t in w['conv_b']], 'lin': [t.to(DEV) for t in w['lin']]})


# ---------------------------------------------------------------------------------------------------- prep
@pytest.mark.parametrize('bi', [0, 4])
@pytest.mark.parametrize('flip,normalize', [(False, False), (True, False), (False, True), (True, True)])
def test_prep_bitwise(ops, ev, bi, flip, normalize):
    pred, gt = images((2, 3, 41, 47), 20 + bi)
    out = ops.lpips_prep(pred.to(DEV), gt.to(DEV), bi, 'alex', flip, normalize).cpu()
    assert out.shape == (4, 41 - 2 * bi, 47 - 2 * bi, 8)
    p, g = ev.lpips_prepare(pred, gt, bi, flip)
    x = torch.cat([p, g], 0)
    if normalize:
        x = 2 * x - 1
    want = (x - torch.tensor(ev.LPIPS_SHIFT).view(1, 3, 1, 1)) / torch.tensor(ev.LPIPS_SCALE).view(1, 3, 1, 1)
    assert torch.equal(out[..., :3], want.permute(0, 2, 3, 1))
    assert torch.equal(out[..., 3:], torch.zeros(4, 41 - 2 * bi, 47 - 2 * bi, 5))


# ------------------------------------------------------------------------------------------------- maxpool
@pytest.mark.parametrize('shape,k,s', [((2, 8, 11, 64), 3, 2), ((1, 3, 5, 192), 3, 2), ((1, 7, 9, 128), 2, 2),
                                       ((1, 3, 3, 256), 3, 2)])
def test_maxpool_bitwise(ops, shape, k, s):
    x = torch.randn(shape, generator=torch.Generator().manual_seed(shape[1] * 100 + shape[2]))
    y = ops.maxpool2d(x.to(DEV), k, s).cpu()
    want = F.max_pool2d(x.permute(0, 3, 1, 2), k, s).permute(0, 2, 3, 1)
    assert y.shape == want.shape == (shape[0], (shape[1] - k) // s + 1, (shape[2] - k) // s + 1, shape[3])
    assert torch.equal(y, want)


# ------------------------------------------------------------------------------------------ backbone convs
@pytest.mark.parametrize('cin,cout,k,s,p,n,h,w', [
    (3, 64, 11, 4, 2, 2, 35, 47), (64, 192, 5, 1, 2, 2, 3, 5),
    (192, 384, 3, 1, 1, 2, 2, 2), (192, 384, 3, 1, 1, 1, 1, 1),
    (512, 512, 3, 1, 1, 2, 2, 2), (512, 512, 3, 1, 1, 1, 1, 1)])
def test_backbone_conv_vs_float64(ops, cin, cout, k, s, p, n, h, w):
    """dbsr_conv2d in fp32 with ReLU at the backbone's shapes, within 4e-7 * (|w| conv |x| + |b|) of float64."""
    from dbsr_amd import _lib as L
    gen = torch.Generator().manual_seed(cin + cout + h)
    x = torch.randn(n, cin, h, w, generator=gen)
    wt = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    b = 0.1 * torch.randn(cout, generator=gen)
    y = ops.conv2d(x.to(DEV), wt.to(DEV), b.to(DEV), stride=s, padding=p, act=L.ACT_RELU).cpu().double()
    want = F.relu(F.conv2d(x.double(), wt.double(), b.double(), stride=s, padding=p))
    bound = 4e-7 * (F.conv2d(x.double().abs(), wt.double().abs(), b.double().abs(), stride=s, padding=p))
    assert y.shape == want.shape
    ratio = float(((y - want).abs() / bound).max())
    print('conv %d->%d k%d s%d on %dx%dx%d: kernel %d, max err / bound %.3f'
          % (cin, cout, k, s, n, h, w, ops.conv2d.last_kernel, ratio))
    assert ratio <= 1.0


# --------------------------------------------------------------------------------------- the layer kernel
@functools.lru_cache(maxsize=None)
def _layer_case(C, h, w, B):
    """Post-ReLU-like features of two nearby images with the edge pixels planted, their float64 map and the float32
    CPU restatement's error against it.  The seed is the first at which that error exceeds one float32 ulp of the
    map's maximum: below that the yardstick would be finer than the format the kernel stores."""
    from dbsr_amd import evaluation
    for seed in range(32):
        gen = torch.Generator().manual_seed(100000 * C + 1000 * h + 10 * w + B + 7919 * seed)
        n0 = torch.randn(B, h, w, C, generator=gen).clamp(min=0)                   # NHWC storage
        n1 = (n0 + 0.3 * torch.randn(B, h, w, C, generator=gen)).clamp(min=0)
        lin = 2.0 * torch.rand(C, generator=gen) / C
        flat0, flat1 = n0.view(-1, C), n1.view(-1, C)
        f0, f1 = n0.permute(0, 3, 1, 2), n1.permute(0, 3, 1, 2)                      # NCHW views of the same
        n = flat0.shape[0]
        flat0[0] = 0                                           # all zero in one image
        if n > 1:
            flat0[1] = 0
            flat1[1] = 0                                       # all zero in both
        if n > 2:
            flat0[2] *= 1e-6 / flat0[2].norm()                 # norm ~1e-6
        m64 = evaluation.lpips_layer_map(f0.double(), f1.double(), lin.double())
        m32 = evaluation.lpips_layer_map(f0, f1, lin)
        err = float((m32.double() - m64).abs().max())
        if err > ulp32(m64.max()):
            return f0, f1, lin, m64, err
    raise AssertionError('no seed gives a usable yardstick')


@pytest.mark.parametrize('C', [64, 128, 192, 256, 384, 512])
@pytest.mark.parametrize('h,w', [(1, 1), (3, 5), (18, 11), (37, 37)])
@pytest.mark.parametrize('B', [1, 3])
def test_layer_kernel_vs_float64(ops, C, h, w, B):
    f0, f1, lin, m64, err32 = _layer_case(C, h, w, B)
    feat = torch.cat([f0, f1], 0).permute(0, 2, 3, 1).contiguous().to(DEV)
    value, per_layer, dmap = ops.lpips_layer(feat, lin.to(DEV), layer=0, want_map=True)
    dmap, per_layer, value = dmap.double().cpu(), per_layer.double().cpu(), value.double().cpu()
    e_map = float((dmap - m64).abs().max())
    e_val = float((per_layer[:, 0] - m64.mean(dim=(1, 2))).abs().max())
    print('C %d %dx%d B %d: map err %.3e, value err %.3e, fp32 restatement %.3e -> ratios %.2f %.2f'
          % (C, h, w, B, e_map, e_val, err32, e_map / err32, e_val / err32))
    assert torch.isfinite(dmap).all()
    flat = dmap.reshape(-1)
    if flat.numel() > 1:
        assert float(flat[1]) == 0.0                          # both vectors zero: exactly 0
    assert e_map <= 4 * err32
    assert e_val <= 4 * err32
    assert torch.equal(value, per_layer[:, 0]) and float(per_layer[:, 1:].abs().max()) == 0.0
    # layer > 0 adds into value and keeps the other columns
    v2, pl2, none = ops.lpips_layer(feat, lin.to(DEV), layer=3, per_layer=per_layer.float().to(DEV),
                                    value=value.float().to(DEV))
    assert none is None
    assert torch.equal(pl2[:, 3].cpu(), pl2[:, 0].cpu())
    assert torch.equal(v2.cpu(), (pl2[:, 0] + pl2[:, 3]).cpu())


def test_layer_kernel_bitwise_and_batch_independent(ops):
    f0, f1, lin, _, _ = _layer_case(384, 18, 11, 3)
    feat = torch.cat([f0, f1], 0).permute(0, 2, 3, 1).contiguous().to(DEV)
    a = ops.lpips_layer(feat, lin.to(DEV), want_map=True)
    b = ops.lpips_layer(feat, lin.to(DEV), want_map=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    for i in range(3):
        one = ops.lpips_layer(feat[[i, 3 + i]].contiguous(), lin.to(DEV), want_map=True)
        assert torch.equal(one[0][0], a[0][i]) and torch.equal(one[2][0], a[2][i])


# ---------------------------------------------------------------------------------------------- end to end
@functools.lru_cache(maxsize=None)
def _scoring_case(net):
    """The scoring shape 1 x 3 x 384 x 384, boundary_ignore 40: the restatement on the CPU in float64, and the float32
    restatement's errors against it."""
    from dbsr_amd import evaluation
    pred, gt = images((1, 3, 384, 384), 103)
    w = _weights(net)[1]
    p, g = evaluation.lpips_prepare(pred, gt, 40)
    v64, _, m64 = evaluation.lpips_value(p.double(), g.double(), w)
    v32, _, m32 = evaluation.lpips_value(p, g, w)
    err_map = [float((a.double() - b).abs().max()) for a, b in zip(m32, m64)]
    return pred, gt, v64.numpy(), [m.numpy() for m in m64], err_map, np.abs(v32.double().numpy() - v64.numpy())


def _check_end_to_end(net, pred, gt, bi, v64, m64, err_map, err_value, tag):
    value, per_layer, maps = _plan(net).forward(pred.to(DEV), gt.to(DEV), bi, want_maps=True)
    value, maps = value.double().cpu().numpy(), [m.double().cpu().numpy() for m in maps]
    for l in range(5):
        assert maps[l].shape == m64[l].shape
        e = float(np.abs(maps[l] - m64[l]).max())
        print('%s %s layer %d: map err %.3e, fp32 restatement %.3e, ratio %.2f' % (net, tag, l, e, err_map[l],
                                                                                e / err_map[l]))
    for b in range(len(v64)):
        print('%s %s image %d: value %.9g, err %.3e, fp32 restatement %.3e, ulp %.3e'
              % (net, tag, b, v64[b], abs(value[b] - v64[b]), err_value[b], ulp32(v64[b])))
    for l in range(5):
        assert float(np.abs(maps[l] - m64[l]).max()) <= 4 * err_map[l], l
    for b in range(len(v64)):
        assert abs(value[b] - v64[b]) <= max(4 * err_value[b], 4 * ulp32(v64[b])), b


@pytest.mark.parametrize('net', ['alex', 'vgg'])
@pytest.mark.parametrize('case', ['a', 'b'])
def test_end_to_end_vs_fixture(net, case):
    golden = np.load(GOLDEN)
    shape, bi, seed = CASES[case]
    pred, gt = images(shape, seed)
    pre = '%s_%s_' % (net, case)
    _check_end_to_end(net, pred, gt, bi, golden[pre + 'value'], [golden[pre + 'map%d' % l] for l in range(5)],
                      golden[pre + 'err32_map'], golden[pre + 'err32_value'], case)


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_end_to_end_scoring_shape(net):
    pred, gt, v64, m64, err_map, err_value = _scoring_case(net)
    _check_end_to_end(net, pred, gt, 40, v64, m64, err_map, err_value, '384')


# ---------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_runs_are_bitwise_equal_and_batch_independent(net):
    pred, gt = images((3, 3, 51, 39), 104)
    plan = _plan(net)
    first = [t.clone() if torch.is_tensor(t) else [m.clone() for m in t]
             for t in plan.forward(pred.to(DEV), gt.to(DEV), 4, want_maps=True)]
    again = plan.forward(pred.to(DEV), gt.to(DEV), 4, want_maps=True)
    assert torch.equal(first[0], again[0]) and torch.equal(first[1], again[1])
    assert all(torch.equal(a, b) for a, b in zip(first[2], again[2]))
    for i in range(3):
        one = plan.forward(pred[i:i + 1].to(DEV), gt[i:i + 1].to(DEV), 4)
        assert torch.equal(one[0][0], first[0][i]) and torch.equal(one[1][0], first[1][i])


def test_module_on_the_device_matches_ops(ev):
    sd = _weights('alex')[0]
    pred, gt = images((2, 3, 51, 39), 105)
    mod = ev.LPIPS(boundary_ignore=4, type='alex', weights=sd, bgr2rgb=True, per_image=True).to(DEV)
    v = mod(pred.to(DEV), gt.to(DEV), valid=torch.zeros(2, 1, 51, 39, device=DEV))
    want = _plan('alex').forward(pred.to(DEV), gt.to(DEV), 4, bgr2rgb=True)[0]
    assert v.shape == (2,) and torch.equal(v, want)
    mean = ev.LPIPS(boundary_ignore=4, type='alex', weights=sd, bgr2rgb=True).to(DEV)
    assert torch.equal(mean(pred.to(DEV), gt.to(DEV)), want.mean())
    assert float(mean(pred[0].to(DEV), gt[0].to(DEV))) == float(want[0])              # 3-dim inputs
    with pytest.raises(ValueError, match='smaller than 31 x 31'):
        mod(pred[..., :38, :].to(DEV), gt[..., :38, :].to(DEV))


def test_device_pred_that_requires_grad_raises(ev):
    mod = ev.LPIPS(type='alex', weights=_weights('alex')[0]).to(DEV)
    pred, gt = images((1, 3, 33, 33), 106)
    p = pred.to(DEV).requires_grad_(True)
    with pytest.raises(RuntimeError, match='forward-only'):
        mod(p, gt.to(DEV))
    with torch.no_grad():
        assert np.isfinite(float(mod(p, gt.to(DEV))))


class _StubNet:
    def __call__(self, burst):
        return F.interpolate(burst[:, 0, :3], scale_factor=8, mode='bilinear', align_corners=False), {}


class _Bursts(torch.utils.data.Dataset):
    def __init__(self, n):
        g = torch.Generator().manual_seed(3)
        self.items = [(torch.rand(2, 4, 6, 6, generator=g), torch.rand(3, 48, 48, generator=g)) for _ in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i][0], self.items[i][1], {'burst_name': '%04d' % i}


def test_scorers_third_column_on_the_device(ev, monkeypatch):
    from dbsr_amd import burstsr
    sd = _weights('alex')[0]
    ds = _Bursts(2)
    lp = ev.LPIPS(boundary_ignore=4, type='alex', weights=sd).to(DEV)
    res = ev.compute_score(_StubNet(), ds, boundary_ignore=4, device=DEV, metrics=('psnr', 'ssim', 'lpips'), lpips=lp)
    base = ev.compute_score(_StubNet(), ds, boundary_ignore=4, device=DEV)
    assert {k: res[k] for k in base} == base
    pred = ev.quantize_prediction(_StubNet()(ds[1][0].unsqueeze(0).to(DEV))[0])
    want = float(_plan('alex').forward(pred, ds[1][1].unsqueeze(0).to(DEV), 4)[0][0])
    assert res['per_image_lpips']['0001'] == want
    assert res['lpips'] == sum(res['per_image_lpips'].values()) / 2

    class _Sca:                                          # the alignment, stubbed: identity and an all-valid mask
        def __init__(self, alignment_net, sr_factor=4):
            pass

        def __call__(self, pred, gt, burst):
            return pred, torch.ones(pred.shape[0], 1, *pred.shape[-2:], dtype=torch.bool, device=pred.device)

    monkeypatch.setattr(burstsr, 'SpatialColorAlignment', _Sca)
    res2 = burstsr.compute_score_burstsr(_StubNet(), ds, None, boundary_ignore=4, device=DEV, lpips=lp)
    assert res2['per_image_lpips'] == res['per_image_lpips'] and res2['lpips'] == res['lpips']
