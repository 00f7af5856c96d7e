"""The HIP backward of LPIPS (csrc/lpips_grad.hip, the fp32 dbsr_conv2d input gradients, ops.LPIPSPlan.backward,
evaluation.LPIPS(differentiable=True)) against values computed on the CPU.  No torch convolution runs on the device
here: every expected value comes from the host.

Bounds, none of them taken from the code under test:
  * the pool backward is within 1 float32 ulp of a host loop with the same tie rule and the same order of addition.
  * the stem backward and the stride-1 input gradients are within 4e-7 * sum |a||b| of their float64 value, the
    forward convs' bound (test_gpu_lpips.py).
  * the layer backward gets 4x the float32 closed form's (evaluation.lpips_layer_grad on the CPU) own error against
    float64, per pixel relative to that pixel's largest gradient (a planted all-zero vector's gradient is 1e10 times
    its neighbours').
  * end to end the reference is the gated float64 backward (evaluation.lpips_backward_reference) with the ReLU masks
    and pool arg-max indices of the device's own saved activations: a pre-activation within rounding of zero may
    gate differently on the device than in float64, and that is not an error of the backward.  The yardstick is the
    same helper in float32 with the same gates; the bar is device error <= 4x yardstick, as max-abs over the
    gradient's maximum.  The plain alex case, whose margins are ten times the forward's error, is also compared with
    the fixture's float64 autograd gradient at 4x the fixture's float32 autograd error.

Measured on MI355X: DESIGN.md, 'LPIPS as a training objective'."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips_grad.npz')
WEIGHT_SEED = 11                                        # make_golden_lpips_grad.WEIGHT_SEED


def images(shape, seed):
    """make_golden_lpips_grad.images: gt = rand, pred = clamp(gt + 0.25 randn, 0, 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = rng.random(shape, dtype=np.float64).astype(np.float32)
    pred = np.clip(gt + np.float32(0.25) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(gt)


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


def _plain_seed():
    return int(np.load(GOLDEN)['plain_seed'])


# ------------------------------------------------------------------------------------------ layer backward
@functools.lru_cache(maxsize=None)
def _layer_case(C, h, w, B=2):
    """test_gpu_lpips._layer_case's features (post-ReLU-like, two nearby images, planted all-zero and 1e-6-norm
    vectors), a non-uniform gvalue, the float64 closed form and the float32 closed form's error per pixel."""
    from dbsr_amd import evaluation
    gen = torch.Generator().manual_seed(100000 * C + 1000 * h + 10 * w + B)
    n0 = torch.randn(B, h, w, C, generator=gen).clamp(min=0)                       # NHWC storage
    n1 = (n0 + 0.3 * torch.randn(B, h, w, C, generator=gen)).clamp(min=0)
    lin = 2.0 * torch.rand(C, generator=gen) / C
    flat0, flat1 = n0.view(-1, C), n1.view(-1, C)
    n = flat0.shape[0]
    flat0[0] = 0                                               # all zero in pred only: the limit I / eps
    if n > 1:
        flat0[1] = 0
        flat1[1] = 0                                           # all zero in both: exactly 0
    if n > 2:
        flat0[2] *= 1e-6 / flat0[2].norm()                     # norm ~1e-6
    gv = torch.tensor([0.75, -1.5, 2.25, 0.3][:B])
    f0, f1 = n0.permute(0, 3, 1, 2), n1.permute(0, 3, 1, 2)
    gmap = lambda dt: (gv.to(dt) / (h * w)).view(B, 1, 1).expand(B, h, w)
    g64 = evaluation.lpips_layer_grad(f0.double(), f1.double(), lin.double(), gmap(torch.float64))
    g32 = evaluation.lpips_layer_grad(f0, f1, lin, gmap(torch.float32))
    return n0, n1, lin, gv, g64.permute(0, 2, 3, 1).contiguous(), g32.permute(0, 2, 3, 1).contiguous()


def _pixel_error(g, g64):
    """max over pixels of max_c |g - g64| / max_c |g64| (pixels whose float64 gradient is all zero must be exactly
    zero and are left out)."""
    scale = g64.abs().amax(dim=-1)
    live = scale > 0
    assert float(g.double()[~live].abs().max()) == 0.0 if (~live).any() else True
    return float(((g.double() - g64).abs().amax(dim=-1)[live] / scale[live]).max())


@pytest.mark.parametrize('C', [64, 192, 256, 512])
@pytest.mark.parametrize('h,w', [(1, 1), (3, 5), (7, 9)])
def test_layer_backward_vs_float64(ops, C, h, w):
    n0, n1, lin, gv, g64, g32 = _layer_case(C, h, w)
    feat = torch.cat([n0, n1], 0).contiguous().to(DEV)
    got = ops.lpips_layer_backward(feat, lin.to(DEV), gv.to(DEV))
    again = ops.lpips_layer_backward(feat, lin.to(DEV), gv.to(DEV))
    assert torch.equal(got, again)                                             # two runs are bitwise equal
    assert got.shape == g64.shape and torch.isfinite(got).all()
    err, yard = _pixel_error(got.cpu(), g64), _pixel_error(g32, g64)
    print('C %d %dx%d: layer backward err %.3e, fp32 closed form %.3e, ratio %.2f, |zero-vector grad| %.3g'
          % (C, h, w, err, yard, err / yard, float(g64[0, 0, 0].abs().max())))
    assert err <= 4 * yard
    # accumulate adds the same values to what the buffer held; without it a NaN-filled buffer is overwritten
    base = torch.randn(g64.shape, generator=torch.Generator().manual_seed(C + h)).to(DEV)
    acc = ops.lpips_layer_backward(feat, lin.to(DEV), gv.to(DEV), out=base.clone(), accumulate=True)
    assert torch.equal(acc, base + got)
    over = ops.lpips_layer_backward(feat, lin.to(DEV), gv.to(DEV), out=torch.full_like(base, float('nan')))
    assert torch.equal(over, got)
    # an image's gradient does not depend on its batch
    one = ops.lpips_layer_backward(feat[[1, 3]].contiguous(), lin.to(DEV), gv[1:2].to(DEV))
    assert torch.equal(one[0], got[1])


# ------------------------------------------------------------------------------------------- pool backward
def _pool_backward_host(x, dy, k, s):
    """float32 numpy: windows in (oy, ox) order, each adding its dy at its first maximum (np.argmax)."""
    N, H, W, C = x.shape
    dx = np.zeros_like(x)
    for oy in range(dy.shape[1]):
        for ox in range(dy.shape[2]):
            win = x[:, oy * s:oy * s + k, ox * s:ox * s + k, :].reshape(N, k * k, C)
            idx = win.argmax(axis=1)
            for e in range(k * k):
                dx[:, oy * s + e // k, ox * s + e % k, :] += np.where(idx == e, dy[:, oy, ox, :], np.float32(0))
    return dx


@pytest.mark.parametrize('H,W,k,s', [(7, 7, 3, 2), (8, 8, 3, 2), (5, 4, 2, 2)])
@pytest.mark.parametrize('C', [64, 192])
def test_pool_backward_vs_host(ops, H, W, k, s, C):
    gen = torch.Generator().manual_seed(H * 100 + W * 10 + C)
    x = (torch.randn(2, H, W, C, generator=gen) * 2).round() / 2           # steps of 0.5: ties in most windows
    x[0, 0, 0] = x[0, 0, 1] = 7.0                                          # a planted tie: the first element wins
    x[1, 2, 2] = 9.0                                                       # the maximum of overlapping windows
    oh, ow = (H - k) // s + 1, (W - k) // s + 1
    dy = torch.randn(2, oh, ow, C, generator=gen)
    want = _pool_backward_host(x.numpy(), dy.numpy(), k, s)
    idx = F.max_pool2d(x.permute(0, 3, 1, 2), k, s, return_indices=True)[1]                # torch's tie rule
    tw = torch.zeros(2, C, H * W).scatter_add_(2, idx.flatten(2), dy.permute(0, 3, 1, 2).flatten(2))
    assert np.abs(tw.view(2, C, H, W).permute(0, 2, 3, 1).numpy() - want).max() <= 1e-6
    out = torch.full((2, H, W, C), float('nan'), device=DEV)
    got = ops.maxpool2d_backward(x.to(DEV), dy.to(DEV), k, s, out=out).cpu().numpy()
    assert np.isfinite(got).all()
    assert (np.abs(got - want) <= np.spacing(np.abs(want))).all()
    assert (got[0, 0, 1] == 0).all() and (got[0, 0, 0] == want[0, 0, 0]).all() and (want[0, 0, 0] != 0).all()
    if k == 3:
        assert (got[1, 2, 2] == want[1, 2, 2]).all()
        assert np.allclose(want[1, 2, 2], dy[1, :2, :2].sum(dim=(0, 1)).numpy(), atol=1e-5)
    if (H - k) % s:
        assert (got[:, (oh - 1) * s + k:] == 0).all()                      # rows floor mode drops
    if (W - k) % s:
        assert (got[:, :, (ow - 1) * s + k:] == 0).all()


# ------------------------------------------------------------------------------------------- stem backward
@pytest.mark.parametrize('net,Hc,Wc,bi,flip,normalize', [
    ('alex', 31, 31, 0, False, False), ('alex', 31, 33, 4, True, False), ('alex', 33, 34, 0, False, True),
    ('alex', 31, 34, 4, True, True), ('vgg', 16, 16, 0, False, False), ('vgg', 16, 16, 4, True, True)])
def test_stem_backward_vs_float64(ops, ev, net, Hc, Wc, bi, flip, normalize):
    """alex at widths 31, 33, 34: (W + 2 pad - k) % stride = 0, 2, 3 trailing columns of the padded input reach no
    output; the first `pad` of them are the padding itself, so a real column is left out (and gets zero) only at
    34."""
    cin, cout, k, s, p = ev.LPIPS_NETS[net]['convs'][0]
    B, H, W = 2, Hc + 2 * bi, Wc + 2 * bi
    oh, ow = (Hc + 2 * p - k) // s + 1, (Wc + 2 * p - k) // s + 1
    gen = torch.Generator().manual_seed(Hc * 100 + Wc + bi)
    dy = torch.randn(B, oh, ow, cout, generator=gen)
    w = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cin * k * k)) ** 0.5
    out = torch.full((B, 3, H, W), float('nan'), device=DEV)
    got = ops.lpips_stem_backward(dy.to(DEV), w.to(DEV), (B, 3, H, W), bi, net, flip, normalize, out=out).cpu().double()
    assert torch.isfinite(got).all()

    def transpose(a, b):                                       # the conv's transpose, out to the crop's size
        extra = (Hc - ((oh - 1) * s - 2 * p + k), Wc - ((ow - 1) * s - 2 * p + k))
        t = F.conv_transpose2d(a.permute(0, 3, 1, 2).double(), b.double(), stride=s, padding=p, output_padding=extra)
        assert t.shape[2:] == (Hc, Wc)
        return t

    mul = (2.0 if normalize else 1.0) / torch.tensor(ev.LPIPS_SCALE, dtype=torch.float32).double().view(1, 3, 1, 1)
    want, bound = transpose(dy, w) * mul, 4e-7 * transpose(dy.abs(), w.abs()) * mul
    if flip:
        want, bound = want[:, [2, 1, 0]], bound[:, [2, 1, 0]]
    want, bound = F.pad(want, (bi,) * 4), F.pad(bound, (bi,) * 4)
    err = (got - want).abs()
    print('%s stem %dx%d bi %d: max err / bound %.3f' % (net, Hc, Wc, bi, float((err / bound)[bound > 0].max())))
    assert (err <= bound).all()
    assert float(got[bound == 0].abs().max()) == 0.0 if (bound == 0).any() else True
    dropped = max(0, (Wc + 2 * p - k) % s - p)
    assert dropped == (1 if (net, Wc) == ('alex', 34) else 0)
    if dropped:
        assert float(bound[..., bi:H - bi, W - bi - dropped:W - bi].max()) == 0.0
        assert float(got[..., W - bi - dropped:].abs().max()) == 0.0


# ------------------------------------------------------------------------------- stride-1 input gradients
@pytest.mark.parametrize('cin,cout,k,p,h,w', [(64, 192, 5, 2, 3, 3), (512, 512, 3, 1, 1, 1), (512, 512, 3, 1, 2, 2),
                                              (64, 64, 3, 1, 33, 33)])
def test_conv_dgrad_vs_float64(ops, cin, cout, k, p, h, w):
    """The input gradient of a cin -> cout conv as the plan launches it: per image, K = cout in blocks of 32."""
    gen = torch.Generator().manual_seed(cin + cout + h)
    dy = torch.randn(2, h, w, cout, generator=gen)
    wt = torch.randn(cout, cin, k, k, generator=gen) * (2.0 / (cout * k * k)) ** 0.5
    got = ops.lpips_conv_dgrad(dy.to(DEV), wt.to(DEV), p).cpu().double().permute(0, 3, 1, 2)
    want = F.conv_transpose2d(dy.permute(0, 3, 1, 2).double(), wt.double(), padding=p)
    bound = 4e-7 * F.conv_transpose2d(dy.permute(0, 3, 1, 2).double().abs(), wt.double().abs(), padding=p)
    assert got.shape == want.shape == (2, cin, h, w)
    ratio = float(((got - want).abs() / bound).max())
    print('dgrad %d<-%d k%d on %dx%d: max err / bound %.3f' % (cin, cout, k, h, w, ratio))
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------- end to end
def _device_gates(plan, B):
    """The ReLU masks and arg-max indices of the plan's saved activations (pred half), computed on the host."""
    pools = [op for op in plan.spec['program'] if isinstance(op, tuple)]
    masks, argmax = [], []
    for act in plan.activations():
        if act[0] == 'relu':
            masks.append((act[1][:B] > 0).permute(0, 3, 1, 2).cpu())
        else:
            _, k, s = pools[len(argmax)]
            x = act[1][:B].permute(0, 3, 1, 2).cpu().contiguous()
            y, idx = F.max_pool2d(x, k, s, return_indices=True)
            assert torch.equal(y, act[2][:B].permute(0, 3, 1, 2).cpu())
            argmax.append(idx)
    return masks, argmax


def _gated_check(net, shape, bi, seed, flip=False, normalize=False, gv=None):
    from dbsr_amd import evaluation as evm
    pred, gt = images(shape, seed)
    B = shape[0]
    plan, w = _plan(net), _weights(net)[1]
    value = plan.forward(pred.to(DEV), gt.to(DEV), bi, flip, normalize)[0].cpu()
    got = plan.backward(None if gv is None else gv.to(DEV)).cpu().double()
    masks, argmax = _device_gates(plan, B)
    p, g = evm.lpips_prepare(pred, gt, bi, flip)
    v64, r64 = evm.lpips_backward_reference(p.double(), g.double(), w, masks, argmax, normalize,
                                            None if gv is None else gv.double())
    _, r32 = evm.lpips_backward_reference(p, g, w, masks, argmax, normalize, gv)
    own = evm.lpips_gates(p.double(), w, normalize)
    flips = sum(int((a != b).sum()) for a, b in zip(masks + argmax, own[0] + own[1]))
    H, W = shape[2:]
    crop = got[..., bi:H - bi, bi:W - bi]
    if flip:
        crop = crop[:, [2, 1, 0]]
    frame = got.clone()
    frame[..., bi:H - bi, bi:W - bi] = 0
    assert float(frame.abs().max()) == 0.0
    top = float(r64.abs().max())
    err, yard = float((crop - r64).abs().max()) / top, float((r32.double() - r64).abs().max()) / top
    print('%s %s bi %d: value %s, max |grad| %.3g, device err %.3e, fp32 gated reference %.3e, ratio %.2f, '
          'gates that differ from float64: %d' % (net, shape, bi, value.tolist(), top, err, yard, err / yard, flips))
    assert torch.isfinite(got).all() and top > 0
    assert err <= 4 * yard
    return got


@pytest.mark.parametrize('net', ['alex', 'vgg'])
@pytest.mark.parametrize('case', ['plain', 'b', 'min'])
def test_end_to_end_vs_gated_reference(net, case):
    """1x3x41x41 (alex's taps 2..4 are 1 x 1 maps), 2x3x51x39, and the smallest crops."""
    if case == 'plain':
        _gated_check(net, (1, 3, 41, 41), 4, _plain_seed())
    elif case == 'b':
        _gated_check(net, (2, 3, 51, 39), 4, 102)
    else:
        side = 31 if net == 'alex' else 16
        _gated_check(net, (1, 3, side, side), 0, 107)


def test_end_to_end_flags_and_gvalue():
    _gated_check('alex', (2, 3, 45, 43), 4, 108, flip=True, normalize=True, gv=torch.tensor([0.75, -1.5]))


def test_plain_alex_vs_fixture_autograd():
    golden = np.load(GOLDEN)
    assert float(golden['alex_plain_relu_margin']) >= 1e-5 and float(golden['alex_plain_pool_margin']) >= 1e-5
    pred, gt = images((1, 3, 41, 41), _plain_seed())
    plan = _plan('alex')
    plan.forward(pred.to(DEV), gt.to(DEV), 4)
    got = plan.backward().cpu().double().numpy()
    want, yard = golden['alex_plain_grad'], float(golden['alex_plain_err32'])
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print('alex plain vs float64 autograd: err %.3e, fp32 autograd %.3e, ratio %.2f' % (err, yard, err / yard))
    assert err <= 4 * yard


# ---------------------------------------------------------------------------------------------- properties
@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_backward_is_bitwise_reproducible_batch_independent_and_linear(net):
    pred, gt = images((3, 3, 51, 39), 104)
    plan = _plan(net)
    p, g = pred.to(DEV), gt.to(DEV)
    plan.forward(p, g, 4)
    first = plan.backward().clone()
    assert torch.equal(plan.backward(), first)                                 # two runs are bitwise equal
    plan.forward(p, g, 4)
    assert torch.equal(plan.backward(), first)
    # gvalue scales each image's gradient: powers of two exactly, zero gives zero
    scaled = plan.backward(torch.tensor([2.0, -0.5, 0.0], device=DEV)).clone()
    assert torch.equal(scaled[0], 2 * first[0]) and torch.equal(scaled[1], -0.5 * first[1])
    assert float(scaled[2].abs().max()) == 0.0
    # and any factor up to the rounding of a handful of fp32 operations per term (1e-5 of the maximum is ~100
    # ulps: the factor enters once, at the layer kernels)
    tripled = plan.backward(torch.full((3,), 3.0, device=DEV))
    assert float((tripled - 3 * first).abs().max()) <= 1e-5 * float(first.abs().max())
    for i in range(3):
        plan.forward(p[i:i + 1], g[i:i + 1], 4)
        assert torch.equal(plan.backward()[0], first[i])                      # bitwise the B = 1 gradient


def test_backward_needs_a_forward_and_its_newest_one():
    from dbsr_amd import ops
    w = _weights('alex')[1]
    plan = ops.LPIPSPlan({'net': 'alex', 'conv_w': [t.to(DEV) for t in w['conv_w']],
                          'conv_b': [t.to(DEV) for t in w['conv_b']], 'lin': [t.to(DEV) for t in w['lin']]})
    with pytest.raises(RuntimeError, match='no forward'):
        plan.backward()
    pred, gt = images((1, 3, 33, 35), 109)
    plan.forward(pred.to(DEV), gt.to(DEV))
    token = plan.token()
    plan.backward(token=token)
    plan.forward(pred.to(DEV), gt.to(DEV))
    with pytest.raises(RuntimeError, match='another forward of the same shape'):
        plan.backward(token=token)
    plan.backward(token=plan.token())
    with pytest.raises(ValueError, match='gvalue'):
        plan.backward(torch.ones(2, device=DEV))


# -------------------------------------------------------------------------------------------------- module
def test_module_gradient_is_the_plans(ev):
    sd = _weights('alex')[0]
    pred, gt = images((2, 3, 51, 39), 105)
    kw = dict(boundary_ignore=4, type='alex', weights=sd, bgr2rgb=True)
    plain = ev.LPIPS(**kw).to(DEV)
    mean = ev.LPIPS(differentiable=True, **kw).to(DEV)
    per = ev.LPIPS(differentiable=True, per_image=True, **kw).to(DEV)
    plan = _plan('alex')

    def plan_grad(gv):
        plan.forward(pred.to(DEV), gt.to(DEV), 4, bgr2rgb=True)
        return plan.backward(torch.tensor(gv, device=DEV)).clone()

    p = pred.to(DEV).requires_grad_(True)
    v = mean(p, gt.to(DEV))
    assert v.requires_grad and torch.equal(v.detach(), plain(pred.to(DEV), gt.to(DEV)))
    v.backward()
    assert torch.equal(p.grad, plan_grad([0.5, 0.5]))                          # the mean divides by B
    p = pred.to(DEV).requires_grad_(True)
    (3 * mean(p, gt.to(DEV))).backward()
    assert torch.equal(p.grad, plan_grad([1.5, 1.5]))                          # 3 * lp triples the gradient
    p = pred.to(DEV).requires_grad_(True)
    (per(p, gt.to(DEV)) * torch.tensor([0.75, -1.5], device=DEV)).sum().backward()
    assert torch.equal(p.grad, plan_grad([0.75, -1.5]))
    # no_grad and detached calls: bitwise the default module's value, no graph
    with torch.no_grad():
        assert torch.equal(mean(p, gt.to(DEV)), plain(pred.to(DEV), gt.to(DEV)))
    d = mean(p.detach(), gt.to(DEV))
    assert not d.requires_grad and torch.equal(d, plain(pred.to(DEV), gt.to(DEV)))
    with pytest.raises(ValueError, match='gt.requires_grad'):
        mean(p, gt.to(DEV).requires_grad_(True))
    # one forward per backward for a shape
    a = mean(p, gt.to(DEV))
    b = mean(p, gt.to(DEV))
    with pytest.raises(RuntimeError, match='another forward of the same shape'):
        a.backward()
    b.backward()


# --------------------------------------------------------------------------------------- one training loop
def test_training_loop_with_a_perceptual_term(ev, synth_sd):
    """loss = L1 + 0.1 LPIPS on a DBSR prediction in fp32 training mode: every trainable parameter gets a finite
    gradient, and it is the network's backward of dL1/dpred + 0.1 plan.backward -- fed as pred's upstream gradient
    in a second run it gives the same parameter gradients (to the order of the fp32 sum), and they differ from the
    L1-only ones."""
    import dbsr_amd
    from dbsr_amd.burst import synthetic_bursts
    BI = 4
    burst, gt = synthetic_bursts(1, 3, 16, 16, sr_factor=8, seed=45)            # pred 1 x 3 x 128 x 128
    burst, gt = burst.to(DEV), gt.to(DEV)
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV).set_compute_dtype(torch.float32).train()
    lp = ev.LPIPS(boundary_ignore=BI, type='alex', weights=_weights('alex')[0], differentiable=True).to(DEV)
    crop = lambda t: t[..., BI:-BI, BI:-BI]

    def grads():
        out = {n: p.grad.clone() for n, p in net.named_parameters() if p.grad is not None}
        net.zero_grad(set_to_none=True)
        return out

    pred, _ = net(burst)
    assert pred.grad_fn is not None and pred.shape[-1] - 2 * BI >= 31
    (F.l1_loss(crop(pred), crop(gt)) + 0.1 * lp(pred, gt)).backward()
    both = grads()
    trainable = [n for n, p in net.named_parameters() if p.requires_grad and not n.startswith('encoder.alignment_net')]
    assert trainable and all(n in both and torch.isfinite(both[n]).all() for n in trainable)

    pred, _ = net(burst)
    F.l1_loss(crop(pred), crop(gt)).backward()
    l1_only = grads()

    pred, _ = net(burst)
    leaf = pred.detach().requires_grad_(True)
    F.l1_loss(crop(leaf), crop(gt)).backward()
    plan = lp.plan()
    plan.forward(pred.detach(), gt, BI)
    gp = plan.backward()
    assert float(gp.abs().max()) > 0
    pred.backward(leaf.grad + 0.1 * gp)
    fed = grads()
    gmax = max(float(both[n].abs().max()) for n in trainable)
    moved, real = 0, 0
    for n in trainable:
        top = float(both[n].abs().max())
        if top <= 1e-4 * gmax:     # gradients at the level of the others' rounding (the weight predictor's last bias
            # has an exact gradient of 0, softmax shift invariance): held to that level, as test_gpu_flow_grad does
            assert float((both[n] - fed[n]).abs().max()) <= 1e-4 * gmax, n
            continue
        assert float((both[n] - fed[n]).abs().max()) <= 1e-5 * top, n
        real += 1
        moved += float((both[n] - l1_only[n]).abs().max()) > 1e-4 * top
    assert real > len(trainable) // 2 and moved > real // 2
