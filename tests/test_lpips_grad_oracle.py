"""The host-side references of the LPIPS gradient, checked on the CPU against each other and against finite
differences, so that the GPU tests (tests/test_gpu_lpips_grad.py) compare the HIP backward with something pinned:

  * evaluation.lpips_backward_reference with its own float64 gates is float64 autograd of lpips_value (1e-12);
  * the float64 gradients of tests/golden/lpips_grad.npz agree with central differences of lpips_value (h = 1e-6
    along three seeded standard-normal directions inside the crop, 1e-6 relative): independent of torch's backward formulas;
  * the closed form of the per-layer distance (evaluation.lpips_layer_grad) equals autograd away from zero and,
    at a planted all-zero pred vector, a float64 central difference (h = 1e-16, far below eps = 1e-10, since
    n(t) = t / (|t| + eps) is linear only there): the limit dn/df = I / eps, where autograd gives NaN.
"""
import functools
import os

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips_grad.npz')
WEIGHT_SEED = 11                                        # make_golden_lpips_grad.WEIGHT_SEED


def images(shape, seed):
    """make_golden_lpips_grad.images."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = rng.random(shape, dtype=np.float64).astype(np.float32)
    pred = np.clip(gt + np.float32(0.25) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(gt)


@functools.lru_cache(maxsize=None)
def _weights(net):
    from dbsr_amd import evaluation as ev
    return ev.load_lpips_weights(ev.generate_lpips_state_dict(net, seed=WEIGHT_SEED), net)


def _cases():
    g = np.load(GOLDEN)
    return {'plain': ((1, 3, 41, 41), 4, int(g['plain_seed'])), 'b': ((2, 3, 51, 39), 4, 102)}


def _autograd(pred, gt, w, bi, flip, normalize, gvalue):
    from dbsr_amd import evaluation as ev
    p = pred.double().requires_grad_(True)
    a, g = ev.lpips_prepare(p, gt.double(), bi, flip)
    value = ev.lpips_value(a, g, w, normalize)[0]
    (value * gvalue).sum().backward()
    return value.detach(), p.grad


@pytest.mark.parametrize('net', ['alex', 'vgg'])
@pytest.mark.parametrize('case,flip,normalize,per_image', [
    ('plain', False, False, False), ('plain', True, False, True), ('b', False, True, True), ('b', True, True, False)])
def test_gated_reference_with_its_own_gates_is_autograd(net, case, flip, normalize, per_image):
    from dbsr_amd import evaluation as ev
    shape, bi, seed = _cases()[case]
    pred, gt = images(shape, seed)
    B = shape[0]
    # per_image: each value has its own upstream gradient; else the batch mean's 1 / B
    gv = torch.tensor([0.75, -1.5][:B], dtype=torch.float64) if per_image else torch.full((B,), 1.0 / B).double()
    value, want = _autograd(pred, gt, _weights(net), bi, flip, normalize, gv)
    a, g = ev.lpips_prepare(pred.double(), gt.double(), bi, flip)
    v, got = ev.lpips_backward_reference(a, g, _weights(net), normalize=normalize, gvalue=gv)
    crop = want[..., bi:-bi, bi:-bi]
    if flip:
        crop = crop[:, [2, 1, 0]]
    frame = want.clone()
    frame[..., bi:-bi, bi:-bi] = 0
    assert float(frame.abs().max()) == 0.0                                    # nothing outside the crop
    assert torch.allclose(v, value, rtol=1e-12, atol=0)
    assert float((got - crop).abs().max()) <= 1e-12 * float(crop.abs().max())


@pytest.mark.parametrize('net', ['alex', 'vgg'])
@pytest.mark.parametrize('case', ['plain', 'b'])
def test_fixture_gradient_agrees_with_central_differences(net, case):
    from dbsr_amd import evaluation as ev
    golden = np.load(GOLDEN)
    shape, bi, seed = _cases()[case]
    pred, gt = images(shape, seed)
    grad = torch.from_numpy(golden['%s_%s_grad' % (net, case)])
    assert grad.dtype == torch.float64 and tuple(grad.shape) == shape
    w, h = _weights(net), 1e-6

    def f(p):
        a, g = ev.lpips_prepare(p, gt.double(), bi)
        return float(ev.lpips_value(a, g, w)[0].sum())

    def gates(p):
        masks, argmax = ev.lpips_gates(ev.lpips_prepare(p, gt.double(), bi)[0], w)
        return torch.cat([t.flatten().long() for t in masks + argmax])

    here = gates(pred.double())
    gen = torch.Generator().manual_seed(7)
    for i in range(3):
        d = torch.zeros(shape, dtype=torch.float64)
        d[..., bi:-bi, bi:-bi] = torch.randn(shape[0], 3, shape[2] - 2 * bi, shape[3] - 2 * bi, generator=gen,
                                             dtype=torch.float64)
        # Not normalised: the difference of two values near 2e-3 carries ~1e-13 of rounding after the division by
        # 2h, which a unit direction's derivative of ~1e-7 would not stand at 1e-6 relative.  But LPIPS is only
        # piecewise smooth, and a central difference across a ReLU's kink or a change of a pool's arg-max is not
        # a derivative (vgg has pre-activations within 1e-7 of a layer's maximum of zero): the direction is
        # shortened by 4 until pred +- h d gate exactly as pred does.
        for _ in range(4):
            if all(torch.equal(gates(pred.double() + sg * h * d), here) for sg in (1, -1)):
                break
            d = d / 4
        else:
            raise AssertionError('no step without a gate change')
        fd = (f(pred.double() + h * d) - f(pred.double() - h * d)) / (2 * h)
        an = float((grad * d).sum())
        print('%s %s direction %d: central difference %.12g, gradient %.12g, relative %.2e'
              % (net, case, i, fd, an, abs(fd - an) / abs(an)))
        assert abs(fd - an) <= 1e-6 * abs(an)


def _layer_inputs(C=64, h=3, w=5, B=2):
    gen = torch.Generator().manual_seed(5)
    f0 = torch.randn(B, C, h, w, generator=gen, dtype=torch.float64).clamp(min=0)
    f1 = (f0 + 0.3 * torch.randn(B, C, h, w, generator=gen, dtype=torch.float64)).clamp(min=0)
    lin = 2.0 * torch.rand(C, generator=gen, dtype=torch.float64) / C
    gmap = torch.rand(B, h, w, generator=gen, dtype=torch.float64) + 0.5
    return f0, f1, lin, gmap


def test_layer_closed_form_is_autograd_away_from_zero():
    from dbsr_amd import evaluation as ev
    f0, f1, lin, gmap = _layer_inputs()
    f0[0, :, 1, 1] *= 1e-6 / f0[0, :, 1, 1].norm()                     # a vector of norm 1e-6
    x = f0.clone().requires_grad_(True)
    (ev.lpips_layer_map(x, f1, lin) * gmap).sum().backward()
    got = ev.lpips_layer_grad(f0, f1, lin, gmap)
    assert float((got - x.grad).abs().max()) <= 1e-12 * float(x.grad.abs().max())


def test_layer_closed_form_at_an_all_zero_vector_is_the_finite_difference():
    from dbsr_amd import evaluation as ev
    f0, f1, lin, gmap = _layer_inputs()
    f0[1, :, 2, 3] = 0
    x = f0.clone().requires_grad_(True)
    (ev.lpips_layer_map(x, f1, lin) * gmap).sum().backward()
    assert torch.isnan(x.grad[1, :, 2, 3]).all()                       # the deviation: autograd has no value here
    got = ev.lpips_layer_grad(f0, f1, lin, gmap)
    assert torch.isfinite(got).all()
    ok = torch.ones_like(f0, dtype=torch.bool)
    ok[1, :, 2, 3] = False
    assert float((got - x.grad)[ok].abs().max()) <= 1e-12 * float(got[ok].abs().max())
    n1 = f1[1, :, 2, 3] / (f1[1, :, 2, 3].norm() + ev.LPIPS_EPS)
    assert torch.allclose(got[1, :, 2, 3], -2 * gmap[1, 2, 3] * lin * n1 / ev.LPIPS_EPS, rtol=1e-12, atol=0)
    h = 1e-16

    def f(t):
        return float((ev.lpips_layer_map(t, f1, lin) * gmap).sum())

    for j in (0, 17, 63):
        e = torch.zeros_like(f0)
        e[1, j, 2, 3] = h
        fd = (f(f0 + e) - f(f0 - e)) / (2 * h)
        assert abs(fd - float(got[1, j, 2, 3])) <= 1e-5 * abs(fd), (j, fd, float(got[1, j, 2, 3]))
