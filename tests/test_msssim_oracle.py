"""dbsr_amd.evaluation.MSSSIM / msssim_levels (a torch restatement, run on the host) pinned to what the
reference's own msssim.msssim produced
(tests/golden/make_golden_msssim.py -> msssim.npz): a float64 run must reproduce the stored float64 results to
1e-12."""
import math

import numpy as np
import pytest
import torch

from dbsr_amd import evaluation as ev

CASES = [('a40', 40), ('a8', 8), ('b0', 0), ('c0', 0)]
W = np.array(ev.MSSSIM_WEIGHTS, dtype=np.float32).astype(np.float64)


def _inputs(golden, tag):
    g = golden('msssim')
    if tag.startswith('a'):
        a = golden('burstsr')
        return g, torch.from_numpy(a['a_out']), torch.from_numpy(a['a_gt'])
    return g, torch.from_numpy(g[tag[0] + '_pred']), torch.from_numpy(g[tag[0] + '_gt'])


def _crop(t, bi):
    return t[..., bi:t.shape[-2] - bi, bi:t.shape[-1] - bi]


def _formula(levels, normalize, product):
    """(prod_{l<4} cs_l^w_l) * s_4^E from a [5, 2] float64 array of (s_l, cs_l)."""
    s, cs = levels[:, 0], levels[:, 1]
    if normalize:
        s, cs = (s + 1) / 2, (cs + 1) / 2
    e = W[4] if product == 'wang2003' else 4 * W[4]
    return float(np.prod(cs[:4] ** W[:4]) * s[4] ** e)


@pytest.mark.parametrize('tag,bi', CASES)
def test_msssim_cpu_fp64_vs_reference(golden, tag, bi):
    g, pred, gt = _inputs(golden, tag)
    p = pred.double().requires_grad_(True)
    value = ev.MSSSIM(boundary_ignore=bi, val_range=1)(p, gt.double())
    assert value.dtype == torch.float64 and value.dim() == 0
    value.backward()
    assert abs(float(value.detach()) - float(g[tag + '_value64'])) <= 1e-12
    levels = ev.msssim_levels(_crop(pred.double(), bi), _crop(gt.double(), bi), 1)
    got = np.array([[float(s), float(c)] for s, c in levels])
    assert levels[0][0].dtype == torch.float64
    assert np.abs(got - g[tag + '_levels64']).max() <= 1e-12
    assert float((_crop(p.grad, bi) - torch.from_numpy(g[tag + '_dpred64'])).abs().max()) <= 1e-12
    outside = p.grad.clone()
    _crop(outside, bi).zero_()
    assert float(outside.abs().max()) == 0.0
    # val_range=None infers 1 on [0, 1] images; use_for_loss returns 1 - value
    loss = ev.MSSSIM(boundary_ignore=bi, use_for_loss=True)(pred.double(), gt.double())
    assert abs(float(loss) - (1.0 - float(g[tag + '_value64']))) <= 1e-12


@pytest.mark.parametrize('tag,bi', CASES)
def test_msssim_normalize_and_products(golden, tag, bi):
    g, pred, gt = _inputs(golden, tag)
    p, q = pred.double(), gt.double()
    norm = ev.MSSSIM(boundary_ignore=bi, val_range=1, normalize=True)(p, q)
    assert abs(float(norm) - float(g[tag + '_norm64'])) <= 1e-12
    lv = g[tag + '_levels64']
    assert abs(_formula(lv, False, 'reference') - float(g[tag + '_value64'])) <= 1e-12     # the formula itself
    assert abs(_formula(lv, True, 'reference') - float(g[tag + '_norm64'])) <= 1e-12
    for normalize in (False, True):
        wang = ev.MSSSIM(boundary_ignore=bi, val_range=1, normalize=normalize, product='wang2003')(p, q)
        assert abs(float(wang) - _formula(lv, normalize, 'wang2003')) <= 1e-12
    assert float(wang) != float(norm)
    with pytest.raises(ValueError, match='product'):
        ev.MSSSIM(product='matlab')


def test_msssim_fp32_within_the_references_own_error(golden):
    """A float32 run of the restatement lands as near the float64 results as the reference's float32 run (x2)."""
    for tag, bi in CASES:
        g, pred, gt = _inputs(golden, tag)
        v = float(ev.MSSSIM(boundary_ignore=bi, val_range=1)(pred, gt))
        assert abs(v - float(g[tag + '_value64'])) <= 2 * float(g[tag + '_err_value'])


def test_msssim_nan_case(golden):
    g, _, gt = _inputs(golden, 'c0')
    neg = 1.0 - gt
    assert bool(g['n0_value64_is_nan'])
    assert math.isnan(float(ev.MSSSIM(val_range=1)(neg.double(), gt.double())))
    norm = float(ev.MSSSIM(val_range=1, normalize=True)(neg.double(), gt.double()))
    assert math.isfinite(norm) and abs(norm - float(g['n0_norm64'])) <= 1e-12


def test_msssim_per_image_equals_single_calls(golden):
    g, pred, gt = _inputs(golden, 'b0')
    p = pred.double().requires_grad_(True)
    per = ev.MSSSIM(val_range=1, per_image=True)(p, gt.double())
    assert per.shape == (2,)
    per.sum().backward()
    for b in range(2):
        pb = pred[b:b + 1].double().requires_grad_(True)
        one = ev.MSSSIM(val_range=1)(pb, gt[b:b + 1].double())
        one.backward()
        assert float(one.detach()) == float(per[b].detach())
        assert torch.equal(pb.grad[0], p.grad[b])
    batch = float(ev.MSSSIM(val_range=1)(pred.double(), gt.double()))
    assert batch != float(per.detach().mean())                      # the batch call averages the levels, not the values
    loss = ev.MSSSIM(val_range=1, per_image=True, use_for_loss=True)(pred.double(), gt.double())
    assert torch.equal(loss, 1.0 - per.detach())


def test_msssim_small_crop_raises_and_3dim(golden):
    g, pred, gt = _inputs(golden, 'c0')                     # [1, 1, 35, 47]
    with pytest.raises(ValueError, match='smaller than 32 x 32'):
        ev.MSSSIM(boundary_ignore=2, val_range=1)(pred, gt)             # a 31-pixel crop
    with pytest.raises(ValueError, match='smaller than 32 x 32'):
        ev.msssim_levels(pred[..., :31, :], gt[..., :31, :], 1)
    ok = ev.MSSSIM(boundary_ignore=1, val_range=1)(pred, gt)            # 33 x 45
    assert math.isfinite(float(ok))
    assert float(ev.MSSSIM(val_range=1)(pred[0], gt[0])) == float(ev.MSSSIM(val_range=1)(pred, gt))


def test_msssim_val_range_rule(golden):
    """None applies ssim_val_range to the cropped prediction once and uses it at all five levels."""
    g, pred, gt = _inputs(golden, 'b0')
    one = float(ev.MSSSIM(val_range=1)(pred, gt))
    assert float(ev.MSSSIM()(pred, gt)) == one
    p255, g255 = pred * 255.0, gt * 255.0
    assert float(p255.max()) > 128 and ev.ssim_val_range(p255) == 255
    auto = float(ev.MSSSIM()(p255, g255))
    assert auto == float(ev.MSSSIM(val_range=255)(p255, g255))
    assert abs(auto - one) <= 1e-4                          # invariant to a common scale with its range
    assert float(ev.MSSSIM(val_range=255)(pred, gt)) != one
    bright = pred.clone()
    bright[..., 0, 0] = 200.0                               # in the ignored border: does not select 255
    assert float(ev.MSSSIM(boundary_ignore=1)(bright, gt)) == float(ev.MSSSIM(boundary_ignore=1, val_range=1)(pred, gt))


class _StubNet:
    """CPU stand-in for the network (the product forward is GPU-only): the nearest-upsampled green plane."""
    def __call__(self, burst):
        g = burst[:, 0, 1:3].mean(1, keepdim=True).repeat(1, 3, 1, 1)
        return torch.nn.functional.interpolate(g, scale_factor=8), {}


def test_compute_score_opt_in_column(tmp_path):
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(3, 2, 12, 12, sr_factor=8, seed=1)             # 96 x 96 outputs, crop 80
    ev.write_synthetic_burst_val(str(tmp_path / 'ds'), burst, gt)
    ds = ev.SyntheticBurstVal(str(tmp_path / 'ds'), burst_size=2)
    plain = ev.compute_score(_StubNet(), ds, boundary_ignore=8, device='cpu', batch=2)
    assert sorted(plain) == ['per_image', 'per_image_ssim', 'psnr', 'ssim']      # exactly today's four keys
    s = ev.compute_score(_StubNet(), ds, boundary_ignore=8, device='cpu', batch=2, metrics=('psnr', 'ssim', 'msssim'))
    assert sorted(s) == ['msssim', 'per_image', 'per_image_msssim', 'per_image_ssim', 'psnr', 'ssim']
    assert s['per_image'] == plain['per_image'] and s['per_image_ssim'] == plain['per_image_ssim']
    assert sorted(s['per_image_msssim']) == ['0000', '0001', '0002']
    fn = ev.MSSSIM(boundary_ignore=8)
    vals = []
    for i in range(3):
        b, g, meta = ds[i]
        p, _ = _StubNet()(b.unsqueeze(0))
        vals.append(float(fn(ev.quantize_prediction(p), g.unsqueeze(0))))
        assert abs(vals[-1] - s['per_image_msssim'][meta['burst_name']]) < 1e-6
    assert abs(s['msssim'] - sum(vals) / 3) < 1e-6
    assert len(set(vals)) == 3
    with pytest.raises(ValueError, match='unknown metrics'):
        ev.compute_score(_StubNet(), ds, boundary_ignore=8, device='cpu', metrics=('lpips',))
