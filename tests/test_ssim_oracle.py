"""dbsr_amd.evaluation.SSIM on CPU (the torch restatement, which is also the oracle of the HIP kernels) pinned to
values the reference's own image_quality_v2.SSIM produced (tests/golden/make_golden_ssim.py -> ssim.npz).

Bounds: the fixture records how far the reference's float32 run is from its float64 run (err_scalar, err_map);
a float32 run here is allowed twice that (the same arithmetic, possibly summed in another order), and a float64
run must reproduce the stored float64 results to 1e-12."""
import numpy as np
import pytest
import torch

from dbsr_amd import evaluation as ev

CASES = [('a40', 40), ('a8', 8), ('b3', 3)]


def _inputs(golden, tag):
    g = golden('ssim')
    if tag.startswith('a'):
        a = golden('burstsr')
        return g, torch.from_numpy(a['a_out']), torch.from_numpy(a['a_gt']), torch.from_numpy(a['a_valid'])
    return g, torch.from_numpy(g['b_pred']), torch.from_numpy(g['b_gt']), torch.from_numpy(g['b_valid'])


@pytest.mark.parametrize('tag,bi', CASES)
def test_ssim_cpu_fp32_vs_reference(golden, tag, bi):
    g, pred, gt, valid = _inputs(golden, tag)
    s = float(ev.SSIM(boundary_ignore=bi, use_for_loss=False)(pred, gt, valid=valid))
    smap = ev.ssim_map(pred[..., bi:-bi, bi:-bi], gt[..., bi:-bi, bi:-bi], 1)
    e_s = abs(s - float(g[tag + '_scalar64']))
    e_m = float((smap.double() - torch.from_numpy(g[tag + '_map64'])).abs().max())
    print('%s: scalar err %.3e (ref %.3e), map err %.3e (ref %.3e)' % (tag, e_s, g[tag + '_err_scalar'], e_m,
                                                                       g[tag + '_err_map']))
    assert e_s <= 2 * float(g[tag + '_err_scalar'])
    assert e_m <= 2 * float(g[tag + '_err_map'])
    loss = float(ev.SSIM(boundary_ignore=bi)(pred, gt, valid=valid))               # use_for_loss defaults to True
    assert abs(loss - float(g[tag + '_loss64'])) <= 2 * float(g[tag + '_err_scalar'])


@pytest.mark.parametrize('tag,bi', CASES)
def test_ssim_cpu_fp64_vs_reference(golden, tag, bi):
    g, pred, gt, valid = _inputs(golden, tag)
    p = pred.double().requires_grad_(True)
    s = ev.SSIM(boundary_ignore=bi, use_for_loss=False)(p, gt.double(), valid=valid)
    s.backward()
    assert s.dtype == torch.float64
    assert abs(float(s.detach()) - float(g[tag + '_scalar64'])) <= 1e-12
    smap = ev.ssim_map(pred.double()[..., bi:-bi, bi:-bi], gt.double()[..., bi:-bi, bi:-bi], 1)
    assert float((smap - torch.from_numpy(g[tag + '_map64'])).abs().max()) <= 1e-12
    assert float((p.grad[..., bi:-bi, bi:-bi] - torch.from_numpy(g[tag + '_dpred64'])).abs().max()) <= 1e-12
    outside = p.grad.clone()
    outside[..., bi:-bi, bi:-bi] = 0
    assert float(outside.abs().max()) == 0.0
    loss = ev.SSIM(boundary_ignore=bi, use_for_loss=True)(pred.double(), gt.double(), valid=valid)
    assert abs(float(loss) - float(g[tag + '_loss64'])) <= 1e-12


def test_ssim_no_mask_3dim_and_no_crop(golden):
    """valid is optional (the plain mean), 3-dim images are unsqueezed, boundary_ignore None means no crop."""
    g, pred, gt, _ = _inputs(golden, 'b3')
    fn = ev.SSIM(boundary_ignore=None, use_for_loss=False)
    whole = float(fn(pred[:1], gt[:1]))
    assert whole == float(fn(pred[0], gt[0]))
    assert abs(whole - float(ev.ssim_map(pred[:1], gt[:1], 1).mean())) <= 1e-7
    ones = torch.ones(1, 1, 29, 37, dtype=torch.bool)
    assert abs(whole - float(fn(pred[:1], gt[:1], valid=ones))) <= 1e-6


def test_val_range_rule(golden):
    """msssim.py:24-34: None infers the range from the (cropped) prediction."""
    g, pred, gt, valid = _inputs(golden, 'b3')
    assert ev.ssim_val_range(pred) == 1 and ev.ssim_val_range(pred - 1.0) == 2
    auto = ev.SSIM(boundary_ignore=3, use_for_loss=False)(pred, gt, valid=valid)
    one = ev.SSIM(boundary_ignore=3, use_for_loss=False, val_range=1.0)(pred, gt, valid=valid)
    assert float(auto) == float(one)
    p255, g255 = pred * 255.0, gt * 255.0
    assert float(p255.max()) > 128 and ev.ssim_val_range(p255) == 255
    s255 = ev.SSIM(boundary_ignore=3, use_for_loss=False)(p255, g255, valid=valid)
    assert float(s255) == float(ev.SSIM(boundary_ignore=3, use_for_loss=False, val_range=255)(p255, g255, valid=valid))
    assert abs(float(s255) - float(one)) <= 1e-4                    # SSIM is invariant to a common scale with its range
    assert float(ev.SSIM(boundary_ignore=3, use_for_loss=False, val_range=255)(pred, gt, valid=valid)) != float(one)
    # the rule looks at the crop only: a bright pixel in the ignored border does not select 255
    bright = pred.clone()
    bright[..., 0, 0] = 200.0
    assert float(ev.SSIM(boundary_ignore=3, use_for_loss=False)(bright, gt, valid=valid)) == float(one)


class _StubNet:
    """CPU stand-in for the network (the product forward is GPU-only): the nearest-upsampled green plane."""
    def __call__(self, burst):
        g = burst[:, 0, 1:3].mean(1, keepdim=True).repeat(1, 3, 1, 1)
        return torch.nn.functional.interpolate(g, scale_factor=8), {}


def test_compute_score_reports_ssim(tmp_path):
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(3, 2, 12, 12, sr_factor=8, seed=1)
    ev.write_synthetic_burst_val(str(tmp_path / 'ds'), burst, gt)
    ds = ev.SyntheticBurstVal(str(tmp_path / 'ds'), burst_size=2)
    s = ev.compute_score(_StubNet(), ds, boundary_ignore=8, device='cpu', batch=2)
    assert sorted(s['per_image_ssim']) == ['0000', '0001', '0002'] == sorted(s['per_image'])
    # the reference's loop (compute_score.py:92-117): one burst at a time, the quantised prediction
    ssim = ev.SSIM(boundary_ignore=8, use_for_loss=False)
    vals = []
    for i in range(3):
        b, g, meta = ds[i]
        p, _ = _StubNet()(b.unsqueeze(0))
        vals.append(float(ssim(ev.quantize_prediction(p), g.unsqueeze(0))))
        assert abs(vals[-1] - s['per_image_ssim'][meta['burst_name']]) < 1e-6
    assert abs(s['ssim'] - sum(vals) / 3) < 1e-6
    assert all(-1.0 <= v <= 1.0 for v in vals) and len(set(vals)) == 3


def test_burstsr_exports_ssim():
    from dbsr_amd import burstsr
    assert burstsr.SSIM is ev.SSIM
    assert np.isclose(float(burstsr.SSIM(use_for_loss=False)(torch.full((1, 11, 11), 0.5), torch.full((1, 11, 11), 0.5))), 1)
