"""dbsr_amd.objectives on CPU tensors -- PixelWiseError, PSNR, the masked MSE of AlignedL2 and Objective's sum --
pinned to values the reference's own image_quality_v2 classes produced (tests/golden/make_golden_objective.py ->
objective.npz): float64 runs reproduce the stored float64 losses, gradients and PSNR values to 1e-12."""
import pytest
import torch

from dbsr_amd import objectives as obj

METRICS = ('l1', 'l2', 'l2_sqrt', 'charbonnier')
CASES = [('a', 3), ('b', None), ('c', 4)]


def inputs(g, tag):
    if tag == 'b':
        return torch.from_numpy(g['b_pred_q']).float() / 256.0, torch.from_numpy(g['b_gt_q']).float() / 256.0
    return torch.from_numpy(g[tag + '_pred']), torch.from_numpy(g[tag + '_gt'])


def crop(t, bi):
    return t[..., bi:-bi, bi:-bi] if bi else t


def _check(g, key, fn, pred, gt, bi, **kw):
    p = pred.double().requires_grad_(True)
    loss = fn(p, gt.double(), **kw)
    loss.backward()
    assert loss.dtype == torch.float64
    assert abs(float(loss.detach()) - float(g[key + '_loss64'])) <= 1e-12
    assert float((crop(p.grad, bi) - torch.from_numpy(g[key + '_grad64'])).abs().max()) <= 1e-12
    outside = p.grad.clone()
    crop(outside, bi).zero_()
    assert float(outside.abs().max()) == 0.0


@pytest.mark.parametrize('metric', METRICS)
@pytest.mark.parametrize('tag,bi', CASES)
def test_pixelwise_cpu_fp64_vs_reference(golden, tag, bi, metric):
    g = golden('objective')
    pred, gt = inputs(g, tag)
    _check(g, '%s_%s' % (tag, metric), obj.PixelWiseError(metric, bi), pred, gt, bi or 0)


@pytest.mark.parametrize('metric', ['l1', 'l2'])
def test_pixelwise_masked_cpu_fp64_vs_reference(golden, metric):
    g = golden('objective')
    pred, gt = inputs(g, 'a')
    valid = torch.from_numpy(g['a_valid'])
    _check(g, 'a_%sm' % metric, obj.PixelWiseError(metric, 3), pred, gt, 3, valid=valid)


def test_masked_mse_is_aligned_l2_tail(golden):
    g = golden('objective')
    pred, gt = inputs(g, 'a')
    valid = torch.from_numpy(g['a_valid'])
    v = obj.masked_mse(pred.double(), gt.double(), valid, 3)
    assert abs(float(v) - float(g['a_al2_loss64'])) <= 1e-12
    assert abs(float(g['a_al2_loss64']) - float(g['a_l2m_loss64'])) <= 1e-12


@pytest.mark.parametrize('metric', ['l2_sqrt', 'charbonnier'])
def test_mask_refused_for_metrics_without_reduction(golden, metric):
    g = golden('objective')
    pred, gt = inputs(g, 'a')
    with pytest.raises(ValueError, match='valid mask'):
        obj.PixelWiseError(metric, 3)(pred, gt, valid=torch.from_numpy(g['a_valid']))
    with pytest.raises(ValueError, match='unknown metric'):
        obj.PixelWiseError('huber')


@pytest.mark.parametrize('tag,bi', CASES)
def test_psnr_cpu_fp64_vs_reference(golden, tag, bi):
    g = golden('objective')
    pred, gt = inputs(g, tag)
    assert abs(float(obj.PSNR(bi)(pred.double(), gt.double())) - float(g[tag + '_psnr64'])) <= 1e-12
    assert abs(float(obj.PSNR(bi, max_value=None)(pred.double(), gt.double())) - float(g[tag + '_psnr_gtmax64'])) <= 1e-12


def test_psnr_cpu_mask_and_drop_rule(golden):
    g = golden('objective')
    pred, gt = inputs(g, 'a')
    valid = torch.from_numpy(g['a_valid'])
    assert abs(float(obj.PSNR(3)(pred.double(), gt.double(), valid)) - float(g['a_psnrm64'])) <= 1e-12
    drop = pred.clone()
    drop[1] = gt[1]                                                    # image 1 is dropped: the mean of the rest
    assert abs(float(obj.PSNR(3)(drop.double(), gt.double())) - float(g['a_psnr_drop64'])) <= 1e-12
    cp, cg = inputs(g, 'c')
    assert obj.PSNR(4)(cg.double(), cg.double()) == 0 and float(g['c_psnr_alldrop64']) == 0.0


def test_objective_sum_on_cpu(golden):
    """Objective.__call__: weight * metric + ssim * (1 - SSIM) + extra(pred, gt) through the modules."""
    from dbsr_amd import evaluation as ev
    g = golden('objective')
    pred, gt = inputs(g, 'a')
    pred, gt = pred.double(), gt.double()
    o = obj.Objective('charbonnier', weight=2.0, ssim=0.2, extra=lambda p, q: 0.5 * ((p - q) ** 2).mean(),
                      boundary_ignore=3)
    want = 2.0 * float(g['a_charbonnier_loss64']) + 0.2 * float(ev.SSIM(3, val_range=1.0)(pred, gt)) + \
        0.5 * float(((pred - gt) ** 2).mean())
    assert abs(float(o(pred, gt)) - want) <= 1e-12
    assert obj.Objective.of('l2', 7).boundary_ignore == 7 and obj.Objective.of(o) is o
    with pytest.raises(ValueError):
        obj.Objective.of(3)
    with pytest.raises(ValueError):
        obj.Objective('l1', extra=1.0)
