"""Generate tests/golden/objective.npz by running the REFERENCE objectives on torch-CPU:
image_quality_v2.PixelWiseError (all four metrics; 'l1' and 'l2' also with a validity mask), image_quality_v2.PSNR
(max_value 1.0 and None) and the masked-MSE tail of image_quality_v2.AlignedL2 (models/loss/image_quality_v2.py:24-101,
176-191; its alignment is replaced by a stand-in that returns the prediction and the mask as they are), with autograd
to the prediction.

Build container only (needs the reference checkout make_golden.py names; `lpips` is stubbed in-process by
make_golden._install_stubs()).

Cases (prefix: shape, boundary_ignore):
  a: [2, 3, 37, 29], 3     ragged sizes, seeded floats, a seeded random mask (a_valid) for the masked forms
  b: [3, 3, 75, 90], none  several blocks per image; inputs on the 1/256 grid, stored as uint8 (b_pred_q, b_gt_q:
                           value = q / 256) with differences of a few levels, so that the float64 arrays compress
  c: [1, 3, 9, 9], 4       a 1 x 1 crop
Every case has a handful of elements with pred == gt exactly (sign(0), charbonnier at 0; their gt is positive) and
some with pred == 0 (the predictor's ReLU gate in the step op), and no pixel whose three differences are all zero
(torch's l2_sqrt gradient is NaN there; asserted below).

Stored per case X and metric M in l1, l2, l2_sqrt, charbonnier:
  X_M_loss64, X_M_grad64   the loss and dloss/dpred of the inputs cast to double; the gradient INSIDE THE CROP only
                           (the script asserts that it is exactly zero outside)
  X_M_err_loss, X_M_err_grad   max |float32 run - float64 run| of the reference itself (the tests' yardstick)
  a_l1m_*, a_l2m_*         the same with valid=a_valid;  a_al2_loss64: AlignedL2's tail (its gradient is asserted
                           equal to a_l2m_grad64 and not stored again)
  X_psnr64, X_psnr_gtmax64, X_psnr_err   PSNR(bi, 1.0), PSNR(bi, None) in double, and the float32 run's distance
  a_psnrm64                PSNR(3)(pred, gt, valid)
  a_psnr_drop64            PSNR(3) with image 1 of the prediction replaced by its gt (dropped: the mean of the rest)
  c_psnr_alldrop64         PSNR(4)(gt, gt): every image dropped, 0

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_objective.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402

METRICS = ('l1', 'l2', 'l2_sqrt', 'charbonnier')


def crop(t, bi):
    return t[..., bi:-bi, bi:-bi] if bi else t


def run(fn, pred, gt, **kw):
    p = pred.clone().requires_grad_(True)
    loss = fn(p, gt, **kw)
    loss.backward()
    return loss.detach(), p.grad


def both(d, key, fn, pred, gt, bi, **kw):
    l32, g32 = run(fn, pred, gt, **kw)
    l64, g64 = run(fn, pred.double(), gt.double(), **kw)
    assert l32.dtype == torch.float32 and l64.dtype == torch.float64
    assert torch.isfinite(g64).all() and torch.isfinite(g32).all(), key
    outside = g64.clone()
    crop(outside, bi).zero_()
    assert outside.abs().max().item() == 0.0
    d[key + '_loss64'] = np.float64(l64.item())
    d[key + '_grad64'] = crop(g64, bi).contiguous().numpy()
    d[key + '_err_loss'] = np.float64(abs(l32.item() - l64.item()))
    d[key + '_err_grad'] = np.float64((g32.double() - g64).abs().max().item())
    print('%-18s loss64 %.9f  err_loss %.2e  err_grad %.2e  max|grad| %.2e'
          % (key, l64.item(), d[key + '_err_loss'], d[key + '_err_grad'], g64.abs().max().item()))
    return g64


def check_inputs(tag, pred, gt, bi):
    dz = crop(pred - gt, bi) == 0
    assert int(dz.sum()) >= 3, (tag, 'too few pred == gt elements in the crop')
    assert not bool(dz.all(dim=1).any()), (tag, 'a pixel with all three differences zero')
    assert bool((crop(gt, bi)[dz] > 0).all())
    assert int((crop(pred, bi) == 0).sum()) >= 1, (tag, 'no pred == 0 element in the crop')
    assert float(pred.min()) >= 0.0


def psnr_value(ref_iq, bi, max_value, pred, gt, valid=None):
    v = ref_iq.PSNR(boundary_ignore=bi, max_value=max_value)(pred, gt, valid=valid)
    return float(v)


def case(ref_iq, d, tag, pred, gt, bi):
    check_inputs(tag, pred, gt, bi or 0)
    for m in METRICS:
        both(d, '%s_%s' % (tag, m), ref_iq.PixelWiseError(metric=m, boundary_ignore=bi), pred, gt, bi or 0)
    for name, mv in (('psnr', 1.0), ('psnr_gtmax', None)):
        v64 = psnr_value(ref_iq, bi, mv, pred.double(), gt.double())
        v32 = psnr_value(ref_iq, bi, mv, pred, gt)
        d['%s_%s64' % (tag, name)] = np.float64(v64)
        if name == 'psnr':
            d[tag + '_psnr_err'] = np.float64(abs(v32 - v64))
        print('%-18s %.9f (float32 run off by %.2e)' % (tag + '_' + name, v64, abs(v32 - v64)))


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden
    make_golden._install_stubs()
    sys.path.insert(0, make_golden.REF)
    import models.loss.image_quality_v2 as ref_iq

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    d = {}

    # ---- a: ragged, floats, mask
    gen = torch.Generator().manual_seed(20231)
    a_gt = 0.05 + 0.9 * torch.rand(2, 3, 37, 29, generator=gen)
    a_pred = (a_gt + 0.05 * torch.randn(a_gt.shape, generator=gen)).clamp(0.0, 1.0)
    a_valid = torch.rand(2, 1, 37, 29, generator=gen) > 0.4
    for (b, c, y, x) in ((0, 0, 5, 5), (0, 1, 20, 11), (1, 2, 33, 25), (1, 0, 3, 3), (0, 2, 17, 9)):
        a_pred[b, c, y, x] = a_gt[b, c, y, x]
    for (b, c, y, x) in ((0, 1, 6, 7), (1, 0, 18, 18), (1, 2, 30, 4), (0, 0, 0, 0), (0, 2, 12, 20)):
        a_pred[b, c, y, x] = 0.0
    case(ref_iq, d, 'a', a_pred, a_gt, 3)
    g_l2m = None
    for m in ('l1', 'l2'):
        g = both(d, 'a_%sm' % m, ref_iq.PixelWiseError(metric=m, boundary_ignore=3), a_pred, a_gt, 3, valid=a_valid)
        g_l2m = g if m == 'l2' else g_l2m
    al2 = ref_iq.AlignedL2.__new__(ref_iq.AlignedL2)
    torch.nn.Module.__init__(al2)
    al2.boundary_ignore = 3
    al2.sca = lambda pred, gt, burst: (pred, a_valid)          # the tail alone: no warp, no colour match
    l64, g64 = run(lambda p, g: al2(p, g, None), a_pred.double(), a_gt.double())
    assert float((g64 - g_l2m).abs().max()) == 0.0
    d['a_al2_loss64'] = np.float64(l64.item())
    d['a_psnrm64'] = np.float64(psnr_value(ref_iq, 3, 1.0, a_pred.double(), a_gt.double(), a_valid))
    drop = a_pred.clone()
    drop[1] = a_gt[1]
    d['a_psnr_drop64'] = np.float64(psnr_value(ref_iq, 3, 1.0, drop.double(), a_gt.double()))
    one = psnr_value(ref_iq, 3, 1.0, a_pred[:1].double(), a_gt[:1].double())
    assert abs(d['a_psnr_drop64'] - one) < 1e-12               # the mean of the remaining image
    d.update(a_pred=a_pred.numpy(), a_gt=a_gt.numpy(), a_valid=a_valid.numpy())

    # ---- b: several blocks per image, the 1/256 grid
    gen = torch.Generator().manual_seed(20232)
    gq = torch.randint(8, 248, (3, 3, 75, 90), generator=gen)
    dq = torch.randint(-3, 4, gq.shape, generator=gen)
    zero3 = (dq == 0).all(dim=1, keepdim=True).expand_as(dq).clone()
    zero3[:, 1:] = False
    dq[zero3] = 2                                              # no pixel with all three differences zero
    pq = gq + dq
    for (b, c, y, x) in ((0, 0, 0, 0), (1, 1, 40, 45), (2, 2, 74, 89), (2, 0, 10, 80)):
        pq[b, c, y, x] = 0
    b_pred, b_gt = pq.float() / 256.0, gq.float() / 256.0
    case(ref_iq, d, 'b', b_pred, b_gt, None)
    d.update(b_pred_q=pq.to(torch.uint8).numpy(), b_gt_q=gq.to(torch.uint8).numpy())

    # ---- c: a 1 x 1 crop
    gen = torch.Generator().manual_seed(20233)
    c_gt = 0.05 + 0.9 * torch.rand(1, 3, 9, 9, generator=gen)
    c_pred = (c_gt + 0.05 * torch.randn(c_gt.shape, generator=gen)).clamp(0.0, 1.0)
    c_pred[0, 1, 4, 4] = c_gt[0, 1, 4, 4]
    c_pred[0, 2, 4, 4] = 0.0
    check = crop(c_pred - c_gt, 4)
    assert check.shape[-2:] == (1, 1)
    # (the crop has three elements: one with pred == gt, one with pred == 0; check_inputs wants three zeros)
    dz = check == 0
    assert int(dz.sum()) == 1 and not bool(dz.all(dim=1).any())
    for m in METRICS:
        both(d, 'c_%s' % m, ref_iq.PixelWiseError(metric=m, boundary_ignore=4), c_pred, c_gt, 4)
    d['c_psnr64'] = np.float64(psnr_value(ref_iq, 4, 1.0, c_pred.double(), c_gt.double()))
    d['c_psnr_gtmax64'] = np.float64(psnr_value(ref_iq, 4, None, c_pred.double(), c_gt.double()))
    d['c_psnr_err'] = np.float64(abs(psnr_value(ref_iq, 4, 1.0, c_pred, c_gt) - float(d['c_psnr64'])))
    d['c_psnr_alldrop64'] = np.float64(psnr_value(ref_iq, 4, 1.0, c_gt.double(), c_gt.double()))
    assert d['c_psnr_alldrop64'] == 0.0
    d.update(c_pred=c_pred.numpy(), c_gt=c_gt.numpy())

    path = os.path.join(HERE, 'objective.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
