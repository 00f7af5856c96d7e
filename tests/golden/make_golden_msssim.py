"""Generate tests/golden/msssim.npz by running the REFERENCE msssim.msssim (models/loss/msssim.py:77-103) on
torch-CPU, in float32 and in float64, with autograd to the prediction.

Build container only (needs the reference checkout make_golden.py names).  For the float64 run create_window is
wrapped so that the float taps are cast to double, which is what msssim.SSIM.forward does (msssim.py:125); the
module's own `ssim` is patched with full=True results captured per level, so the stored (s_l, cs_l) are the very
numbers the product was formed from.  val_range is 1 throughout.

Cases (the crop is applied here, as every metric of the package does; inputs of case A are not stored again):
  a40, a8   a_out / a_gt of burstsr.npz [1, 3, 128, 128] at boundary_ignore 40 (levels 48, 24, 12, 6, 3) and 8
            (levels 112, 56, 28, 14, 7)
  b0        seeded [2, 3, 40, 52]: smooth content plus 0.02 noise, the generator of make_golden_ssim.py (b_pred, b_gt)
  c0        seeded [1, 1, 35, 47]: odd sizes, rows and columns dropped at three levels (c_pred, c_gt)
  n0        pred = 1 - gt on case c's gt: plain is NaN, normalize=True is finite (n0_value64_is_nan, n0_norm64)

Stored per case, with X the case's prefix:
  X_value64, X_norm64      the float64 value, plain and with normalize=True
  X_levels64               [5, 2] float64 (s_l, cs_l)
  X_dpred64                d value64 / d pred INSIDE THE CROP only (asserted exactly zero outside)
  X_value32                the reference's own float32 value
  X_err_value, X_err_levels [5, 2], X_err_grad, X_err_norm
                           |float32 run - float64 run| of the reference itself (max over elements for the gradient):
                           the yardstick every implementation is held to (tests allow twice these)

Asserted: every stored number is finite and every cs_l > 0; at the seeded cases the float32 value is off the
float64 one by more than one float32 ulp (seeds are searched as in make_golden_ssim.py).

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_msssim.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def run(ref, pred, gt, bi, normalize=False):
    """The reference on the crop of (pred, gt) in their own dtype: value, levels [5, 2], d value / d pred."""
    p = pred.clone().requires_grad_(True)
    crop = (lambda t: t[..., bi:-bi, bi:-bi]) if bi else (lambda t: t)
    seen = []
    plain_ssim, plain_window = ref.ssim, ref.create_window

    def recording_ssim(*a, **kw):
        sim, cs = plain_ssim(*a, **kw)
        seen.append((sim.detach(), cs.detach()))
        return sim, cs

    ref.ssim = recording_ssim
    ref.create_window = lambda size, channel=1: plain_window(size, channel).to(pred.dtype)
    try:
        value = ref.msssim(crop(p), crop(gt), val_range=1, normalize=normalize)
    finally:
        ref.ssim, ref.create_window = plain_ssim, plain_window
    assert value.dtype == pred.dtype and len(seen) == 5
    value.backward()
    levels = torch.stack([torch.stack(lv) for lv in seen])
    return value.detach(), levels, p.grad


def case(ref, tag, pred, gt, bi):
    v32, l32, g32 = run(ref, pred, gt, bi)
    v64, l64, g64 = run(ref, pred.double(), gt.double(), bi)
    n32, _, _ = run(ref, pred, gt, bi, normalize=True)
    n64, _, _ = run(ref, pred.double(), gt.double(), bi, normalize=True)
    inside = g64[..., bi:g64.shape[-2] - bi, bi:g64.shape[-1] - bi]
    outside = g64.clone()
    outside[..., bi:g64.shape[-2] - bi, bi:g64.shape[-1] - bi] = 0
    assert outside.abs().max().item() == 0.0
    d = {tag + '_value64': np.float64(v64.item()), tag + '_norm64': np.float64(n64.item()),
         tag + '_levels64': l64.numpy(), tag + '_dpred64': inside.contiguous().numpy(),
         tag + '_value32': np.float32(v32.item()),
         tag + '_err_value': np.float64(abs(v32.item() - v64.item())),
         tag + '_err_norm': np.float64(abs(n32.item() - n64.item())),
         tag + '_err_levels': (l32.double() - l64).abs().numpy(),
         tag + '_err_grad': np.float64((g32.double() - g64).abs().max().item())}
    for k, v in d.items():
        assert np.isfinite(v).all(), k
    assert (d[tag + '_levels64'][:, 1] > 0).all(), 'cs_l must be positive'
    print('%s: bi %d value64 %.7f norm64 %.7f err_value %.2e err_norm %.2e err_grad %.2e max|grad| %.2e\n'
          '    levels %s\n    err_levels %s' % (tag, bi, v64.item(), n64.item(), d[tag + '_err_value'],
                                                d[tag + '_err_norm'], d[tag + '_err_grad'], g64.abs().max().item(),
                                                np.array2string(l64.numpy().ravel(), precision=5),
                                                np.array2string(d[tag + '_err_levels'].ravel(), precision=1)))
    return d


def seeded(ref, tag, shape, seed0):
    """The first seed of seed0, seed0 + 1, ... at which the reference's float32 value is off its float64 one by
    more than one float32 ulp of the value: below that the yardstick would be finer than the format."""
    B, C, H, W = shape
    for seed in range(seed0, seed0 + 8):
        gen = torch.Generator().manual_seed(seed)
        gt = F.avg_pool2d(torch.rand(B, C, H + 4, W + 4, generator=gen), 5, 1)
        pred = (gt + 0.02 * torch.randn(gt.shape, generator=gen)).clamp(0.0, 1.0)
        d = case(ref, tag, pred, gt, 0)
        if d[tag + '_err_value'] > 2.0 ** -23 * d[tag + '_value64']:
            break
    else:
        raise AssertionError('no seed gives a usable yardstick')
    print('case', tag, 'seed', seed)
    return d, pred, gt, seed


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden
    import npz_parts
    make_golden._install_stubs()
    sys.path.insert(0, make_golden.REF)
    import models.loss.msssim as ref

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g = npz_parts.load(HERE, 'burstsr')
    pred, gt = torch.from_numpy(g['a_out']), torch.from_numpy(g['a_gt'])
    d = {}
    d.update(case(ref, 'a40', pred, gt, 40))
    d.update(case(ref, 'a8', pred, gt, 8))
    db, b_pred, b_gt, b_seed = seeded(ref, 'b0', (2, 3, 40, 52), 20311)
    dc, c_pred, c_gt, c_seed = seeded(ref, 'c0', (1, 1, 35, 47), 20411)
    d.update(db)
    d.update(dc)
    d.update(b_pred=b_pred.numpy(), b_gt=b_gt.numpy(), b_seed=np.int32(b_seed),
             c_pred=c_pred.numpy(), c_gt=c_gt.numpy(), c_seed=np.int32(c_seed))

    # pred = 1 - gt: negative cs_l, NaN from the fractional powers; finite with normalize
    neg = 1.0 - c_gt
    v64, _, _ = run(ref, neg.double(), c_gt.double(), 0)
    n64, _, _ = run(ref, neg.double(), c_gt.double(), 0, normalize=True)
    n32, _, _ = run(ref, neg, c_gt, 0, normalize=True)
    assert torch.isnan(v64) and torch.isfinite(n64)
    d.update(n0_value64_is_nan=np.bool_(True), n0_norm64=np.float64(n64.item()),
             n0_err_norm=np.float64(abs(n32.item() - n64.item())))
    print('n0: plain %s normalize %.7f (float32 off by %.2e)' % (v64.item(), n64.item(), d['n0_err_norm']))

    path = os.path.join(HERE, 'msssim.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
