"""Generate tests/golden/ssim.npz by running the REFERENCE SSIM metric on torch-CPU:
image_quality_v2.SSIM(boundary_ignore, use_for_loss=False / True) (models/loss/image_quality_v2.py:104-136) over
msssim.SSIM(spatial_out=True) (models/loss/msssim.py:10-74), with autograd to the prediction.

Build container only (needs the reference checkout make_golden.py names; `lpips` is stubbed in-process by
make_golden._install_stubs()).

Case A: a_out / a_gt / a_valid of burstsr.npz ([1, 3, 128, 128], the colour-aligned prediction and its mask; the
inputs are not stored again) at boundary_ignore 40 (keys a40_*: the scorer's setting, the mask is all ones inside
the map region) and 8 (keys a8_*: both sides of the mask are exercised, asserted below).
Case B: seeded [2, 3, 29, 37] images with a seeded random mask at boundary_ignore 3 (keys b3_*, inputs stored as
b_pred, b_gt, b_valid; main() says how the seed is chosen).

Stored per case, with X the case's prefix:
  X_map64, X_scalar64, X_loss64   the SSIM map, the masked mean (use_for_loss=False) and 1 - it (use_for_loss=True)
                                  of the inputs cast to double
  X_dpred64                       d scalar64 / d pred in double, INSIDE THE CROP only ([B, 3, H - 2 bi, W - 2 bi]; the
                                  script asserts that it is exactly zero outside), to keep the file small
  X_scalar32                      the reference's own float32 scalar
  X_err_map, X_err_scalar, X_err_grad   max |float32 run - float64 run| of the reference itself: the yardstick
                                  every implementation is held to (tests allow twice these)
  X_valid_mean                    the mask's mean over the map region

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ssim.py
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def run_case(ref_iq, pred, gt, valid, bi):
    """The reference on (pred, gt, valid) in their own dtype: map, scalar, loss, dscalar/dpred."""
    p = pred.clone().requires_grad_(True)
    scalar = ref_iq.SSIM(boundary_ignore=bi, use_for_loss=False)(p, gt, valid=valid)
    scalar.backward()
    loss = ref_iq.SSIM(boundary_ignore=bi, use_for_loss=True)(pred, gt, valid=valid)
    with torch.no_grad():
        smap = ref_iq.SSIM(boundary_ignore=bi).ssim(pred[..., bi:-bi, bi:-bi], gt[..., bi:-bi, bi:-bi])
    return smap, scalar.detach(), loss, p.grad


def case(ref_iq, tag, pred, gt, valid, bi):
    m32, s32, l32, g32 = run_case(ref_iq, pred, gt, valid, bi)
    m64, s64, l64, g64 = run_case(ref_iq, pred.double(), gt.double(), valid, bi)
    assert m32.dtype == torch.float32 and m64.dtype == torch.float64
    outside = g64.clone()
    outside[..., bi:-bi, bi:-bi] = 0
    assert outside.abs().max().item() == 0.0
    vm = valid[..., bi + 5:-bi - 5, bi + 5:-bi - 5].float().mean().item()
    d = {tag + '_map64': m64.numpy(), tag + '_scalar64': np.float64(s64.item()), tag + '_loss64': np.float64(l64.item()),
         tag + '_dpred64': g64[..., bi:-bi, bi:-bi].contiguous().numpy(), tag + '_scalar32': np.float32(s32.item()),
         tag + '_err_map': np.float64((m32.double() - m64).abs().max().item()),
         tag + '_err_scalar': np.float64(abs(s32.item() - s64.item())),
         tag + '_err_grad': np.float64((g32.double() - g64).abs().max().item()),
         tag + '_valid_mean': np.float32(vm)}
    print('%s: bi %d  scalar64 %.7f  loss64 %.7f  err_scalar %.2e  err_map %.2e  err_grad %.2e  max|grad| %.2e  '
          'valid %.3f' % (tag, bi, s64.item(), l64.item(), d[tag + '_err_scalar'], d[tag + '_err_map'],
                          d[tag + '_err_grad'], g64.abs().max().item(), vm))
    return d, vm


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden
    import npz_parts
    make_golden._install_stubs()
    sys.path.insert(0, make_golden.REF)
    import models.loss.image_quality_v2 as ref_iq

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    g = npz_parts.load(HERE, 'burstsr')
    pred, gt, valid = torch.from_numpy(g['a_out']), torch.from_numpy(g['a_gt']), torch.from_numpy(g['a_valid'])
    d = {}
    d40, vm40 = case(ref_iq, 'a40', pred, gt, valid, 40)
    d8, vm8 = case(ref_iq, 'a8', pred, gt, valid, 8)
    assert vm40 == 1.0, vm40                                   # the scorer's setting: nothing masked
    assert 0.1 < vm8 < 0.9, vm8                                # both sides of the mask are exercised
    d.update(d40)
    d.update(d8)

    # The seed is the first of 20211, 20212, ... at which the reference's float32 scalar is off its float64 one by
    # more than one float32 ulp of the value (2^-23 * scalar): below that the yardstick would be finer than the
    # format the result is stored in, and no float32 implementation could be held to it.
    for seed in range(20211, 20219):
        gen = torch.Generator().manual_seed(seed)
        b_gt = F.avg_pool2d(torch.rand(2, 3, 33, 41, generator=gen), 5, 1)      # smooth content: [2, 3, 29, 37]
        b_pred = (b_gt + 0.02 * torch.randn(b_gt.shape, generator=gen)).clamp(0.0, 1.0)
        b_valid = torch.rand(2, 1, 29, 37, generator=gen) > 0.4
        db, vmb = case(ref_iq, 'b3', b_pred, b_gt, b_valid, 3)
        if db['b3_err_scalar'] > 2.0 ** -23 * db['b3_scalar64']:
            break
    else:
        raise AssertionError('no seed gives a usable yardstick')
    print('case B seed', seed)
    assert 0.1 < vmb < 0.9, vmb
    d.update(db)
    d.update(b_pred=b_pred.numpy(), b_gt=b_gt.numpy(), b_valid=b_valid.numpy(), b_seed=np.int32(seed))

    path = os.path.join(HERE, 'ssim.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
