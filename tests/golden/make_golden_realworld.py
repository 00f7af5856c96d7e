"""Generate tests/golden/realworld.npz by running the REFERENCE real-world objective on torch-CPU:
SpatialColorAlignment (models/loss/spatial_color_alignment.py:87-108) + PixelWiseError('l1',
boundary_ignore=40) (models/loss/image_quality_v2.py:24-66) times the loss weight 10
(train_settings/dbsr/default_realworld.py:65-79, actors/dbsr_actors.py:68-80), with autograd to the
prediction, on fixture A of burstsr.npz (a_pred with requires_grad, a_gt, a_burst).

Build container only (needs the reference checkout make_golden.py names).  Same in-process stubs as
make_golden_burstsr.py (cupy, lpips, admin.local, torch.lstsq, FunctionCorrelation) and the same PWC-Net
weights (the alignment-net part of generate_state_dict(seed=0)).

Stored: loss (scalar) and dpred [1, 3, 128, 128] fp32, plus the fraction of the 40-pixel crop that is valid.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_realworld.py
"""
import os
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    sys.path.insert(0, HERE)
    sys.path.insert(0, REPO)
    import make_golden
    import npz_parts
    from oracle import dbsr_oracle as orc
    import dbsr_amd
    from dbsr_amd import arch
    from dbsr_amd.weights import generate_state_dict
    make_golden._install_stubs()

    def lstsq(B, A):
        sol = torch.linalg.lstsq(A, B).solution
        m, n = A.shape
        full = torch.zeros(max(m, n), B.shape[1], dtype=sol.dtype)
        full[:n] = sol
        return types.SimpleNamespace(solution=full)
    torch.lstsq = lstsq

    sys.path.insert(0, make_golden.REF)
    import models.alignment.pwcnet as ref_pwc
    import models.loss.spatial_color_alignment as ref_sca
    import models.loss.image_quality_v2 as ref_iq
    ref_pwc.correlation.FunctionCorrelation = lambda tenFirst, tenSecond: orc.correlation(tenFirst, tenSecond)

    torch.set_num_threads(min(16, os.cpu_count() or 1))
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    sd = generate_state_dict(arch.state_dict_shapes(net), seed=0)
    pre = 'encoder.alignment_net.'
    pwc = ref_pwc.PWCNet(load_pretrained=False).eval()
    pwc.load_state_dict({k[len(pre):]: torch.from_numpy(v) for k, v in sd.items() if k.startswith(pre)})

    g = npz_parts.load(HERE, 'burstsr')
    pred = torch.from_numpy(g['a_pred']).clone().requires_grad_(True)
    gt, burst = torch.from_numpy(g['a_gt']), torch.from_numpy(g['a_burst'])
    sca = ref_sca.SpatialColorAlignment(pwc, sr_factor=4)
    obj = ref_iq.PixelWiseError(metric='l1', boundary_ignore=40)
    out, valid = sca(pred, gt, burst)
    loss = 10.0 * obj(out, gt, valid=valid)
    loss.backward()
    assert np.array_equal(valid.numpy(), g['a_valid'])
    valid_crop = valid[..., 40:-40, 40:-40].float()
    assert 0.2 < valid_crop.mean() < 0.95, valid_crop.mean()         # both sides of the mask are exercised
    d = dict(loss=np.float32(loss.item()), dpred=pred.grad.numpy().astype(np.float32),
             valid_crop_mean=np.float32(valid_crop.mean().item()))
    print('loss %.6f  |dpred| max %.3e  valid in crop %.3f' % (loss.item(), pred.grad.abs().max(), valid_crop.mean()))
    path = os.path.join(HERE, 'realworld.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path))


if __name__ == '__main__':
    main()
