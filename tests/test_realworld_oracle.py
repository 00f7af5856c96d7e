"""The torch restatement of the real-world objective that the GPU tests compare against (tests/realworld_ref.py:
oracle.warp + oracle.match_colors + the masked L1 x 10, flow under no_grad) reproduces the REFERENCE's own loss
and gradient on fixture A of burstsr.npz (tests/golden/make_golden_realworld.py ran SpatialColorAlignment +
PixelWiseError('l1', boundary_ignore=40) x 10 with autograd on torch-CPU).  Bars as test_oracle.py's: the loss
to 1e-5 relative, the gradient to 1e-6 of its largest entry."""
import numpy as np
import torch

from tests.realworld_ref import sca_objective


def test_oracle_realworld_objective_vs_reference(golden, synth_sd):
    g, r = golden('burstsr'), golden('realworld')
    loss, dpred, (flow, cmat, valid) = sca_objective(torch.from_numpy(g['a_pred']), torch.from_numpy(g['a_gt']),
                                                     torch.from_numpy(g['a_burst']), synth_sd, bi=40, weight=10.0)
    np.testing.assert_array_equal(valid.numpy(), g['a_valid'])
    crop = g['a_valid'][..., 40:-40, 40:-40].mean()
    assert 0.2 < crop < 0.95 and abs(crop - float(r['valid_crop_mean'])) < 1e-6      # both sides of the mask
    print('loss', float(loss), float(r['loss']))
    assert abs(float(loss) - float(r['loss'])) <= 1e-5 * abs(float(r['loss']))
    d = np.abs(dpred.numpy() - r['dpred']).max() / np.abs(r['dpred']).max()
    print('dpred max diff / max', d)
    assert r['dpred'].shape == (1, 3, 128, 128) and np.abs(r['dpred']).max() > 0
    assert d <= 1e-6, d
    # outside the crop and the mask the gradient is exactly zero only before the warp: after warp^T a border
    # pixel can receive a tap, so only the far border (beyond the largest flow) is checked
    reach = int(np.ceil(np.abs(g['a_flow']).max())) + 1
    assert not dpred[..., :40 - reach, :].any() and not dpred[..., :, :40 - reach].any()
