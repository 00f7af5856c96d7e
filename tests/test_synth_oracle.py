"""CPU checks of dbsr_amd.synthetic against tests/golden/synth.npz (the reference's camera pipeline run on torch-CPU,
tests/golden/make_golden_synth.py): the torch restatements are held to twice the reference's own fp32 error, the host
samplers reproduce the reference's values under the same seeds, and the transform helpers satisfy closed forms."""
import math
import random

import numpy as np
import pytest
import torch


@pytest.fixture(scope='module')
def g(golden):
    return golden('synth')


@pytest.fixture(scope='module')
def S():
    from dbsr_amd import synthetic
    return synthetic


UN_SETS = {'a': (True, True, False), 'b': (True, False, False), 'c': (False, True, False), 'd': (False, False, True)}


def _within(out, ref64, err, what):
    e = (out.double() - torch.from_numpy(ref64)).abs().max().item()
    print('%s: max |out - ref64| %.3e, bar 2 x %.3e' % (what, e, err))
    assert e <= 2 * err, (what, e, err)


@pytest.mark.parametrize('tag', sorted(UN_SETS))
def test_unprocess_restatement(g, S, tag):
    ss, gm, ident = UN_SETS[tag]
    x = torch.from_numpy(g['un_img_u8']).permute(0, 3, 1, 2).float() / 255.0
    out = []
    for b in range(2):
        m = torch.eye(3) if ident else torch.from_numpy(g['un_rgb2cam'][b])
        gains = (1.0, 1.0, 1.0) if ident else tuple(float(v) for v in g['un_gains'][b])
        out.append(S.unprocess_rgb_cpu(x[b], m, *gains, smoothstep=ss, gamma=gm))
    out = torch.stack(out)
    assert out.dtype == torch.float32
    _within(out, g['un_%s_ref64' % tag], float(g['un_%s_err' % tag]), 'unprocess ' + tag)


def test_mosaic_and_noise_restatement(g, S):
    rgb = torch.from_numpy(g['ns_rgb'])
    mos = S.mosaic(rgb)
    assert torch.equal(mos, torch.from_numpy(g['ns_mosaic']))
    shot, read = (float(v) for v in g['ns_levels'])
    out = S.add_noise_cpu(mos, shot, read, torch.from_numpy(g['ns_z']))
    _within(out, g['ns_ref64'], float(g['ns_err']), 'noise')


def test_postprocess_restatement(g, S):
    img = torch.from_numpy(g['pp_img'])
    rgb, red, blue = (float(v) for v in g['pp_gains'])
    for i, (ga, cc, gm, ss, mg, ms) in enumerate(g['pp_cases'].tolist()):
        meta = {'cam2rgb': torch.from_numpy(g['pp_cam2rgb']), 'rgb_gain': rgb, 'red_gain': red, 'blue_gain': blue,
                'gamma': bool(mg), 'smoothstep': bool(ms)}
        kw = dict(gains=bool(ga), ccm=bool(cc), gamma=bool(gm), smoothstep=bool(ss))
        out = S.process_linear_image_rgb(img, meta, **kw)                # CPU tensor: the torch restatement
        assert out.shape == img.shape and out.dtype == torch.float32
        _within(out, g['pp_ref64'][i], float(g['pp_err'][i]), 'postprocess %d' % i)
        # batched input and batched meta_info, and the uint8 array
        metab = dict(meta, cam2rgb=meta['cam2rgb'][None].repeat(2, 1, 1), rgb_gain=torch.tensor([rgb, rgb]),
                     red_gain=torch.tensor([red, red]), blue_gain=torch.tensor([blue, blue]))
        outb = S.process_linear_image_rgb(torch.stack([img, img]), metab, **kw)
        assert torch.equal(outb[0], out) and torch.equal(outb[1], out)
        u8 = S.SimplePostProcess(return_np=True, **kw).process(img, meta)
        assert u8.dtype == np.uint8 and u8.shape == (24, 40, 3)
        assert np.array_equal(u8, (out.permute(1, 2, 0).numpy() * 255).astype(np.uint8))


def test_samplers_reproduce_reference(g, S):
    for i, (ps, ts) in enumerate(g['sm_seeds'].tolist()):
        random.seed(ps)
        torch.manual_seed(ts)
        ccm = S.random_ccm()
        gains = S.random_gains()
        noise = S.random_noise_levels()
        assert ccm.dtype == torch.float32 and np.array_equal(ccm.numpy(), g['sm_ccm'][i])
        assert np.array_equal(np.array(gains, dtype=np.float64), g['sm_gains'][i])           # to the last bit
        assert np.array_equal(np.array(noise, dtype=np.float64), g['sm_noise'][i])


def test_get_tmat_closed_forms(S):
    shape = (48, 64)
    cx, cy = 32.0, 24.0
    np.testing.assert_array_equal(S.get_tmat(shape, (0.0, 0.0), 0.0, (0.0, 0.0), (1.0, 1.0)),
                                  np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]))
    np.testing.assert_array_equal(S.get_tmat(shape, (3.5, -2.0), 0.0, (0.0, 0.0), (1.0, 1.0)),
                                  np.array([[1.0, 0.0, 3.5], [0.0, 1.0, -2.0]]))
    r = S.get_tmat(shape, (0.0, 0.0), 90.0, (0.0, 0.0), (1.0, 1.0))
    np.testing.assert_allclose(r @ np.array([cx + 1.0, cy, 1.0]), [cx, cy - 1.0], atol=1e-12)
    np.testing.assert_allclose(r @ np.array([cx, cy, 1.0]), [cx, cy], atol=1e-12)
    # the order of composition, against a product written out here
    tr, th, sh, sc = (2.0, -1.5), 7.0, (0.03, -0.02), (1.1, 0.9)
    a, b = math.cos(math.radians(th)), math.sin(math.radians(th))
    t_tr = np.array([[1, 0, tr[0]], [0, 1, tr[1]], [0, 0, 1.0]])
    t_rot = np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy], [0, 0, 1.0]])
    t_sh = np.array([[1, sh[0], -sh[0] * cx], [sh[1], 1, -sh[1] * cy], [0, 0, 1.0]])
    t_sc = np.diag([sc[0], sc[1], 1.0])
    want = (t_sc @ t_rot @ t_sh @ t_tr)[:2]
    got = S.get_tmat(shape, tr, th, sh, sc)
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-12)
    other = (t_tr @ t_sh @ t_rot @ t_sc)[:2]
    assert np.abs(got - other).max() > 1e-3                                 # the order is observable
    inv = S.inverse_tmat(got)
    p = np.array([10.0, 20.0, 1.0])
    np.testing.assert_allclose(inv @ np.append(got @ p, 1.0), p[:2], atol=1e-10)


def test_sample_transform_replays_the_draws(S):
    f = 4
    assert S.sample_transform({'max_translation': 24.0}, f, first=True) == ((1.5, 1.5), 0.0, (0.0, 0.0), (1.0, 1.0))
    params = {'max_translation': 24.0, 'max_rotation': 1.0, 'max_shear': 0.0, 'max_scale': 0.0, 'border_crop': 24}
    random.seed(99)
    state = random.getstate()
    got = [S.sample_transform(params, f) for _ in range(2)]
    after = random.random()
    random.setstate(state)
    for tr, th, sh, sc in got:
        tx = random.uniform(-24.0, 24.0)
        ty = random.uniform(-24.0, 24.0)
        theta = random.uniform(-1.0, 1.0)
        shx = random.uniform(-0.0, 0.0)                  # maxima of 0 still consume their draws
        shy = random.uniform(-0.0, 0.0)
        ar = np.exp(random.uniform(-0.0, 0.0))
        s = np.exp(random.uniform(-0.0, 0.0))
        assert (tr, th, sh, sc) == ((tx, ty), theta, (shx, shy), (s, s * ar))
        assert sh == (0.0, 0.0) and sc == (1.0, 1.0)
    assert random.random() == after                      # exactly seven draws per frame
    # max_translation <= 0.01: the centring shift, and (as the reference) no translation draws
    random.seed(5)
    tr, th, _, _ = S.sample_transform({'max_translation': 0.0, 'max_rotation': 2.0}, f)
    random.seed(5)
    assert tr == (1.5, 1.5) and th == random.uniform(-2.0, 2.0)


def test_unsupported_options_raise(S):
    with pytest.raises(NotImplementedError, match='lanczos'):
        S.rgb2rawburst(torch.zeros(3, 8, 8), 2, interpolation_type='lanczos')
    with pytest.raises(NotImplementedError, match='crop_scale_range'):
        S.SyntheticBurstProcessing(64, 4, 4, crop_scale_range=(0.5, 1.0))
    with pytest.raises(NotImplementedError, match='crop_ar_range'):
        S.SyntheticBurstProcessing(64, 4, 4, crop_ar_range=(0.9, 1.1))
    with pytest.raises(NotImplementedError, match='HIP device'):                # the generator is the HIP path only
        S.rgb2rawburst(torch.zeros(3, 8, 8), 2)


def test_save_visualization_needs_camera_meta(tmp_path):
    """SyntheticBurstVal samples carry 'burst_name' only: refused before the network is touched."""
    from dbsr_amd import evaluation as ev
    with pytest.raises(ValueError, match='meta_info'):
        ev.save_visualization(None, [(torch.zeros(2, 4, 8, 8), torch.zeros(3, 64, 64), {'burst_name': '0000'})],
                              str(tmp_path))
