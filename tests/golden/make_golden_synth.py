"""Generate tests/golden/synth.npz by running the REFERENCE camera pipeline on torch-CPU: data/camera_pipeline.py
(random_ccm, random_gains, random_noise_levels, invert_smoothstep, gamma_expansion, apply_ccm, safe_invert_gains,
mosaic, add_noise) in the order rgb2rawburst calls them (data/synthetic_burst_generation.py:47-97), and
data/postprocessing_functions.process_linear_image_rgb.

Build container only (needs the reference checkout make_golden.py names).  `import data` fails on this stack
(data/__init__.py pulls torch._six through the loaders), so a bare `data` package with only __path__ set is
registered and the two modules are loaded from their files; cv2 is stubbed as an empty module, the way lpips is
(nothing of cv2 is called with return_np=False).

Every group stores the reference's result on float64 inputs (X_ref64), on float32 inputs (X_ref32) and
X_err = max |ref32 - ref64|: the reference's own fp32 rounding error, the yardstick tests hold every implementation
to (they allow twice it).

  un_*   the unprocess chain on un_img_u8 [2,24,40,3] uint8 (the image fed is value / 255, as the recipe's 8-bit
         crops are), per image un_rgb2cam [2,3,3] and un_gains [2,3] = (rgb, red, blue) float64.  Flag sets
         a: smoothstep + gamma, b: smoothstep only, c: gamma only, d: neither, with the identity matrix and unit
         gains.  The image holds 0 and 255 and a highlight block; the script asserts that safe_invert_gains' mask
         is non-zero on some pixels and zero on others, for every set.
  ns_*   mosaic and add_noise (then rgb2rawburst's clamp) on ns_rgb [3,3,12,20]: ns_mosaic, the normals ns_z
         (recorded by re-seeding torch and drawing the same FloatTensor(shape).normal_()), ns_levels (shot, read).
  pp_*   process_linear_image_rgb on pp_img [3,24,40] (values spill below 0 and above 1), pp_cam2rgb, pp_gains;
         pp_cases [7,6] = (gains, ccm, gamma, smoothstep arguments, meta gamma, meta smoothstep): all on, then each
         switched off once.  The script asserts that, per case, at most 1 % of the elements have ref64 * 255 within
         255 * 2 * err of an integer, and that the reference's own float32 run truncates to floor(ref64 * 255)
         everywhere else.
  sm_*   random_ccm, random_gains, random_noise_levels (called in that order) under three
         (random.seed, torch.manual_seed) pairs sm_seeds [3,2]: sm_ccm [3,3,3] float32, sm_gains [3,3] and
         sm_noise [3,2] float64.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_synth.py
"""
import importlib.util
import os
import random
import sys
import types

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def load_reference():
    sys.path.insert(0, HERE)
    import make_golden
    ref = make_golden.REF
    sys.path.insert(0, ref)
    sys.modules['cv2'] = types.ModuleType('cv2')
    pkg = types.ModuleType('data')
    pkg.__path__ = [os.path.join(ref, 'data')]
    sys.modules['data'] = pkg
    mods = {}
    for name in ('camera_pipeline', 'postprocessing_functions'):
        spec = importlib.util.spec_from_file_location('data.' + name, os.path.join(ref, 'data', name + '.py'))
        mod = importlib.util.module_from_spec(spec)
        sys.modules['data.' + name] = mod
        spec.loader.exec_module(mod)
        mods[name] = mod
    return mods['camera_pipeline'], mods['postprocessing_functions']


def unprocess(cp, image, rgb2cam, gains, smoothstep, gamma):
    """rgb2rawburst:60-77; also returns safe_invert_gains' mask."""
    if smoothstep:
        image = cp.invert_smoothstep(image)
    if gamma:
        image = cp.gamma_expansion(image)
    image = cp.apply_ccm(image, rgb2cam)
    mask = ((image.mean(dim=0, keepdims=True) - 0.9).clamp(0.0) / (1.0 - 0.9)) ** 2.0
    image = cp.safe_invert_gains(image, *gains)
    return image.clamp(0.0, 1.0), mask


def main():
    cp, pf = load_reference()
    torch.set_num_threads(1)
    d = {}

    # ---- unprocess chain
    rng = np.random.RandomState(20260)
    img = rng.randint(0, 200, size=(2, 24, 40, 3)).astype(np.uint8)
    img[:, 4:10, 6:16, :] = rng.randint(236, 256, size=(2, 6, 10, 3)).astype(np.uint8)        # highlights
    img[:, 0, 0, :] = 0
    img[:, 0, 1, :] = 255
    img[:, 0, 2, :] = (255, 0, 128)
    random.seed(11)
    torch.manual_seed(11)
    ccms, gains = [], []
    for _ in range(2):
        ccms.append(cp.random_ccm())
        gains.append(cp.random_gains())
    d.update(un_img_u8=img, un_rgb2cam=torch.stack(ccms).numpy(), un_gains=np.array(gains, dtype=np.float64))
    x32 = torch.from_numpy(img).permute(0, 3, 1, 2).float() / 255.0
    assert x32.min() == 0.0 and x32.max() == 1.0
    for tag, ss, gm, ident in (('a', True, True, False), ('b', True, False, False), ('c', False, True, False),
                               ('d', False, False, True)):
        r64, r32 = [], []
        for b in range(2):
            m = torch.eye(3) if ident else ccms[b]
            g = (1.0, 1.0, 1.0) if ident else gains[b]
            o64, mask = unprocess(cp, x32[b].double(), m, g, ss, gm)
            o32, _ = unprocess(cp, x32[b], m, g, ss, gm)
            assert o64.dtype == torch.float64 and o32.dtype == torch.float32
            assert (mask > 0).any() and (mask == 0).any(), 'the mask branch must be exercised on both sides'
            r64.append(o64)
            r32.append(o32)
        r64, r32 = torch.stack(r64), torch.stack(r32)
        err = (r32.double() - r64).abs().max().item()
        d.update({'un_%s_ref64' % tag: r64.numpy(), 'un_%s_ref32' % tag: r32.numpy(), 'un_%s_err' % tag: np.float64(err)})
        print('unprocess %s: err %.3e  mean %.4f  clamped at 1: %.3f' % (tag, err, r64.mean().item(),
                                                                          (r64 == 1.0).double().mean().item()))

    # ---- mosaic and noise
    gen = torch.Generator().manual_seed(20261)
    rgb = torch.rand(3, 3, 12, 20, generator=gen)
    rgb[0, :, 0, :4] = 0.0
    rgb[0, :, 1, :4] = 1.0
    random.seed(12)
    shot, read = cp.random_noise_levels()
    shot = max(shot, 0.004)                       # a level at which the noise clamps some values at both ends
    res = {}
    for name, x in (('ref32', rgb), ('ref64', rgb.double())):
        mos = cp.mosaic(x.clone())
        torch.manual_seed(20262)
        res[name] = cp.add_noise(mos, shot, read).clamp(0.0, 1.0)
        res[name + '_mos'] = mos
    torch.manual_seed(20262)
    z = torch.FloatTensor(res['ref32_mos'].shape).normal_()
    assert torch.equal(res['ref32'], (res['ref32_mos'] + z * (res['ref32_mos'] * shot + read).sqrt()).clamp(0.0, 1.0))
    assert res['ref64'].dtype == torch.float64
    assert (res['ref64'] == 0).any() and (res['ref64'] == 1).any()
    err = (res['ref32'].double() - res['ref64']).abs().max().item()
    d.update(ns_rgb=rgb.numpy(), ns_mosaic=res['ref32_mos'].numpy(), ns_z=z.numpy(),
             ns_levels=np.array([shot, read], dtype=np.float64), ns_ref64=res['ref64'].numpy(),
             ns_ref32=res['ref32'].numpy(), ns_err=np.float64(err))
    print('noise: shot %.4g read %.4g err %.3e' % (shot, read, err))

    # ---- postprocess
    random.seed(13)
    torch.manual_seed(13)
    rgb2cam = cp.random_ccm()
    rgb_gain, red_gain, blue_gain = cp.random_gains()
    cam2rgb = rgb2cam.inverse()
    gen = torch.Generator().manual_seed(20263)
    base = 0.04 + 0.88 * torch.rand(1, 24, 40, generator=gen)
    wb = torch.tensor([1.0 / red_gain, 1.0, 1.0 / blue_gain]).view(3, 1, 1) / rgb_gain
    pimg = base * wb * (1.0 + 0.05 * (torch.rand(3, 24, 40, generator=gen) - 0.5))
    pimg[:, 3, 5:8] = torch.tensor([-0.05, -0.2, -0.01])                    # spills below 0 ...
    pimg[:, 9, 5:8] = torch.tensor([1.3, 1.05, 2.0])                        # ... and above 1
    pimg[0, 15, 7] = 1.5
    pimg[2, 15, 9] = -0.3
    assert pimg.min() < 0 and pimg.max() > 1
    cases = [(1, 1, 1, 1, 1, 1), (0, 1, 1, 1, 1, 1), (1, 0, 1, 1, 1, 1), (1, 1, 0, 1, 1, 1), (1, 1, 1, 0, 1, 1),
             (1, 1, 1, 1, 0, 1), (1, 1, 1, 1, 1, 0)]
    r64s, r32s, errs = [], [], []
    for ga, cc, gm, ss, mg, ms in cases:
        meta = {'rgb_gain': rgb_gain, 'red_gain': red_gain, 'blue_gain': blue_gain, 'cam2rgb': cam2rgb,
                'gamma': bool(mg), 'smoothstep': bool(ms)}
        kw = dict(gains=bool(ga), ccm=bool(cc), gamma=bool(gm), smoothstep=bool(ss), return_np=False)
        o64 = pf.process_linear_image_rgb(pimg.double(), meta, **kw)
        o32 = pf.process_linear_image_rgb(pimg, meta, **kw)
        assert o64.dtype == torch.float64 and o32.dtype == torch.float32
        # what reaches the first clamp of this case lies on both sides of [0, 1]: the clamps matter
        g3 = (torch.tensor([red_gain, 1.0, blue_gain]) * rgb_gain).view(3, 1, 1).double()
        first = pimg.double() * g3 if ga else (cp.apply_ccm(pimg.double(), cam2rgb) if cc else pimg.double())
        assert (first < 0).any() and (first > 1).any(), 'the clamps must matter'
        err = (o32.double() - o64).abs().max().item()
        v = o64 * 255
        near = (v - v.round()).abs() <= 255 * 2 * err
        share = near.double().mean().item()
        assert share <= 0.01, share
        u32 = (o32.numpy() * 255).astype(np.uint8)                          # torch_to_npimage's arithmetic
        assert np.array_equal(u32[~near.numpy()], np.floor(v.numpy())[~near.numpy()].astype(np.uint8))
        r64s.append(o64)
        r32s.append(o32)
        errs.append(err)
        print('postprocess %s: err %.3e  near-integer share %.4f' % ((ga, cc, gm, ss, mg, ms), err, share))
    d.update(pp_img=pimg.numpy(), pp_cam2rgb=cam2rgb.numpy(),
             pp_gains=np.array([rgb_gain, red_gain, blue_gain], dtype=np.float64),
             pp_cases=np.array(cases, dtype=np.int32), pp_ref64=torch.stack(r64s).numpy(),
             pp_ref32=torch.stack(r32s).numpy(), pp_err=np.array(errs, dtype=np.float64))

    # ---- samplers
    seeds = [(1, 2), (20264, 7), (3, 3)]
    sm_ccm, sm_gains, sm_noise = [], [], []
    for ps, ts in seeds:
        random.seed(ps)
        torch.manual_seed(ts)
        sm_ccm.append(cp.random_ccm().numpy())
        sm_gains.append(cp.random_gains())
        sm_noise.append(cp.random_noise_levels())
    d.update(sm_seeds=np.array(seeds, dtype=np.int64), sm_ccm=np.stack(sm_ccm),
             sm_gains=np.array(sm_gains, dtype=np.float64), sm_noise=np.array(sm_noise, dtype=np.float64))

    path = os.path.join(HERE, 'synth.npz')
    np.savez_compressed(path, **d)
    print('wrote', path, os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
