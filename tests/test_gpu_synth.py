"""GPU tests of the synthetic-data kernels (csrc/synth_ops.hip) and of dbsr_amd.synthetic on top of them.

The warp is held to a torch restatement of its definition (include/dbsr_hip.h: explicit index gathers, taps outside
the image contribute 0) evaluated in float64; the same function evaluated in float32 gives the yardstick: the kernel
may be off the float64 result by at most twice what the float32 restatement is, on the same inputs.  The pointwise
kernels are held to twice the reference's own float32 error stored in tests/golden/synth.npz.  Every bar is printed
next to the measured error.
"""
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.fixture(scope='module')
def g(golden):
    return golden('synth')


@pytest.fixture(scope='module')
def S():
    from dbsr_amd import synthetic
    return synthetic


@pytest.fixture(scope='module')
def ops():
    from dbsr_amd import ops
    return ops


# ------------------------------------------------------------------------------------------ the restatement

def _bil(P, x, y):
    """bil(P, (x, y)) for planes P [C,H,W] at positions x, y (any common shape): (value [C, ...], any tap outside)."""
    H, W = P.shape[-2:]
    x0, y0 = torch.floor(x), torch.floor(y)
    fx, fy = x - x0, y - y0
    xi, yi = x0.long(), y0.long()
    s = torch.zeros((P.shape[0],) + tuple(x.shape), dtype=P.dtype)
    outside = torch.zeros(x.shape, dtype=torch.bool)
    for (dy, dx), w in (((0, 0), (1.0 - fx) * (1.0 - fy)), ((0, 1), fx * (1.0 - fy)), ((1, 0), (1.0 - fx) * fy),
                        ((1, 1), fx * fy)):
        xx, yy = xi + dx, yi + dy
        ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        v = P[:, yy.clamp(0, H - 1), xx.clamp(0, W - 1)] * ok.to(P.dtype)
        s = s + w * v
        outside |= ~ok
    return s, outside


def warp_restatement(lin, ainv, bc, f, dtype):
    """rgb [B,N,3,H2,W2], flow [B,N,2,H2,W2] and `outside` [B,N,H2,W2] (some tap of the pixel fell outside the
    image) of the definition, as CPU torch ops in `dtype` (ainv is rounded to float32 first: what the kernel gets)."""
    lin, ainv = lin.to(dtype), ainv.float().to(dtype)
    B, N = ainv.shape[:2]
    Hc, Wc = lin.shape[-2:]
    H2, W2 = (Hc - 2 * bc) // f, (Wc - 2 * bc) // f
    taps = [f // 2 - 1, f // 2] if f % 2 == 0 else [(f - 1) // 2]
    Y, X = torch.meshgrid(torch.arange(H2), torch.arange(W2), indexing='ij')
    rgb = torch.zeros(B, N, 3, H2, W2, dtype=dtype)
    flow = torch.zeros(B, N, 2, H2, W2, dtype=dtype)
    outside = torch.zeros(B, N, H2, W2, dtype=torch.bool)
    fc = 0.5 * (f - 1)
    for b in range(B):
        for n in range(N):
            a = ainv[b, n]
            acc = torch.zeros(3, H2, W2, dtype=dtype)
            for j in taps:
                for i in taps:
                    px, py = (bc + f * X + i).to(dtype), (bc + f * Y + j).to(dtype)
                    sx = a[0, 0] * px + a[0, 1] * py + a[0, 2]
                    sy = a[1, 0] * px + a[1, 1] * py + a[1, 2]
                    v, out = _bil(lin[b], sx, sy)
                    acc = acc + v
                    outside[b, n] |= out
            rgb[b, n] = acc * (1.0 / len(taps) ** 2)
            d = a - ainv[b, 0]
            px, py = (bc + f * X).to(dtype) + fc, (bc + f * Y).to(dtype) + fc
            flow[b, n, 0] = (d[0, 0] * px + d[0, 1] * py + d[0, 2]) / f
            flow[b, n, 1] = (d[1, 0] * px + d[1, 1] * py + d[1, 2]) / f
    return rgb, flow, outside


def mosaic_noise(S, rgb, levels, z):
    raw = S.mosaic(rgb)
    if z is None:
        return raw.clamp(0.0, 1.0)
    shot = levels[:, 0].view(-1, 1, 1, 1, 1).to(rgb.dtype)
    read = levels[:, 1].view(-1, 1, 1, 1, 1).to(rgb.dtype)
    return (raw + z.to(rgb.dtype) * (raw * shot + read).sqrt()).clamp(0.0, 1.0)


TRANSFORMS = [[(5.5, -3.25, 8.0), (-6.0, 4.75, -5.0)], [(2.0, 6.0, -8.0), (-4.5, -5.5, 3.0)]]     # (tx, ty, degrees)


def _ainv(S, Hc, Wc, f):
    shift = f / 2.0 - 0.5
    out = []
    for frames in TRANSFORMS:
        mats = [S.get_tmat((Hc, Wc), (shift, shift), 0.0, (0.0, 0.0), (1.0, 1.0))]
        mats += [S.get_tmat((Hc, Wc), (tx, ty), th, (0.0, 0.0), (1.0, 1.0)) for tx, ty, th in frames]
        out.append(np.stack([S.inverse_tmat(m) for m in mats]))
    return torch.from_numpy(np.stack(out)).float()


@pytest.fixture(scope='module')
def lin_image():
    gen = torch.Generator().manual_seed(20265)
    return torch.rand(2, 3, 48, 64, generator=gen)


def _max_err(a, b):
    return (a.double().cpu() - b.double()).abs().max().item()


@pytest.mark.parametrize('f,Hc,Wc', [(4, 48, 64), (1, 48, 64), (2, 48, 64), (3, 44, 62)])
def test_warp_matches_restatement(S, ops, lin_image, f, Hc, Wc):
    bc = 4
    lin = lin_image[..., :Hc, :Wc].contiguous()
    ainv = _ainv(S, Hc, Wc, f)
    B, N = ainv.shape[:2]
    H2, W2 = (Hc - 2 * bc) // f, (Wc - 2 * bc) // f
    assert H2 % 2 == 0 and W2 % 2 == 0
    if f == 4:
        assert (H2 // 2, W2 // 2) == (5, 7)                       # odd, non-square RAW planes
    gen = torch.Generator().manual_seed(7)
    z = torch.randn(B, N, 4, H2 // 2, W2 // 2, generator=gen)
    levels = torch.tensor([[0.004, 1e-5], [0.01, 1e-4]])
    rgb64, flow64, outside = warp_restatement(lin, ainv, bc, f, torch.float64)
    rgb32, flow32, _ = warp_restatement(lin, ainv, bc, f, torch.float32)
    raw64, raw32 = mosaic_noise(S, rgb64, levels, z), mosaic_noise(S, rgb32, levels, z)
    share = S.mosaic(outside.unsqueeze(2).expand(-1, -1, 3, -1, -1).float()).mean().item()
    print('f %d: share of RAW elements with an outside tap %.3f' % (f, share))
    assert 0.01 <= share <= 0.5, share
    assert not outside[:, 0].any()                                # the base frame stays inside the border

    burst, rgb, flow = ops.burst_synth(lin.to(DEV), ainv.to(DEV), bc, f, levels.to(DEV), z.to(DEV))
    assert burst.shape == (B, N, 4, H2 // 2, W2 // 2) and rgb.shape == (B, N, 3, H2, W2)
    assert flow.shape == (B, N, 2, H2, W2)
    for name, out, r64, r32 in (('rgb', rgb, rgb64, rgb32), ('burst', burst, raw64, raw32),
                                ('flow', flow, flow64, flow32)):
        bar, err = 2 * _max_err(r32, r64), _max_err(out, r64)
        print('f %d %s: max |hip - ref64| %.3e, bar 2 x %.3e' % (f, name, err, bar / 2))
        assert bar > 0 and err <= bar, (name, err, bar)
    assert torch.equal(flow[:, 0], torch.zeros_like(flow[:, 0]))            # flow to the base frame: exactly 0

    burst_only, none_rgb, none_flow = ops.burst_synth(lin.to(DEV), ainv.to(DEV), bc, f, levels.to(DEV), z.to(DEV),
                                                      want_rgb=False, want_flow=False)
    assert none_rgb is None and none_flow is None
    assert torch.equal(burst_only, burst)                                   # one-channel sampling: bitwise the same
    clean, rgb2, _ = ops.burst_synth(lin.to(DEV), ainv.to(DEV), bc, f)     # null z: no noise
    assert torch.equal(rgb2, rgb)
    assert torch.equal(clean, S.mosaic(rgb))


def test_warp_closed_forms(S, ops, lin_image):
    """Frame 0 at f = 4 is the separable [1/4, 1/2, 1/4] average around (bc + 4X, bc + 4Y): its centring shift 1.5
    puts the two taps per axis at -0.5 and +0.5.  A frame translated by (tx, ty) = (4, -8) on top of that shift,
    without rotation, has the constant flow -(tx, ty) / f and equals frame 0 moved by (tx, ty) / f pixels."""
    bc, f, Hc, Wc = 4, 4, 48, 64
    lin = lin_image[:1]
    tx, ty = 4.0, -8.0
    mats = [S.get_tmat((Hc, Wc), (1.5, 1.5), 0.0, (0.0, 0.0), (1.0, 1.0)),
            S.get_tmat((Hc, Wc), (1.5 + tx, 1.5 + ty), 0.0, (0.0, 0.0), (1.0, 1.0))]
    ainv = torch.from_numpy(np.stack([S.inverse_tmat(m) for m in mats])).float()[None]
    _, rgb, flow = ops.burst_synth(lin.to(DEV), ainv.to(DEV), bc, f)
    rgb, flow = rgb.cpu(), flow.cpu()
    H2, W2 = 10, 14
    k = torch.tensor([0.25, 0.5, 0.25], dtype=torch.float64)
    L = lin[0].double()
    want = torch.zeros(3, H2, W2, dtype=torch.float64)
    for j in range(3):
        for i in range(3):
            want += k[j] * k[i] * L[:, bc - 1 + j:bc - 1 + j + 4 * H2:4, bc - 1 + i:bc - 1 + i + 4 * W2:4]
    # a convex combination of 16 values in [0, 1]: 16 products and 19 sums, each rounded once at <= 2^-24
    bar = 35 * 2.0 ** -24
    err = _max_err(rgb[0, 0], want)
    print('frame 0 vs the [1/4, 1/2, 1/4] average: %.3e, bar %.3e' % (err, bar))
    assert err <= bar
    assert torch.equal(flow[0, 0], torch.zeros(2, H2, W2))
    # single2lrburst: (sample_pos_inv_n - sample_pos_inv_0) / f = -(tx, ty) / f everywhere
    assert torch.equal(flow[0, 1, 0], torch.full((H2, W2), -tx / f))
    assert torch.equal(flow[0, 1, 1], torch.full((H2, W2), -ty / f))
    sx, sy = int(tx) // f, int(ty) // f                               # frame 1 [Y, X] = frame 0 [Y - sy, X - sx]
    assert torch.equal(rgb[0, 1, :, :H2 + sy, sx:], rgb[0, 0, :, -sy:, :W2 - sx])


# ------------------------------------------------------------------------------------------ pointwise kernels

UN_SETS = {'a': (True, True, False), 'b': (True, False, False), 'c': (False, True, False), 'd': (False, False, True)}


def _un_params(S, g, ss, gm, ident):
    mats = [torch.eye(3) if ident else torch.from_numpy(g['un_rgb2cam'][b]) for b in range(2)]
    gains = [(1.0, 1.0, 1.0) if ident else tuple(float(v) for v in g['un_gains'][b]) for b in range(2)]
    return S._pack_params(mats, [x[0] for x in gains], [x[1] for x in gains], [x[2] for x in gains], [ss] * 2,
                          [gm] * 2)


@pytest.mark.parametrize('tag', sorted(UN_SETS))
def test_unprocess_matches_reference(S, ops, g, tag):
    ss, gm, ident = UN_SETS[tag]
    params = _un_params(S, g, ss, gm, ident).to(DEV)
    u8 = torch.from_numpy(g['un_img_u8'])
    lin = ops.unprocess_rgb(u8.to(DEV), params)
    f32 = (u8.permute(0, 3, 1, 2).float() / 255.0).contiguous()             # divided on the host: IEEE division
    lin_f = ops.unprocess_rgb(f32.to(DEV), params)
    assert torch.equal(lin, lin_f)                                           # uint8 HWC == float NCHW, bitwise
    err, bar = _max_err(lin, torch.from_numpy(g['un_%s_ref64' % tag])), 2 * float(g['un_%s_err' % tag])
    print('unprocess %s: max |hip - ref64| %.3e, bar 2 x %.3e' % (tag, err, bar / 2))
    assert err <= bar
    # rows that do not allow 16-byte accesses (width 37, an odd offset): the scalar path, same values
    sub = f32[:, :, 1:, 3:].contiguous()
    assert torch.equal(ops.unprocess_rgb(sub.to(DEV), params), lin[:, :, 1:, 3:])
    sub8 = u8[:, 1:, 3:, :].contiguous()
    assert torch.equal(ops.unprocess_rgb(sub8.to(DEV), params), lin[:, :, 1:, 3:])


def test_noise_matches_reference(S, ops, g):
    """ns_rgb's three frames as three images with the identity transform at f = 1 (the warp is then exact: every
    position is an integer), the fixture's normals and levels."""
    rgb = torch.from_numpy(g['ns_rgb'])                                      # [3,3,12,20]
    ainv = torch.tensor([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]).expand(3, 1, 2, 3).contiguous()
    levels = torch.from_numpy(g['ns_levels']).float().expand(3, 2).contiguous()
    z = torch.from_numpy(g['ns_z']).unsqueeze(1)
    burst, brgb, _ = ops.burst_synth(rgb.to(DEV), ainv.to(DEV), 0, 1, levels.to(DEV), z.to(DEV))
    assert torch.equal(brgb[:, 0].cpu(), rgb)
    err, bar = _max_err(burst[:, 0], torch.from_numpy(g['ns_ref64'])), 2 * float(g['ns_err'])
    print('noise: max |hip - ref64| %.3e, bar 2 x %.3e' % (err, bar / 2))
    assert err <= bar
    clean, brgb2, _ = ops.burst_synth(rgb.to(DEV), ainv.to(DEV), 0, 1)
    assert torch.equal(clean, S.mosaic(brgb2))
    assert torch.equal(clean[:, 0].cpu(), torch.from_numpy(g['ns_mosaic']))


def test_postprocess_matches_reference(S, ops, g):
    img = torch.from_numpy(g['pp_img']).to(DEV)
    rgb, red, blue = (float(v) for v in g['pp_gains'])
    for i, (ga, cc, gm, ss, mg, ms) in enumerate(g['pp_cases'].tolist()):
        meta = {'cam2rgb': torch.from_numpy(g['pp_cam2rgb']), 'rgb_gain': rgb, 'red_gain': red, 'blue_gain': blue,
                'gamma': bool(mg), 'smoothstep': bool(ms)}
        kw = dict(gains=bool(ga), ccm=bool(cc), gamma=bool(gm), smoothstep=bool(ss))
        out = S.process_linear_image_rgb(img, meta, **kw)
        assert out.is_cuda and out.shape == img.shape
        ref64, e = g['pp_ref64'][i], float(g['pp_err'][i])
        err = _max_err(out, torch.from_numpy(ref64))
        print('postprocess %d: max |hip - ref64| %.3e, bar 2 x %.3e' % (i, err, e))
        assert err <= 2 * e
        u8 = S.process_linear_image_rgb(img, meta, return_np=True, **kw)
        assert u8.dtype == np.uint8 and u8.shape == (24, 40, 3)
        v = ref64.transpose(1, 2, 0) * 255
        near = np.abs(v - np.round(v)) <= 255 * 2 * e
        assert near.mean() <= 0.01
        assert np.array_equal(u8[~near], np.floor(v[~near]).astype(np.uint8))
        assert (np.abs(u8.astype(np.int32) - np.floor(v).astype(np.int32)) <= 1).all()
        # both outputs of one launch equal the separate ones; an odd width takes the scalar path
        p = S._pack_params([meta['cam2rgb']], [rgb], [red], [blue], [bool(ms)], [bool(mg)]).to(DEV)
        o2, u2 = ops.postprocess_rgb(img[None], p, *(bool(x) for x in (ga, cc, gm, ss)), want_f32=True, want_u8=True)
        assert torch.equal(o2[0], out) and np.array_equal(u2[0].cpu().numpy(), u8)
        o3, u3 = ops.postprocess_rgb(img[None, :, 1:, 3:].contiguous(), p, *(bool(x) for x in (ga, cc, gm, ss)),
                                     want_f32=True, want_u8=True)
        assert torch.equal(o3[0], out[:, 1:, 3:]) and np.array_equal(u3[0].cpu().numpy(), u8[1:, 3:])


# ------------------------------------------------------------------------------------------ end to end

def _srgb_image():
    """A seeded 8-bit 440 x 440 image with few highlights, no value below 20 and moderate colour: smooth luminance
    plus a small per-channel variation."""
    gen = torch.Generator().manual_seed(20266)
    lum = torch.nn.functional.interpolate(torch.rand(1, 1, 12, 12, generator=gen), size=(440, 440), mode='bicubic',
                                          align_corners=False)[0, 0]
    lum = 30.0 + 190.0 * lum.clamp(0.0, 1.0)
    img = lum[:, :, None] + 24.0 * (torch.rand(440, 440, 3, generator=gen) - 0.5)
    img[100:140, 200:260] = 246.0 + 9.0 * torch.rand(40, 60, 3, generator=gen)       # the few highlights
    return img.clamp(20.0, 255.0).round().to(torch.uint8)


def _trainer(synth_sd):
    import dbsr_amd
    from dbsr_amd.training import DBSRTrainer
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV).set_compute_dtype(torch.bfloat16)
    tr = DBSRTrainer(net, boundary_ignore=40)
    tr.use_graph = False
    return tr


def test_processing_to_training_step(S, synth_sd):
    img = _srgb_image()
    btp = {'max_translation': 24.0, 'max_rotation': 1.0, 'max_shear': 0.0, 'max_scale': 0.0, 'border_crop': 24}
    runs = []
    for _ in range(2):
        random.seed(31)
        torch.manual_seed(31)
        gen = torch.Generator(device=DEV).manual_seed(31)
        proc = S.SyntheticBurstProcessing(384, 4, 4, burst_transformation_params=btp, random_crop=False, device=DEV,
                                          generator=gen)
        d = proc([img.numpy()])
        assert d['burst'].shape == (1, 4, 4, 48, 48) and d['frame_gt'].shape == (1, 3, 384, 384)
        assert d['burst'].is_cuda and d['frame_gt'].is_contiguous()
        loss = _trainer(synth_sd).step(d['burst'], d['frame_gt'])
        torch.cuda.synchronize()
        assert math.isfinite(float(loss))
        runs.append((d, loss.clone()))
    (d, loss), (d2, loss2) = runs
    assert torch.equal(d['burst'], d2['burst']) and torch.equal(loss, loss2)
    assert torch.equal(d['meta_info']['rgb2cam'], d2['meta_info']['rgb2cam'])

    # the way back: sRGB of frame_gt with the returned meta_info against the input crop
    meta = d['meta_info']
    crop = img[4:436, 4:436].permute(2, 0, 1).float() / 255.0                 # the centre crop, padded by the border
    x = crop[:, 24:-24, 24:-24]
    back = S.SimplePostProcess().process(d['frame_gt'], meta)
    m1 = {k: (v[0] if torch.is_tensor(v) else v) for k, v in meta.items()}
    gains = tuple(float(m1[k]) for k in ('rgb_gain', 'red_gain', 'blue_gain'))
    mid = S.apply_ccm(S.gamma_expansion(S.invert_smoothstep(crop)), m1['rgb2cam'])
    mask = (mid.mean(dim=0) - 0.9).clamp(0.0)[24:-24, 24:-24] > 0
    lin_cpu = S.unprocess_rgb_cpu(crop, m1['rgb2cam'], *gains)[:, 24:-24, 24:-24]
    assert (lin_cpu > 0).all()                        # nothing clamped at 0: the only losses are the two below
    excluded = mask | (lin_cpu == 1.0).any(dim=0)
    print('round trip: %.3f of the pixels excluded (clamped at 1 or masked gains)' % excluded.float().mean().item())
    assert excluded.float().mean().item() < 0.2
    back_cpu = S.process_linear_image_rgb(lin_cpu, {**m1, 'rgb_gain': gains[0], 'red_gain': gains[1],
                                                    'blue_gain': gains[2]})
    keep = ~excluded
    bar = 2 * (back_cpu - x)[:, keep].abs().max().item()
    err = (back[0].cpu() - x)[:, keep].abs().max().item()
    print('round trip: max |sRGB back - input| hip %.3e, bar 2 x %.3e (the CPU float32 restatements)' % (err, bar / 2))
    assert bar > 0 and err <= bar
    u8 = S.SimplePostProcess(return_np=True).process(d['frame_gt'], meta)
    assert u8.shape == (1, 384, 384, 3) and u8.dtype == np.uint8


def test_save_visualization_writes_srgb_png(S, synth_sd, tmp_path):
    import dbsr_amd
    from dbsr_amd import evaluation as ev
    random.seed(5)
    torch.manual_seed(5)
    btp = {'max_translation': 3.0, 'max_rotation': 1.0, 'border_crop': 4}
    proc = S.SyntheticBurstProcessing((192, 256), 3, 4, burst_transformation_params=btp, random_crop=True, device=DEV)
    d = proc([_srgb_image().numpy()])
    assert d['burst'].shape == (1, 3, 4, 24, 32) and d['frame_gt'].shape == (1, 3, 192, 256)
    meta = {k: (v[0] if torch.is_tensor(v) else v) for k, v in d['meta_info'].items()}
    meta['burst_name'] = 'sample'
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV).eval()
    paths = ev.save_visualization(net, [(d['burst'][0].cpu(), d['frame_gt'][0].cpu(), meta)], str(tmp_path),
                                  device=DEV, save_gt=True)
    assert [p.split('/')[-1] for p in paths] == ['sample.png']
    with torch.no_grad():
        pred, _ = net(d['burst'])
    want = S.SimplePostProcess(return_np=True).process(pred[0].float(), meta)
    got = ev.png_read(paths[0])
    assert got.dtype == np.uint8 and got.shape == (192, 256, 3) and np.array_equal(got, want)
    gt8 = ev.png_read(str(tmp_path / 'sample_gt.png'))
    crop8 = S.SimplePostProcess(return_np=True).process(d['frame_gt'][0], meta)
    assert np.array_equal(gt8, crop8)
