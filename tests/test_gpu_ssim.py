"""SSIM on the HIP kernels (csrc/metrics.hip: dbsr_ssim_forward / dbsr_ssim_backward) against the reference's own
float64 results (tests/golden/ssim.npz) and, at the edge shapes, against the torch restatement
(evaluation.ssim_map, pinned to the reference by test_ssim_oracle.py) run in float64 on the device.

Bounds: the yardstick is how far the reference arithmetic in float32 lands from the same arithmetic in float64
(the fixture's err_map / err_scalar / err_grad; at the edge shapes the restatement's float32 run on the device).
The kernels get twice that: the same arithmetic in another summation order.  Never the code under test."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.fixture(scope='module')
def ops():
    from dbsr_amd import ops
    return ops


def _crop(t, bi):
    return t[..., bi:t.shape[-2] - bi, bi:t.shape[-1] - bi]


def _restate(pred, gt, valid, bi, dtype):
    """The torch restatement on the device in `dtype`: (map, masked mean, d mean / d pred) as float64 CPU tensors."""
    from dbsr_amd import evaluation as ev
    p = pred.to(DEV, dtype).requires_grad_(True)
    smap = ev.ssim_map(_crop(p, bi), _crop(gt.to(DEV, dtype), bi), 1)
    if valid is None:
        v = torch.ones(smap.shape[0], 1, *smap.shape[2:], dtype=dtype, device=DEV)
    else:
        v = _crop(_crop(valid.to(DEV), bi), 5).to(dtype)
    s = (smap * v).sum() / (v.sum() * smap.shape[1] + 1e-12)
    s.backward()
    return smap.detach().double().cpu(), float(s.detach().double()), p.grad.double().cpu()


def _hip(ops, pred, gt, valid, bi):
    """The kernels: (map, result[0], gpred with scale result[1]) as float64 CPU tensors, plus sums."""
    p, g = pred.to(DEV), gt.to(DEV)
    v = None if valid is None else valid.to(DEV)
    result, sums, smap = ops.ssim_forward(p, g, v, bi, 1.0, want_map=True)
    gpred = ops.ssim_backward(p, g, v, bi, 1.0, scale=result[1:])
    torch.cuda.synchronize()
    return smap.double().cpu(), float(result[0]), gpred.double().cpu(), sums.cpu()


def _fixture_inputs(golden, tag):
    g = golden('ssim')
    if tag.startswith('a'):
        a = golden('burstsr')
        return g, torch.from_numpy(a['a_out']), torch.from_numpy(a['a_gt']), torch.from_numpy(a['a_valid'])
    return g, torch.from_numpy(g['b_pred']), torch.from_numpy(g['b_gt']), torch.from_numpy(g['b_valid'])


@pytest.mark.parametrize('tag,bi', [('a40', 40), ('a8', 8), ('b3', 3)])
def test_ssim_vs_reference_fixture(ops, golden, tag, bi):
    """Measured on MI355X (kernel error / the reference's own float32 error, both against its float64 run):
    a40 map 8.3e-05 / 9.7e-04, scalar 1.4e-07 / 3.9e-06, grad 3.8e-08 / 8.0e-07;
    a8  map 1.7e-04 / 1.1e-03, scalar 1.1e-07 / 3.1e-06, grad 3.2e-08 / 7.1e-07;
    b3  map 4.9e-06 / 1.4e-04, scalar 2.0e-08 / 1.5e-06, grad 2.4e-08 / 7.7e-07."""
    g, pred, gt, valid = _fixture_inputs(golden, tag)
    smap, s, gpred, _ = _hip(ops, pred, gt, valid, bi)
    e_m = float((smap - torch.from_numpy(g[tag + '_map64'])).abs().max())
    e_s = abs(s - float(g[tag + '_scalar64']))
    e_g = float((_crop(gpred, bi) - torch.from_numpy(g[tag + '_dpred64'])).abs().max())
    print('%s: map err %.3e (ref %.3e)  scalar err %.3e (ref %.3e)  grad err %.3e (ref %.3e)'
          % (tag, e_m, g[tag + '_err_map'], e_s, g[tag + '_err_scalar'], e_g, g[tag + '_err_grad']))
    assert e_m <= 2 * float(g[tag + '_err_map'])
    assert e_s <= 2 * float(g[tag + '_err_scalar'])
    assert e_g <= 2 * float(g[tag + '_err_grad'])
    outside = gpred.clone()
    _crop(outside, bi).zero_()
    assert float(outside.abs().max()) == 0.0                       # exactly zero outside the crop
    assert torch.isfinite(gpred).all()


# (B, C, H, W, bi, masked): a crop of exactly 11 x 11 (one window); ragged tiles in both directions with C = 1; a
# map one larger than the 32 tile (33 x 33: a 1-wide second tile row and column); C = 4
EDGE = [(1, 3, 17, 17, 3, False), (1, 1, 75, 90, 0, True), (2, 3, 43, 43, 0, True), (1, 4, 40, 52, 1, True)]


@functools.lru_cache(maxsize=None)
def _edge_case(shape):
    """Seeded smooth images plus noise (where E[x^2] - mu^2 cancels, as on real images) and the restatement's
    float64 and float32 results.  The seed is the first of 0, 1, ... at which the float32 restatement's scalar is
    off its float64 one by more than one float32 ulp of the value: below that the yardstick would be finer than
    the format the kernel stores its result in."""
    B, C, H, W, bi, masked = shape
    for seed in range(8):
        gen = torch.Generator().manual_seed(1000 * H + W + seed)
        gt = F.avg_pool2d(torch.rand(B, C, H + 4, W + 4, generator=gen), 5, 1)
        pred = (gt + 0.02 * torch.randn(gt.shape, generator=gen)).clamp(0.0, 1.0)
        valid = (torch.rand(B, 1, H, W, generator=gen) > 0.4) if masked else None
        m64, s64, g64 = _restate(pred, gt, valid, bi, torch.float64)
        m32, s32, g32 = _restate(pred, gt, valid, bi, torch.float32)
        if abs(s32 - s64) > 2.0 ** -23 * abs(s64):
            break
    else:
        raise AssertionError('no seed gives a usable yardstick')
    errs = (float((m32 - m64).abs().max()), abs(s32 - s64), float((g32 - g64).abs().max()))
    return pred, gt, valid, (m64, s64, g64), errs


@pytest.mark.parametrize('shape', EDGE, ids=lambda s: 'x'.join(str(v) for v in s[:5]))
def test_ssim_edge_shapes_vs_restatement(ops, shape):
    bi = shape[4]
    pred, gt, valid, (m64, s64, g64), (err_m, err_s, err_g) = _edge_case(shape)
    smap, s, gpred, _ = _hip(ops, pred, gt, valid, bi)
    assert smap.shape == m64.shape == (shape[0], shape[1], shape[2] - 2 * bi - 10, shape[3] - 2 * bi - 10)
    e_m, e_s, e_g = float((smap - m64).abs().max()), abs(s - s64), float((gpred - g64).abs().max())
    print('%s: map err %.3e (fp32 restatement %.3e)  scalar err %.3e (%.3e)  grad err %.3e (%.3e)'
          % (shape, e_m, err_m, e_s, err_s, e_g, err_g))
    assert e_m <= 2 * err_m
    assert e_s <= 2 * err_s
    assert e_g <= 2 * err_g
    outside = gpred.clone()
    _crop(outside, bi).zero_()
    assert float(outside.abs().max()) == 0.0


def test_ssim_bitwise_reproducible(ops, golden):
    _, pred, gt, valid = _fixture_inputs(golden, 'a8')
    p, g, v = pred.to(DEV), gt.to(DEV), valid.to(DEV)
    runs = []
    for _ in range(2):
        result, sums, smap = ops.ssim_forward(p, g, v, 8, 1.0, want_map=True)
        runs.append((result, sums, smap, ops.ssim_backward(p, g, v, 8, 1.0, scale=result[1:])))
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_ssim_mask_semantics(ops, golden):
    """valid None == all ones; all zeros -> 0 and a zero gradient; per-image sums; one masked window."""
    g, pred, gt, valid = _fixture_inputs(golden, 'b3')
    p, q, v = pred.to(DEV), gt.to(DEV), valid.to(DEV)
    bi = 3
    r_none, s_none, _ = ops.ssim_forward(p, q, None, bi)
    r_ones, s_ones, _ = ops.ssim_forward(p, q, torch.ones_like(v), bi)
    assert torch.equal(r_none, r_ones) and torch.equal(s_none, s_ones)
    assert torch.equal(ops.ssim_backward(p, q, None, bi, scale=r_none[1:]),
                       ops.ssim_backward(p, q, torch.ones_like(v), bi, scale=r_ones[1:]))
    assert float(s_none[0, 1]) == (29 - 6 - 10) * (37 - 6 - 10)            # the count: every window of one channel

    r_zero, s_zero, _ = ops.ssim_forward(p, q, torch.zeros_like(v), bi)
    assert float(r_zero[0]) == 0.0 and float(s_zero.abs().max()) == 0.0
    gz = ops.ssim_backward(p, q, torch.zeros_like(v), bi, scale=r_zero[1:])
    assert torch.isfinite(gz).all() and float(gz.abs().max()) == 0.0

    result, sums, smap = ops.ssim_forward(p, q, v, bi, want_map=True)
    for b in range(2):
        _, s1, _ = ops.ssim_forward(p[b:b + 1], q[b:b + 1], v[b:b + 1], bi)
        assert torch.equal(s1[0], sums[b])
    assert float(sums[:, 1].sum()) == float(_crop(_crop(v, bi), 5).sum())

    # mask one valid window of image 1 (map position (y, x); its centre is pixel (bi + 5 + y, bi + 5 + x))
    ys, xs = torch.nonzero(_crop(_crop(v, bi), 5)[1, 0], as_tuple=True)
    y, x = int(ys[len(ys) // 2]), int(xs[len(xs) // 2])
    v2 = v.clone()
    v2[1, 0, bi + 5 + y, bi + 5 + x] = False
    _, sums2, _ = ops.ssim_forward(p, q, v2, bi)
    assert torch.equal(sums2[0], sums[0]) and float(sums[1, 1] - sums2[1, 1]) == 1.0
    gone = float(smap[1, :, y, x].double().sum())
    # both sums are float32 trees over <= 1024 terms per block: allow 16 ulp of the sum's magnitude
    assert abs(float(sums[1, 0].double() - sums2[1, 0].double()) - gone) <= 16 * 2.0 ** -23 * float(sums[1, 0])
    one = torch.ones(1, device=DEV)
    g1, g2 = ops.ssim_backward(p, q, v, bi, scale=one), ops.ssim_backward(p, q, v2, bi, scale=one)
    changed = g1 != g2
    assert bool(changed[1].any()) and not bool(changed[0].any())
    support = torch.zeros_like(changed)
    support[1, :, bi + y:bi + y + 11, bi + x:bi + x + 11] = True           # the masked window's 11 x 11 pixels
    assert not bool((changed & ~support).any())                            # nothing else moved, bit for bit


def test_ssim_module_autograd(ops, golden):
    from dbsr_amd import burstsr
    from dbsr_amd import evaluation as ev
    g, pred, gt, valid = _fixture_inputs(golden, 'b3')
    q, v = gt.to(DEV), valid.to(DEV)
    result, _, _ = ops.ssim_forward(pred.to(DEV), q, v, 3)
    p = pred.to(DEV).requires_grad_(True)
    loss = ev.SSIM(boundary_ignore=3, use_for_loss=True)(p, q, v)
    loss.backward()
    assert torch.equal(p.grad, ops.ssim_backward(pred.to(DEV), q, v, 3, scale=-result[1:]))
    assert float(loss.detach()) == float(1.0 - result[0])
    value = burstsr.SSIM(boundary_ignore=3, use_for_loss=False, val_range=1.0)(pred.to(DEV), q, v)
    assert torch.equal(value, result[0])
    # 3-dim inputs, no mask, no crop: as the CPU restatement within twice its own float32 error
    fn = ev.SSIM(boundary_ignore=None, use_for_loss=False)
    dev, cpu = float(fn(pred[0].to(DEV), q[0])), float(fn(pred[0], gt[0]))
    ref = float(fn(pred[0].double(), gt[0].double()))
    print('3-dim: hip %.8f cpu fp32 %.8f fp64 %.8f' % (dev, cpu, ref))
    assert abs(dev - ref) <= 2 * max(abs(cpu - ref), 2.0 ** -23 * ref)


def test_compute_score_burstsr_reports_ssim(tmp_path, synth_sd, monkeypatch):
    """The BurstSR scorer's SSIM column: per image, the CPU restatement applied to the very aligned outputs and
    masks the scorer produced, within twice the restatement's own float32 error; the PSNR column is unchanged."""
    import dbsr_amd
    from dbsr_amd import burstsr as bs
    from dbsr_amd import evaluation as ev
    from dbsr_amd.burst import synthetic_bursts
    from dbsr_amd.pwcnet import PWCNet
    from tests.test_burstsr import _meta_canon, _meta_samsung
    bursts, gts = synthetic_bursts(2, 14, 40, 40, sr_factor=8, seed=21)
    exp_scale = ((1 / 50) * 200 / 1.7 ** 2) / ((1 / 100) * 100 / 4.0 ** 2)     # the two metas' light factors
    for b in range(2):
        fr = (bursts[b].numpy() * 1023 + 64).round().clip(0, 65535).astype(np.uint16)
        gt = (gts[b].numpy() * 16383 / exp_scale + 512).round().clip(0, 65535).astype(np.uint16)
        bs.write_burstsr_sample(str(tmp_path), '00%02d_0000' % b, fr, gt, _meta_samsung(), _meta_canon())
    ds = bs.BurstSRDataset(str(tmp_path), processing=bs.BurstSRProcessing(crop_sz=40))
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    net = net.to(DEV).set_compute_dtype(torch.float32)
    pre = 'encoder.alignment_net.'
    pwc = PWCNet(load_pretrained=False)
    pwc.load_state_dict({k[len(pre):]: v for k, v in synth_sd.items() if k.startswith(pre)})

    seen = []
    sca_forward = bs.SpatialColorAlignment.forward

    def recording(self, pred, gt, burst):
        out, valid = sca_forward(self, pred, gt, burst)
        seen.append((out.detach().cpu(), gt.cpu(), valid.cpu()))
        return out, valid
    monkeypatch.setattr(bs.SpatialColorAlignment, 'forward', recording)
    res = bs.compute_score_burstsr(net, ds, pwc.to(DEV))
    assert len(seen) == 2 and sorted(res['per_image_ssim']) == sorted(res['per_image'])
    ssim_fn, psnr_fn = ev.SSIM(boundary_ignore=40, use_for_loss=False), ev.PSNR(boundary_ignore=40)
    vals = []
    for i, (out, gt, valid) in enumerate(seen):
        name = ds[i][2]['burst_name']
        s64 = float(ssim_fn(out.double(), gt.double(), valid=valid))
        s32 = float(ssim_fn(out, gt, valid=valid))
        mine = res['per_image_ssim'][name]
        print('%s: ssim hip %.8f  cpu fp32 %.8f  fp64 %.8f  valid %.3f' % (name, mine, s32, s64, valid.float().mean()))
        assert abs(mine - s64) <= 2 * abs(s32 - s64)
        # the PSNR column is the same torch arithmetic as before, on a copy of the same tensors
        assert abs(res['per_image'][name] - float(psnr_fn(out.to(DEV), gt.to(DEV), valid=valid.to(DEV)))) <= 1e-5
        vals.append(mine)
    assert abs(res['ssim'] - sum(vals) / 2) <= 1e-12
