"""CPU checks of the LPIPS restatement (evaluation.lpips_* / LPIPS): against the numpy-only float64 fixture
(tests/golden/make_golden_lpips.py -> tests/golden/lpips.npz), its options against hand-made inputs, the weight
loader's three layouts and its error messages, and the scorers' third column."""
import os

import numpy as np
import pytest
import torch

from dbsr_amd import evaluation as ev

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'lpips.npz')
WEIGHT_SEED = 11                                        # make_golden_lpips.WEIGHT_SEED
CASES = {'a': ((1, 3, 35, 47), 0, 101), 'b': ((2, 3, 51, 39), 4, 102)}     # make_golden_lpips.CASES


def images(shape, seed):
    """make_golden_lpips.images: gt = rand, pred = clamp(gt + 0.25 randn, 0, 1)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = rng.random(shape, dtype=np.float64).astype(np.float32)
    pred = np.clip(gt + np.float32(0.25) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(gt)


@pytest.fixture(scope='module')
def golden():
    return np.load(GOLDEN)


@pytest.fixture(scope='module')
def sds():
    return {net: ev.generate_lpips_state_dict(net, seed=WEIGHT_SEED) for net in ('alex', 'vgg')}


@pytest.mark.parametrize('net', ['alex', 'vgg'])
@pytest.mark.parametrize('case', ['a', 'b'])
def test_float64_restatement_matches_fixture(golden, sds, net, case):
    """The torch restatement in float64 against the numpy sliding-window implementation, to 1e-9 absolute: the two
    differ only in float64 summation order over K <= 4608.  Measured gap on the maps: at most 1.8e-18 (maps up to
    ~3e-2), on the values at most 4.4e-19."""
    shape, bi, seed = CASES[case]
    pred, gt = images(shape, seed)
    w = ev.load_lpips_weights(sds[net], net)
    p, g = ev.lpips_prepare(pred.double(), gt.double(), bi)
    value, per_layer, maps = ev.lpips_value(p, g, w)
    pre = '%s_%s_' % (net, case)
    assert np.abs(value.numpy() - golden[pre + 'value']).max() <= 1e-9
    assert np.abs(per_layer.numpy() - golden[pre + 'per_layer']).max() <= 1e-9
    for l, m in enumerate(maps):
        assert m.shape == golden[pre + 'map%d' % l].shape
        assert np.abs(m.numpy() - golden[pre + 'map%d' % l]).max() <= 1e-9
    mod = ev.LPIPS(boundary_ignore=bi or None, type=net, weights=sds[net], per_image=True)
    assert np.abs(mod(pred.double(), gt.double()).numpy() - golden[pre + 'value']).max() <= 1e-9
    assert 1e-4 < float(value.min()) < 1e-1                # the inputs give a readable value, not a DC-dominated one


@pytest.fixture(scope='module')
def alex(sds):
    return ev.LPIPS(type='alex', weights=sds['alex'])


def test_identical_images_give_exactly_zero(sds):
    x = torch.rand(2, 3, 33, 37, generator=torch.Generator().manual_seed(1))
    for net in ('alex', 'vgg'):
        mod = ev.LPIPS(type=net, weights=sds[net], per_image=True)
        assert torch.equal(mod(x, x.clone()), torch.zeros(2))


def test_options_equal_hand_made_inputs(sds, alex):
    pred, gt = images((2, 3, 45, 41), 5)
    base = lambda p, g: float(alex(p, g))                                           # noqa: E731
    flip = ev.LPIPS(type='alex', weights=sds['alex'], bgr2rgb=True)
    assert float(flip(pred, gt)) == base(pred[:, [2, 1, 0]].contiguous(), gt[:, [2, 1, 0]].contiguous())
    assert float(flip(pred, gt)) != base(pred, gt)
    crop = ev.LPIPS(boundary_ignore=5, type='alex', weights=sds['alex'])
    assert float(crop(pred, gt)) == base(pred[..., 5:-5, 5:-5], gt[..., 5:-5, 5:-5])
    norm = ev.LPIPS(type='alex', weights=sds['alex'], normalize=True)
    assert float(norm(pred, gt)) == base(2 * pred - 1, 2 * gt - 1)
    assert float(norm(pred, gt)) != base(pred, gt)


def test_per_image_valid_and_3dim(sds, alex):
    pred, gt = images((3, 3, 33, 35), 6)
    per = ev.LPIPS(type='alex', weights=sds['alex'], per_image=True)
    v = per(pred, gt)
    assert v.shape == (3,)
    for i in range(3):
        assert float(v[i]) == float(alex(pred[i:i + 1], gt[i:i + 1]))
    assert float(alex(pred, gt)) == float(v.mean())
    assert float(alex(pred, gt, valid=torch.zeros(3, 1, 33, 35))) == float(alex(pred, gt))     # accepted, ignored
    assert float(alex(pred[0], gt[0])) == float(v[0])


def test_differentiable_on_the_cpu(alex):
    pred, gt = images((1, 3, 33, 33), 7)
    pred.requires_grad_(True)
    alex(pred, gt).backward()
    assert pred.grad is not None and float(pred.grad.abs().max()) > 0


@pytest.mark.parametrize('net,side', [('alex', 31), ('vgg', 16)])
def test_smallest_crop(sds, net, side):
    mod = ev.LPIPS(boundary_ignore=2, type=net, weights=sds[net])
    x, y = images((1, 3, side + 4, side + 4), 8)
    assert np.isfinite(float(mod(x, y)))
    with pytest.raises(ValueError, match='smaller than %d x %d' % (side, side)):
        mod(x[..., :-1, :], y[..., :-1, :])
    with pytest.raises(ValueError, match='smaller than %d x %d' % (side, side)):
        mod(x[..., :-1], y[..., :-1])


@pytest.mark.parametrize('net', ['alex', 'vgg'])
def test_loader_layouts_agree(sds, net, tmp_path):
    sd = sds[net]
    spec = ev.LPIPS_NETS[net]
    a = ev.load_lpips_weights(sd, net)
    # (a) with the duplicated heads, the scaling layer, and from a file
    full = dict(sd)
    full.update({'lins.%d.model.1.weight' % l: sd['lin%d.model.1.weight' % l] for l in range(5)})
    full['scaling_layer.shift'] = torch.tensor(ev.LPIPS_SHIFT).view(1, 3, 1, 1)
    full['scaling_layer.scale'] = torch.tensor(ev.LPIPS_SCALE).view(1, 3, 1, 1)
    path = str(tmp_path / 'lpips.pth')
    torch.save(full, path)
    # (b) a torchvision backbone (with its classifier) and the head file
    backbone = {'features.%d.%s' % (fi, kind): sd['net.slice%d.%d.%s' % (sl, fi, kind)]
                for fi, sl in zip(spec['features'], spec['slices']) for kind in ('weight', 'bias')}
    backbone['classifier.1.weight'] = torch.zeros(4, 4)
    heads = {k: v for k, v in sd.items() if k.startswith('lin')}
    # (c) lists
    lists = (a['conv_w'], a['conv_b'], [v.view(1, -1, 1, 1) for v in a['lin']])
    for other in (ev.load_lpips_weights(full, net), ev.load_lpips_weights(path, net),
                  ev.load_lpips_weights(backbone, net, heads=heads), ev.load_lpips_weights(lists, net)):
        for key in ('conv_w', 'conv_b', 'lin'):
            assert len(other[key]) == len(a[key])
            assert all(torch.equal(x, y) for x, y in zip(other[key], a[key]))
    assert [tuple(v.shape) for v in a['lin']] == [(c,) for c in ev.lpips_tap_channels(net)]
    pred, gt = images((1, 3, 33, 33), 9)
    assert float(ev.LPIPS(type=net, weights=(backbone, heads))(pred, gt)) == \
        float(ev.LPIPS(type=net, weights=path)(pred, gt))


def test_loader_names_what_is_wrong(sds):
    sd = dict(sds['alex'])
    del sd['net.slice2.3.bias'], sd['lin4.model.1.weight']
    sd['net.slice9.99.weight'] = torch.zeros(1)
    with pytest.raises(ValueError) as e:
        ev.load_lpips_weights(sd, 'alex')
    msg = str(e.value)
    assert 'missing keys' in msg and 'net.slice2.3.bias' in msg and 'lin4.model.1.weight' in msg
    assert 'unexpected keys' in msg and 'net.slice9.99.weight' in msg
    sd = dict(sds['alex'])
    sd['net.slice3.6.weight'] = torch.zeros(384, 192, 3, 2)
    sd['lin1.model.1.weight'] = torch.zeros(1, 64, 1, 1)
    with pytest.raises(ValueError) as e:
        ev.load_lpips_weights(sd, 'alex')
    msg = str(e.value)
    assert 'net.slice3.6.weight has shape (384, 192, 3, 2), expected (384, 192, 3, 3)' in msg
    assert 'lin1.model.1.weight has shape (1, 64, 1, 1), expected (1, 192, 1, 1)' in msg
    with pytest.raises(ValueError, match='missing keys'):
        ev.load_lpips_weights(sds['vgg'], 'alex')                       # the other net's file
    sd = dict(sds['alex'])
    sd['scaling_layer.shift'] = torch.zeros(1, 3, 1, 1)
    with pytest.raises(ValueError, match='scaling_layer.shift'):
        ev.load_lpips_weights(sd, 'alex')
    with pytest.raises(ValueError, match='expected 5 conv weights'):
        ev.load_lpips_weights(([], [], []), 'alex')
    with pytest.raises(ValueError, match="'alex' or 'vgg'"):
        ev.load_lpips_weights(sds['alex'], 'squeeze')


def test_weights_none_raises():
    with pytest.raises(ValueError, match='No pretrained weights are shipped or downloaded'):
        ev.LPIPS(boundary_ignore=40)


def test_generator_is_seeded_and_heads_non_negative(sds):
    again = ev.generate_lpips_state_dict('alex', seed=WEIGHT_SEED)
    assert list(again) == list(ev.lpips_state_dict_shapes('alex'))
    assert all(torch.equal(again[k], sds['alex'][k]) for k in again)
    other = ev.generate_lpips_state_dict('alex', seed=WEIGHT_SEED + 1)
    assert not torch.equal(other['net.slice1.0.weight'], again['net.slice1.0.weight'])
    assert all(float(again['lin%d.model.1.weight' % l].min()) >= 0 for l in range(5))
    assert all(v.dtype == torch.float32 for v in again.values())


def test_buffers_move_with_the_module(sds):
    mod = ev.LPIPS(type='alex', weights=sds['alex'])
    names = [n for n, _ in mod.named_buffers()]
    assert len(names) == 15 and 'conv0_weight' in names and 'lin4' in names
    assert mod.double().lin0.dtype == torch.float64


# ------------------------------------------------------------------------------------------------- scorers
class _StubNet:
    """Stands in for the SR network: upsamples the first frame's first three planes by 8."""

    def __call__(self, burst):
        x = burst[:, 0, :3]
        return torch.nn.functional.interpolate(x, scale_factor=8, mode='bilinear', align_corners=False), {}


class _Bursts(torch.utils.data.Dataset):
    def __init__(self, n=3):
        g = torch.Generator().manual_seed(3)
        self.items = [(torch.rand(2, 4, 6, 6, generator=g), torch.rand(3, 48, 48, generator=g)) for _ in range(n)]

    def __len__(self):
        return len(self.items)

    def __getitem__(self, i):
        return self.items[i][0], self.items[i][1], {'burst_name': '%04d' % i}


def test_compute_score_third_column(sds):
    ds = _Bursts()
    base = ev.compute_score(_StubNet(), ds, boundary_ignore=4, device='cpu', batch=2)
    assert sorted(base) == ['per_image', 'per_image_ssim', 'psnr', 'ssim']          # what it returns today
    lp = ev.LPIPS(boundary_ignore=4, type='alex', weights=sds['alex'])
    for metrics in (('psnr', 'ssim'), ('psnr', 'ssim', 'lpips')):
        res = ev.compute_score(_StubNet(), ds, boundary_ignore=4, device='cpu', batch=2, metrics=metrics, lpips=lp)
        assert {k: res[k] for k in base} == base
        assert sorted(res['per_image_lpips']) == ['0000', '0001', '0002']
        assert res['lpips'] == sum(res['per_image_lpips'].values()) / 3
        pred = ev.quantize_prediction(_StubNet()(ds[1][0].unsqueeze(0))[0])
        assert res['per_image_lpips']['0001'] == float(lp(pred, ds[1][1].unsqueeze(0)))
    with pytest.raises(ValueError, match='unknown metrics'):
        ev.compute_score(_StubNet(), ds, boundary_ignore=4, device='cpu', metrics=('lpips',))
    with pytest.raises(ValueError, match='boundary_ignore'):
        ev.compute_score(_StubNet(), ds, boundary_ignore=8, device='cpu', lpips=lp)


def test_compute_score_burstsr_third_column(sds, monkeypatch):
    from dbsr_amd import burstsr

    class _Sca:                                          # the alignment, stubbed: identity and an all-valid mask
        def __init__(self, alignment_net, sr_factor=4):
            pass

        def __call__(self, pred, gt, burst):
            return pred, torch.ones(pred.shape[0], 1, *pred.shape[-2:], dtype=torch.bool)

    monkeypatch.setattr(burstsr, 'SpatialColorAlignment', _Sca)
    ds = _Bursts(2)
    base = burstsr.compute_score_burstsr(_StubNet(), ds, None, boundary_ignore=4, device='cpu')
    assert sorted(base) == ['per_image', 'per_image_ssim', 'psnr', 'ssim']
    lp = ev.LPIPS(boundary_ignore=4, type='alex', weights=sds['alex'])
    res = burstsr.compute_score_burstsr(_StubNet(), ds, None, boundary_ignore=4, device='cpu', lpips=lp)
    assert {k: res[k] for k in base} == base
    pred = ev.quantize_prediction(_StubNet()(ds[0][0].unsqueeze(0))[0])
    assert res['per_image_lpips']['0000'] == float(lp(pred, ds[0][1].unsqueeze(0)))
    assert res['lpips'] == sum(res['per_image_lpips'].values()) / 2
