"""Writes tests/golden/lpips_grad.npz: the float64 gradient of LPIPS with respect to pred (torch autograd of the
restatement evaluation.lpips_value on the CPU, which tests/test_lpips_grad_oracle.py pins with finite differences),
and beside it the float32 autograd gradient's own error against it.

Weights and inputs are regenerated from seeds (evaluation.generate_lpips_state_dict(net, seed=WEIGHT_SEED);
`images` below), not stored.

    python tests/golden/make_golden_lpips_grad.py

Per net in (alex, vgg) and case in CASES, keys '<net>_<case>_...':
    value [B]            float64 LPIPS of each image
    grad [B,3,H,W]       float64 d(sum_b value[b]) / d pred, zero in the boundary_ignore frame
    err32 []             max |float32 autograd gradient - grad| / max |grad|
    relu_margin []       min |pre-activation| / its layer's max, over the pred half
    pool_margin []       min (max - runner-up) of a max-pool window / its layer's max, over the pred half's windows
                         whose output is live (> 0)
'plain_seed' is the image seed of the plain case: alex 1x3x41x41, boundary_ignore 4, the first seed from 1 at
which both margins are at least MARGIN.  There no ReLU gate and no arg-max of a device run (whose forward is within
about 3e-6 of a map's maximum of float64) can differ from float64's, so the device gradient is compared with
`grad` itself; every other case goes through the gated reference (evaluation.lpips_backward_reference).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

WEIGHT_SEED = 11
MARGIN = 1e-5
PLAIN_SHAPE, PLAIN_BI = (1, 3, 41, 41), 4
CASES = {'b': dict(shape=(2, 3, 51, 39), boundary_ignore=4, seed=102)}     # 'plain' is added by main()


def images(shape, seed):
    """gt = rand, pred = clamp(gt + 0.25 randn, 0, 1), float32, from numpy PCG64(seed): gt first, then the noise
    (make_golden_lpips.images)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = rng.random(shape, dtype=np.float64).astype(np.float32)
    pred = np.clip(gt + np.float32(0.25) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return pred, gt


def margins(ev, x, weights):
    """(ReLU margin, pool margin) of the float64 forward on prepared images x."""
    import torch
    import torch.nn.functional as F
    spec = ev.LPIPS_NETS[weights['net']]
    shift = torch.tensor(ev.LPIPS_SHIFT, dtype=torch.float32).double().view(1, 3, 1, 1)
    scale = torch.tensor(ev.LPIPS_SCALE, dtype=torch.float32).double().view(1, 3, 1, 1)
    x = (x - shift) / scale
    relu, pool = np.inf, np.inf
    for op in spec['program']:
        if isinstance(op, int):
            _, _, _, s, p = spec['convs'][op]
            pre = F.conv2d(x, weights['conv_w'][op].double(), weights['conv_b'][op].double(), stride=s, padding=p)
            relu = min(relu, float(pre.abs().min() / pre.abs().max()))
            x = F.relu(pre)
        elif op != 'tap':
            k, s = op[1], op[2]
            win = x.unfold(2, k, s).unfold(3, k, s).flatten(4)
            top = win.topk(2, dim=-1).values
            live = top[..., 0] > 0
            if live.any():
                pool = min(pool, float((top[..., 0] - top[..., 1])[live].min() / x.max()))
            x = F.max_pool2d(x, k, s)
    return relu, pool


def gradient(ev, pred, gt, weights, bi, dtype):
    import torch
    p = torch.from_numpy(pred).to(dtype).requires_grad_(True)
    a, g = ev.lpips_prepare(p, torch.from_numpy(gt).to(dtype), bi)
    value = ev.lpips_value(a, g, weights)[0]
    value.sum().backward()
    return value.detach().numpy(), p.grad.numpy()


def main():
    import torch
    from dbsr_amd import evaluation as ev
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = {}
    alex = ev.load_lpips_weights(ev.generate_lpips_state_dict('alex', seed=WEIGHT_SEED), 'alex')
    for seed in range(1, 64):
        pred, gt = images(PLAIN_SHAPE, seed)
        p, _ = ev.lpips_prepare(torch.from_numpy(pred).double(), torch.from_numpy(gt).double(), PLAIN_BI)
        relu, pool = margins(ev, p, alex)
        print('plain alex seed %d: relu margin %.3g, pool margin %.3g' % (seed, relu, pool))
        if relu >= MARGIN and pool >= MARGIN:
            break
    else:
        raise AssertionError('no seed gives the plain case its margins')
    assert relu >= MARGIN and pool >= MARGIN
    out['plain_seed'] = np.array(seed)
    cases = dict(CASES, plain=dict(shape=PLAIN_SHAPE, boundary_ignore=PLAIN_BI, seed=seed))
    for net in ('alex', 'vgg'):
        wts = ev.load_lpips_weights(ev.generate_lpips_state_dict(net, seed=WEIGHT_SEED), net)
        for tag, case in cases.items():
            pred, gt = images(case['shape'], case['seed'])
            bi = case['boundary_ignore']
            v64, g64 = gradient(ev, pred, gt, wts, bi, torch.float64)
            _, g32 = gradient(ev, pred, gt, wts, bi, torch.float32)
            p, _ = ev.lpips_prepare(torch.from_numpy(pred).double(), torch.from_numpy(gt).double(), bi)
            relu, pool = margins(ev, p, wts)
            pre = '%s_%s_' % (net, tag)
            out[pre + 'value'], out[pre + 'grad'] = v64, g64
            out[pre + 'err32'] = np.array(np.abs(g32.astype(np.float64) - g64).max() / np.abs(g64).max())
            out[pre + 'relu_margin'], out[pre + 'pool_margin'] = np.array(relu), np.array(pool)
            print(pre, 'value', v64, 'max |grad| %.3g' % np.abs(g64).max(), 'err32 %.3g' % out[pre + 'err32'],
                  'relu margin %.3g, pool margin %.3g' % (relu, pool))
    path = os.path.join(HERE, 'lpips_grad.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
