"""Writes tests/golden/lpips.npz: LPIPS in float64 from a numpy-only implementation (sliding windows + einsum, no
torch convolution), so that the fixture is not the package's torch restatement grading itself, and beside it the
float32 restatement's own error against those values (the yardstick of the GPU tests).

The definition is the `lpips` package's published v0.1 code as DESIGN.md ('LPIPS') restates it; the package is
not installed, so this is not a recording of it.  Weights and inputs are regenerated from seeds
(evaluation.generate_lpips_state_dict(net, seed=WEIGHT_SEED); `images` below), not stored.

    python tests/golden/make_golden_lpips.py

Per net in (alex, vgg) and case in CASES, keys '<net>_<case>_...':
    value [B], per_layer [B,5], map0..map4 [B,h,w]       float64
    err32_map [5]       max |float32 restatement map - float64 map| per layer
    err32_value [B]     |float32 restatement value - float64 value|
    gap64 []            max |float64 restatement map - float64 numpy map| over the layers (summation order only)
"""
import os
import sys

import numpy as np
from numpy.lib.stride_tricks import sliding_window_view

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

WEIGHT_SEED = 11
CASES = {'a': dict(shape=(1, 3, 35, 47), boundary_ignore=0, seed=101),
         'b': dict(shape=(2, 3, 51, 39), boundary_ignore=4, seed=102)}


def images(shape, seed):
    """gt = rand, pred = clamp(gt + 0.25 randn, 0, 1), float32, from numpy PCG64(seed): gt first, then the noise."""
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = rng.random(shape, dtype=np.float64).astype(np.float32)
    pred = np.clip(gt + np.float32(0.25) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return pred, gt


def conv(x, w, b, s, p):
    k = w.shape[-1]
    xp = np.pad(x, ((0, 0), (0, 0), (p, p), (p, p)))
    win = sliding_window_view(xp, (k, k), axis=(2, 3))[:, :, ::s, ::s]
    return np.einsum('nchwij,ocij->nohw', win, w, optimize=True) + b[None, :, None, None]


def pool(x, k, s):
    return sliding_window_view(x, (k, k), axis=(2, 3))[:, :, ::s, ::s].max(axis=(-1, -2))


def lpips64(pred, gt, sd, net, spec, boundary_ignore):
    bi = boundary_ignore
    if bi:
        pred, gt = pred[..., bi:-bi, bi:-bi], gt[..., bi:-bi, bi:-bi]
    B = pred.shape[0]
    x = np.concatenate([pred, gt], 0).astype(np.float64)
    shift = np.array([-.030, -.088, -.188], np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    scale = np.array([.458, .448, .450], np.float32).astype(np.float64).reshape(1, 3, 1, 1)
    x = (x - shift) / scale
    taps = []
    for op in spec['program']:
        if isinstance(op, int):
            _, _, _, s, p = spec['convs'][op]
            key = 'net.slice%d.%d' % (spec['slices'][op], spec['features'][op])
            x = np.maximum(conv(x, sd[key + '.weight'].numpy().astype(np.float64),
                                sd[key + '.bias'].numpy().astype(np.float64), s, p), 0.0)
        elif op == 'tap':
            taps.append(x)
        else:
            x = pool(x, op[1], op[2])
    maps = []
    for l, f in enumerate(taps):
        lin = sd['lin%d.model.1.weight' % l].numpy().astype(np.float64).reshape(1, -1, 1, 1)
        n = f / (np.sqrt((f * f).sum(1, keepdims=True)) + 1e-10)
        maps.append((lin * (n[:B] - n[B:]) ** 2).sum(1))
    per_layer = np.stack([m.mean(axis=(1, 2)) for m in maps], 1)
    return per_layer.sum(1), per_layer, maps


def main():
    import torch
    from dbsr_amd import evaluation as ev
    out = {}
    for net in ('alex', 'vgg'):
        sd = ev.generate_lpips_state_dict(net, seed=WEIGHT_SEED)
        wts = ev.load_lpips_weights(sd, net)
        for tag, case in CASES.items():
            pred, gt = images(case['shape'], case['seed'])
            value, per_layer, maps = lpips64(pred, gt, sd, net, ev.LPIPS_NETS[net], case['boundary_ignore'])
            pre = '%s_%s_' % (net, tag)
            out[pre + 'value'], out[pre + 'per_layer'] = value, per_layer
            for l, m in enumerate(maps):
                out[pre + 'map%d' % l] = m
            p, g = ev.lpips_prepare(torch.from_numpy(pred), torch.from_numpy(gt), case['boundary_ignore'])
            v32, _, m32 = ev.lpips_value(p, g, wts)
            v64, _, m64 = ev.lpips_value(p.double(), g.double(), wts)
            out[pre + 'err32_map'] = np.array([np.abs(a.double().numpy() - b).max() for a, b in zip(m32, maps)])
            out[pre + 'err32_value'] = np.abs(v32.double().numpy() - value)
            out[pre + 'gap64'] = np.array(max(np.abs(a.numpy() - b).max() for a, b in zip(m64, maps)))
            ulp = [float(np.spacing(np.float32(b.max()))) for b in maps]
            print(pre, 'value', value, 'err32_map / ulp(max)', out[pre + 'err32_map'] / np.array(ulp),
                  'err32_value', out[pre + 'err32_value'], 'gap64 %.3g' % out[pre + 'gap64'],
                  '|v64 - fixture| %.3g' % np.abs(v64.numpy() - value).max())
    path = os.path.join(HERE, 'lpips.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
