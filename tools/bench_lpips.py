"""Timing of LPIPS on the HIP device (ops.LPIPSPlan: dbsr_lpips_prep, fp32 dbsr_conv2d, dbsr_maxpool2d,
dbsr_lpips_layer) beside the float32 torch restatement (evaluation.lpips_value) on the host CPU.  The parent of
this feature has no LPIPS at all, so there is no earlier GPU figure to compare with.

Shapes: LPIPS-alex and -vgg at the SyntheticBurst scoring shape 1x3x384x384 and the BurstSR one 1x3x640x640, both
with boundary_ignore 40, and a batch of 8 of the first.  Weights are the seeded stand-ins of
evaluation.generate_lpips_state_dict (timing does not depend on their values); gt = rand, pred = clamp(gt +
0.25 randn, 0, 1).

Per case: median / min / max of `--reps` HIP-event-timed forward calls after `--warmup` calls, on the plan's
preallocated buffers; the CPU restatement's wall time (one call after one warm-up, `--cpu-reps`); and with
`--steps` an event time per launch group of one forward (prep, each conv, each pool, each layer call; these
include the launch gap, a profiler's kernel times do not), from which the layer kernel's bytes/s over its
compulsory traffic 2*B*h*w*C*4 and each conv's FLOP/s follow.  Prints one JSON line.

With `--backward` each timed call is a forward + backward pair (ops.LPIPSPlan.backward: dbsr_lpips_layer_backward,
dbsr_maxpool2d_backward, dbsr_act_backward, the fp32 dbsr_conv2d input gradients, dbsr_lpips_stem_backward), the host
figure is the float32 restatement's forward + autograd backward, and `--steps` lists the backward's launch groups
(the layer backward's rate over its compulsory traffic 3*B*h*w*C*4: both halves read, one written).  The parent
of that feature has no device backward, so again there is no earlier figure.
    timeout -k 10 900 python tools/bench_lpips.py --backward --steps > profiles/lpips_grad_bench.json

Run it under a time limit, e.g.  timeout -k 10 600 python tools/bench_lpips.py --steps > profiles/lpips_bench.json
Usage: python tools/bench_lpips.py [--backward --reps 20 --warmup 3 --cpu-reps 1 --steps --nets alex,vgg --cases 0,2]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbsr_amd import _lib as L                                   # noqa: E402
from dbsr_amd import evaluation as ev                            # noqa: E402
from dbsr_amd import ops                                         # noqa: E402

CASES = [(1, 384, 384, 40), (1, 640, 640, 40), (8, 384, 384, 40)]


def images(shape, seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    gt = rng.random(shape, dtype=np.float64).astype(np.float32)
    pred = np.clip(gt + np.float32(0.25) * rng.standard_normal(shape).astype(np.float32), 0, 1).astype(np.float32)
    return torch.from_numpy(pred), torch.from_numpy(gt)


def event_times(fn, reps, warmup):
    """ms of each of `reps` calls (one HIP event pair per call) after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def step_times(plan, pred, gt, bi, reps):
    """Median event time of each launch group of one forward, with its size-derived rate."""
    plan.forward(pred, gt, bi)
    st = plan._shapes[(pred.shape[0], pred.shape[2], pred.shape[3], bi, False)]
    lib, s = L.lib(), L.stream_ptr(pred.device)
    rows = []
    for kind, a, bufs in st['steps']:
        if kind == 'conv':
            d = a[0]
            fn = lambda a=a: [L.check(lib.dbsr_conv2d(x, s), 'conv') for x in a]                 # noqa: E731
            # one launch per image pair and block of input channels (LPIPSPlan._build): two frames each
            flop = sum(2.0 * 2 * x.out_h * x.out_w * x.cout * x.cin * x.kh * x.kw for x in a)
            row = {'op': 'conv %d->%d k%d s%d' % (sum(x.cin for x in a) // pred.shape[0], d.cout, d.kh, d.stride),
                   'out': [d.out_h, d.out_w], 'launches': len(a), 'kernel': lib.dbsr_conv_kernel_for(d),
                   'variant': lib.dbsr_conv_dispatch_variant(d), 'flop': flop}
        elif kind == 'pool':
            N, h, w, c, k, ps = a
            fn = lambda a=a, bufs=bufs: L.check(lib.dbsr_maxpool2d(a[0], a[1], a[2], a[3], a[4], a[5],  # noqa: E731
                                                                   bufs[0].data_ptr(), a[3], bufs[1].data_ptr(),
                                                                   a[3], s), 'pool')
            row = {'op': 'maxpool k%d s%d C%d' % (k, ps, c), 'in': [h, w],
                   'bytes': 4.0 * c * (N * h * w + bufs[1].numel() // c)}
        else:
            Bn, h, w, c, layer, need = a
            fn = lambda a=a, bufs=bufs: L.check(lib.dbsr_lpips_layer(                            # noqa: E731
                a[0], a[1], a[2], a[3], a[4], bufs[0].data_ptr(), plan.lins[a[4]].data_ptr(), None,
                st['per_layer'].data_ptr(), st['value'].data_ptr(), bufs[1].data_ptr(), a[5], s), 'layer')
            row = {'op': 'lpips_layer %d C%d' % (layer, c), 'in': [h, w], 'bytes': 2.0 * Bn * h * w * c * 4}
        ms = statistics.median(event_times(fn, reps, 2))
        row['ms'] = ms
        if 'flop' in row:
            row['tflops'] = row['flop'] / ms / 1e9
        if 'bytes' in row:
            row['gbytes_per_s'] = row['bytes'] / ms / 1e6
        rows.append(row)
    return rows


def backward_step_times(plan, pred, gt, bi, reps):
    """Median event time of each launch group of one backward, with its size-derived rate."""
    plan.forward(pred, gt, bi)
    plan.backward()
    B = pred.shape[0]
    st = plan._shapes[(B, pred.shape[2], pred.shape[3], bi, False)]
    bw = st['bwd']
    lib, s = L.lib(), L.stream_ptr(pred.device)
    gv = bw['ones']
    rows = []
    for kind, a, bufs in bw['launches']:
        if kind == 'layer':
            _, h, w, c, layer, acc = a
            fn = lambda a=a, bufs=bufs: L.check(lib.dbsr_lpips_layer_backward(                   # noqa: E731
                a[0], a[1], a[2], a[3], bufs[0].data_ptr(), plan.lins[a[4]].data_ptr(), gv.data_ptr(),
                bufs[1].data_ptr(), a[5], s), 'layer backward')
            row = {'op': 'lpips_layer_backward %d C%d%s' % (layer, c, ' +=' if acc else ''), 'in': [h, w],
                   'bytes': (3.0 + acc) * B * h * w * c * 4, 'compulsory_bytes': 3.0 * B * h * w * c * 4}
        elif kind == 'pool':
            _, h, w, c, k, ps = a
            fn = lambda a=a, bufs=bufs: L.check(lib.dbsr_maxpool2d_backward(                     # noqa: E731
                a[0], a[1], a[2], a[3], a[4], a[5], bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(), s),
                'pool backward')
            row = {'op': 'maxpool_backward k%d s%d C%d' % (k, ps, c), 'in': [h, w],
                   'bytes': 4.0 * c * (2 * B * h * w + bufs[1].numel() // c)}
        elif kind == 'gate':
            _, hw, c = a
            fn = lambda a=a, bufs=bufs: L.check(lib.dbsr_act_backward(a[0], a[1], a[2], L.ACT_RELU, bufs[0],  # noqa: E731
                                                                      bufs[1], bufs[0], s), 'gate')
            row = {'op': 'act_backward C%d' % c, 'pixels': hw, 'bytes': 3.0 * B * hw * c * 4}
        elif kind == 'conv':
            d = a[0]
            fn = lambda a=a: [L.check(lib.dbsr_conv2d(x, s), 'dgrad') for x in a]                # noqa: E731
            flop = sum(2.0 * x.out_h * x.out_w * x.cout * x.cin * x.kh * x.kw for x in a)
            row = {'op': 'dgrad %d<-%d k%d' % (d.cout, sum(x.cin for x in a) // B, d.kh), 'out': [d.out_h, d.out_w],
                   'launches': len(a), 'kernel': lib.dbsr_conv_kernel_for(d),
                   'variant': lib.dbsr_conv_dispatch_variant(d), 'flop': flop}
        else:
            _, H, W, sbi, flip, norm = st['args']
            fn = lambda bufs=bufs: L.check(lib.dbsr_lpips_stem_backward(                         # noqa: E731
                B, H, W, sbi, ops.LPIPS_NET_CODE[plan.net], int(flip), int(norm), bufs[0].data_ptr(),
                plan._w32[0].data_ptr(), bw['gpred'].data_ptr(), s), 'stem backward')
            row = {'op': 'lpips_stem_backward', 'in': list(bufs[0].shape[1:3]),
                   'bytes': 4.0 * (bufs[0].numel() + bw['gpred'].numel())}
        ms = statistics.median(event_times(fn, reps, 2))
        row['ms'] = ms
        if 'flop' in row:
            row['tflops'] = row['flop'] / ms / 1e9
        if 'bytes' in row:
            row['gbytes_per_s'] = row['bytes'] / ms / 1e6
        if 'compulsory_bytes' in row:
            row['compulsory_gbytes_per_s'] = row['compulsory_bytes'] / ms / 1e6
        rows.append(row)
    return rows


def bench_backward_case(net, plan, wts, B, H, W, bi, args):
    pred, gt = images((B, 3, H, W), 1000 + B + H)
    dp, dg = pred.to('cuda'), gt.to('cuda')

    def pair():
        plan.forward(dp, dg, bi)
        return plan.backward()

    ts = event_times(pair, args.reps, args.warmup)
    fwd = event_times(lambda: plan.forward(dp, dg, bi), args.reps, args.warmup)
    res = {'net': net, 'shape': [B, 3, H, W], 'boundary_ignore': bi, 'hip_fwd_bwd_ms_median': statistics.median(ts),
           'hip_fwd_bwd_ms_min': min(ts), 'hip_fwd_bwd_ms_max': max(ts), 'hip_fwd_ms_median': statistics.median(fwd),
           'grad_abs_max_hip': float(pair().abs().max())}
    if args.cpu_reps > 0:
        def host():
            p = pred.clone().requires_grad_(True)
            a, g = ev.lpips_prepare(p, gt, bi)
            ev.lpips_value(a, g, wts)[0].sum().backward()
            return p.grad

        host()
        t0 = time.perf_counter()
        for _ in range(args.cpu_reps):
            grad = host()
        res['cpu_restatement_fwd_bwd_ms'] = (time.perf_counter() - t0) * 1e3 / args.cpu_reps
        res['cpu_over_hip'] = res['cpu_restatement_fwd_bwd_ms'] / res['hip_fwd_bwd_ms_median']
        res['grad_abs_max_cpu'] = float(grad.abs().max())
        res['grad_max_abs_diff_over_max'] = float((pair().cpu() - grad).abs().max() / grad.abs().max())
        res['cpu_threads'] = torch.get_num_threads()
    if args.steps:
        res['steps'] = backward_step_times(plan, dp, dg, bi, max(5, args.reps // 2))
    return res


def bench_case(net, plan, wts, B, H, W, bi, args):
    pred, gt = images((B, 3, H, W), 1000 + B + H)
    dp, dg = pred.to('cuda'), gt.to('cuda')
    ts = event_times(lambda: plan.forward(dp, dg, bi), args.reps, args.warmup)
    res = {'net': net, 'shape': [B, 3, H, W], 'boundary_ignore': bi, 'hip_ms_median': statistics.median(ts),
           'hip_ms_min': min(ts), 'hip_ms_max': max(ts), 'lpips_hip': plan.forward(dp, dg, bi)[0].cpu().tolist()}
    if args.cpu_reps > 0:
        p, g = ev.lpips_prepare(pred, gt, bi)
        with torch.no_grad():
            ev.lpips_value(p, g, wts)
            t0 = time.perf_counter()
            for _ in range(args.cpu_reps):
                v = ev.lpips_value(p, g, wts)[0]
            res['cpu_restatement_ms'] = (time.perf_counter() - t0) * 1e3 / args.cpu_reps
        res['lpips_cpu'] = v.tolist()
        res['cpu_threads'] = torch.get_num_threads()
    if args.steps:
        res['steps'] = step_times(plan, dp, dg, bi, max(5, args.reps // 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--cpu-reps', type=int, default=1)
    ap.add_argument('--steps', action='store_true')
    ap.add_argument('--backward', action='store_true', help='time forward + backward pairs (LPIPSPlan.backward)')
    ap.add_argument('--cases', default='', help='indices into CASES, e.g. 0,2 (default: all)')
    ap.add_argument('--nets', default='alex,vgg')
    ap.add_argument('--k-channels', type=int, default=0,
                    help='input channels per conv launch (0: the plan\'s own LPIPSPlan.K_CHANNELS)')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_lpips: no HIP device (timings are taken on the GPU only)')
    if args.k_channels:
        ops.LPIPSPlan.K_CHANNELS = args.k_channels
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'warmup': args.warmup,
           'k_channels': ops.LPIPSPlan.K_CHANNELS, 'backward': bool(args.backward), 'cases': []}
    for net in args.nets.split(','):
        wts = ev.load_lpips_weights(ev.generate_lpips_state_dict(net, seed=0), net)
        plan = ops.LPIPSPlan({k: ([t.to('cuda') for t in v] if isinstance(v, list) else v) for k, v in wts.items()})
        for i, (B, H, W, bi) in enumerate(CASES):
            if args.cases and str(i) not in args.cases.split(','):
                continue
            res['cases'].append((bench_backward_case if args.backward else bench_case)(net, plan, wts, B, H, W, bi,
                                                                                       args))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
