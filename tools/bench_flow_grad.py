"""Timing of the training step with and without the flow gradient (DBSRTrainer(flow_grad=...)) at configs[3]'s
per-GPU step shape (batch 8, 14 frames, 128x128 RAW -> 1024x1024), one GPU, one process, the same build.

The trainers take turns: `--rounds` rounds, each timing `--reps` back-to-back steps of one and then of the other
(HIP events; the steps replay their HIP graphs after the first), after `--warmup` steps of each.  Reported per leg:
every round's ms per step, their median and spread (max - min over the rounds).  The yardsticks: the
flow_grad=False leg is the step as it was before the option existed (the same op list), and the new kernel
bwd.warp.flow is set beside bwd.warp (the warp's feature gradient, a comparable number of bytes) and the forward
warp of the same run, each timed alone on the whole chip (Plan.time_ops) with its algorithmic bytes:

    warp            reads up to 4 corner rows, writes 1 row per pixel        (5 rows)
    bwd.warp        reads dout rows through the binned gather, writes 1 row  (>= 2 rows + the gate row)
    bwd.warp.flow   reads 1 dout row + up to 4 corner rows, writes 8 bytes   (5 rows)

with a row = c elements of the compute dtype (1 KiB at c = 512, 16-bit).  Neighbouring pixels share corner rows, so
the compulsory HBM traffic of the two samplers is about 2 rows per pixel; the 5-row figure is what the lanes load.

Run it under a time limit, e.g.  timeout -k 10 600 python tools/bench_flow_grad.py
Usage: python tools/bench_flow_grad.py [--batch 8 --burst 14 --size 128 --rounds 5 --reps 5 --warmup 3
                                        --dtype bf16 --out profiles/flow_grad_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import dbsr_amd                                                  # noqa: E402
from dbsr_amd import _lib as L                                   # noqa: E402
from dbsr_amd import arch                                        # noqa: E402
from dbsr_amd.burst import synthetic_bursts                      # noqa: E402
from dbsr_amd.training import DBSRTrainer                        # noqa: E402
from dbsr_amd.weights import generate_state_dict                 # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp16': torch.float16, 'fp32': torch.float32}
OPS = ('warp', 'bwd.warp', 'bwd.warp.flow', 'bwd.ofe.init.dgrad')


def timed(fn, reps):
    """ms per call: HIP events around `reps` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def measure(trainers, burst, gt, rounds, reps, warmup):
    """{leg: {'step_ms_rounds', 'step_ms', 'spread_ms'}} of trainers {leg: trainer}, alternating."""
    for tr in trainers.values():
        for _ in range(warmup):
            tr.step(burst, gt)
    torch.cuda.synchronize()
    ms = {k: [] for k in trainers}
    for _ in range(rounds):
        for k, tr in trainers.items():
            ms[k].append(timed(lambda: tr.step(burst, gt), reps))
    return {k: {'step_ms_rounds': v, 'step_ms': statistics.median(v), 'spread_ms': max(v) - min(v)}
            for k, v in ms.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--burst', type=int, default=14)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--dtype', choices=sorted(DTYPES), default='bf16')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'flow_grad_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_flow_grad: no HIP device (timings are taken on the GPU only)')
    dev = torch.device('cuda')
    dt = DTYPES[args.dtype]
    B, N, H = args.batch, args.burst, args.size
    sd_np = generate_state_dict(arch.state_dict_shapes(dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)),
                                seed=0)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}

    def trainer(flow_grad):
        n = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
        n.load_state_dict(sd)
        return DBSRTrainer(n.to(dev).set_compute_dtype(dt), boundary_ignore=40, flow_grad=flow_grad)

    burst, gt = synthetic_bursts(B, N, H, H, sr_factor=8, seed=1)
    burst, gt = burst.to(dev), gt.to(dev)
    trs = {'flow_grad_off': trainer(False), 'flow_grad_on': trainer(True)}
    res = {'shape': {'batch': B, 'burst': N, 'lr': H, 'hr': 8 * H}, 'dtype': args.dtype, 'rounds': args.rounds,
           'reps': args.reps, 'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}
    res.update(measure(trs, burst, gt, args.rounds, args.reps, args.warmup))
    res['on_minus_off_ms'] = res['flow_grad_on']['step_ms'] - res['flow_grad_off']['step_ms']
    res['graphs'] = all(tr.plans[(B, N, H, H)].graphs is not None for tr in trs.values())

    # the new ops beside the two warps of the same plan, each alone on the whole chip
    plan = trs['flow_grad_on'].plans[(B, N, H, H)]
    times = dict((n, t) for n, t in plan.time_ops(L.stream_ptr(dev), reps=10) if n in OPS)
    C = trs['flow_grad_on'].enc_out.cout
    row = C * (4 if dt == torch.float32 else 2)
    px = B * (N - 1) * H * H
    loaded = {'warp': 5 * row * px, 'bwd.warp': 3 * row * px, 'bwd.warp.flow': 5 * row * px + 8 * px}
    res['ops'] = {n: {'ms': times[n], 'lane_bytes': loaded.get(n),
                      'lane_GBps': loaded[n] / (times[n] * 1e-3) / 1e9 if n in loaded else None} for n in OPS}
    res['bwd_warp_flow_over_bwd_warp'] = times['bwd.warp.flow'] / times['bwd.warp']
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
