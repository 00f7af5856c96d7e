"""Timing of DBSRTrainer.step under the objectives of dbsr_amd.objectives at tools/train_synthetic.py's default
training shape (batch 16, bursts of 8, crops of 384 at factor 4: 48x48 RAW frames -> 384x384), one GPU, one process,
the tool's default compute dtype (bf16).

Variants, each a trainer of its own on the same seeded weights and the same bursts:
  none          objective=None (the built-in L1 plan)
  charbonnier   objective='charbonnier'
  l1_ssim       Objective('l1', ssim=0.2)
  l1_lpips      Objective('l1', extra=0.1 * LPIPS(alex, seeded weights, differentiable=True))
  autograd_lpips   the loop tools/train_synthetic.py --lpips ran before the fused step took objectives: net.train();
                pred, _ = net(burst); loss = l1 + 0.1 * lpips; torch.optim.Adam + torch.amp.GradScaler -- the yardstick
                of l1_lpips
After `--warmup` steps each (the fused steps replay HIP graphs from their third step), `--steps` steps are timed one by
one with HIP events; reported per variant: the median, the minimum and the spread (max - min) of the per-step times.
The variants take turns in `--rounds` rounds so that drift hits them alike.

Run it under a time limit, e.g.  timeout -k 10 600 python tools/bench_objective.py --out profiles/objective_bench.json
Usage: python tools/bench_objective.py [--batch 16 --burst 8 --size 48 --steps 20 --warmup 5 --rounds 2 --out FILE]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbsr_amd                                                  # noqa: E402
from dbsr_amd import arch, evaluation                            # noqa: E402
from dbsr_amd.burst import synthetic_bursts                      # noqa: E402
from dbsr_amd.objectives import Objective                        # noqa: E402
from dbsr_amd.training import DBSRTrainer                        # noqa: E402
from dbsr_amd.weights import generate_state_dict                 # noqa: E402

BI = 40


def timed_steps(fn, steps):
    """ms of each of `steps` calls (HIP events around every call, read after the last)."""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for e0, e1 in ev:
        e0.record()
        fn()
        e1.record()
    torch.cuda.synchronize()
    return [e0.elapsed_time(e1) for e0, e1 in ev]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--burst', type=int, default=8)
    ap.add_argument('--size', type=int, default=48)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_objective: no HIP device (timings are taken on the GPU only)')
    dev = torch.device('cuda')
    B, N, H = args.batch, args.burst, args.size
    sd_np = generate_state_dict(arch.state_dict_shapes(dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)),
                                seed=0)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}
    lp_sd = evaluation.generate_lpips_state_dict('alex', seed=0)

    def net():
        n = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
        n.load_state_dict(sd)
        return n.to(dev).set_compute_dtype(torch.bfloat16)

    def lpips():
        return evaluation.LPIPS(boundary_ignore=BI, type='alex', weights=lp_sd, differentiable=True).to(dev)

    burst, gt = synthetic_bursts(B, N, H, H, sr_factor=8, seed=1)
    burst, gt = burst.to(dev), gt.to(dev)

    lp_fused = lpips()
    trainers = {
        'none': DBSRTrainer(net(), boundary_ignore=BI),
        'charbonnier': DBSRTrainer(net(), boundary_ignore=BI, objective='charbonnier'),
        'l1_ssim': DBSRTrainer(net(), objective=Objective('l1', ssim=0.2, boundary_ignore=BI)),
        'l1_lpips': DBSRTrainer(net(), objective=Objective('l1', extra=lambda p, q: 0.1 * lp_fused(p, q),
                                                           boundary_ignore=BI)),
    }
    fns = {k: (lambda tr=tr: tr.step(burst, gt)) for k, tr in trainers.items()}

    anet, alp = net().train(), lpips()
    opt = torch.optim.Adam([p for p in anet.parameters() if p.requires_grad], lr=1e-4)
    scaler = torch.amp.GradScaler('cuda', enabled=False)         # (bf16: the tool enabled it for fp16 only)

    def autograd_step():
        pred, _ = anet(burst)
        l1 = torch.nn.functional.l1_loss(pred[..., BI:-BI, BI:-BI].float(), gt[..., BI:-BI, BI:-BI].float())
        loss = l1 + 0.1 * alp(pred, gt)
        opt.zero_grad(set_to_none=True)
        scaler.scale(loss).backward()
        scaler.step(opt)
        scaler.update()

    fns['autograd_lpips'] = autograd_step
    for fn in fns.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(args.rounds):
        for k, fn in fns.items():
            ms[k] += timed_steps(fn, args.steps)
    res = {'shape': {'batch': B, 'burst': N, 'lr': H, 'hr': 8 * H}, 'dtype': 'bf16', 'steps': args.steps,
           'warmup': args.warmup, 'rounds': args.rounds, 'device': torch.cuda.get_device_name(0),
           'graphs': all(tr.plans[(B, N, H, H)].graphs is not None for tr in trainers.values())}
    for k, v in ms.items():
        res[k] = {'median_ms': statistics.median(v), 'min_ms': min(v), 'spread_ms': max(v) - min(v)}
    base = res['none']['median_ms']
    for k in ms:
        res[k]['minus_none_ms'] = res[k]['median_ms'] - base
    res['l1_lpips_speedup_over_autograd'] = res['autograd_lpips']['median_ms'] / res['l1_lpips']['median_ms']
    out = json.dumps(res, indent=1)
    print(out, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(out + '\n')


if __name__ == '__main__':
    main()
