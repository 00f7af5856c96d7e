"""Timing of the fp16 training step with the dynamic loss scaler beside the bf16 step (no scaler) at configs[3]'s
per-GPU step shape (batch 8, 14 frames, 128x128 RAW -> 1024x1024), one GPU, one process, the same build.

The two trainers take turns: `--rounds` rounds, each timing `--reps` back-to-back steps of one and then of the
other (HIP events; the steps replay their HIP graphs after the first), after `--warmup` steps of each.  Reported
per dtype: every round's ms per step, their median and spread (max - min over the rounds), and the difference of
the medians.  fp16 moves the same bytes at the same MFMA rates as bf16, so the expectation is bf16's time plus
the scaler's three launches (dbsr_grad_unscale_check, dbsr_adam_step_guarded in place of dbsr_adam_step,
dbsr_loss_scale_update).

The unscale pass is timed on the trainer's own gradient buffer (scale 1, so repeating it changes nothing):
8 bytes per parameter over the event time of back-to-back calls, as a fraction of the 8 TB/s HBM peak -- a
call-level figure: the 3.64 M-parameter buffer (14.6 MB) fits in the last-level cache and the pass is a few
microseconds, so launch gaps weigh in.  The two Adam launches are timed the same way with lr 0.

Run it under a time limit, e.g.  timeout -k 10 600 python tools/bench_loss_scale.py > profiles/loss_scale_bench.json
Usage: python tools/bench_loss_scale.py [--batch 8 --burst 14 --size 128 --rounds 5 --reps 5 --warmup 3]"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbsr_amd                                                  # noqa: E402
from dbsr_amd import _lib as L                                   # noqa: E402
from dbsr_amd import arch                                        # noqa: E402
from dbsr_amd.burst import synthetic_bursts                      # noqa: E402
from dbsr_amd.training import DBSRTrainer                        # noqa: E402
from dbsr_amd.weights import generate_state_dict                 # noqa: E402

HBM_PEAK = 8.0e12                                                # bytes/s (MI355X)


def timed(fn, reps):
    """ms per call: HIP events around `reps` back-to-back calls."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--burst', type=int, default=14)
    ap.add_argument('--size', type=int, default=128)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_loss_scale: no HIP device (timings are taken on the GPU only)')
    dev = torch.device('cuda')
    B, N, H = args.batch, args.burst, args.size
    sd_np = generate_state_dict(arch.state_dict_shapes(dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)),
                                seed=0)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}

    def trainer(dtype):
        n = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
        n.load_state_dict(sd)
        return DBSRTrainer(n.to(dev).set_compute_dtype(dtype), boundary_ignore=40)

    burst, gt = synthetic_bursts(B, N, H, H, sr_factor=8, seed=1)
    burst, gt = burst.to(dev), gt.to(dev)
    trs = {'bf16': trainer(torch.bfloat16), 'fp16': trainer(torch.float16)}
    assert trs['bf16'].loss_scale_state() is None and trs['fp16'].loss_scale_state() is not None
    res = {'shape': {'batch': B, 'burst': N, 'lr': H, 'hr': 8 * H}, 'rounds': args.rounds, 'reps': args.reps,
           'warmup': args.warmup, 'device': torch.cuda.get_device_name(0)}
    for tr in trs.values():
        for _ in range(args.warmup):
            tr.step(burst, gt)
    torch.cuda.synchronize()
    ms = {k: [] for k in trs}
    for _ in range(args.rounds):
        for k, tr in trs.items():
            ms[k].append(timed(lambda: tr.step(burst, gt), args.reps))
    for k in trs:
        res[k + '_step_ms_rounds'] = ms[k]
        res[k + '_step_ms'] = statistics.median(ms[k])
        res[k + '_spread_ms'] = max(ms[k]) - min(ms[k])
    res['fp16_minus_bf16_ms'] = res['fp16_step_ms'] - res['bf16_step_ms']
    res['fp16_scaler_state'] = trs['fp16'].loss_scale_state()
    res['graphs'] = all(tr.plans[(B, N, H, H)].graphs is not None for tr in trs.values())

    # the scaler's launches on the fp16 trainer's own buffers
    tr = trs['fp16']
    lib, s, n = L.lib(), L.stream_ptr(dev), tr.n_params
    tr.set_loss_scale(1.0)
    many = 200

    def unscale():
        L.check(lib.dbsr_grad_unscale_check(n, tr.flat_grad.data_ptr(), tr._ls.data_ptr(), s), 'unscale')

    def adam():
        L.check(lib.dbsr_adam_step(n, tr.flat.data_ptr(), tr.flat_grad.data_ptr(), tr.exp_avg.data_ptr(),
                                   tr.exp_avg_sq.data_ptr(), 0.0, 0.9, 0.999, 1e-8, 1, 1.0, s), 'adam')

    def adam_guarded():
        L.check(lib.dbsr_adam_step_guarded(n, tr.flat.data_ptr(), tr.flat_grad.data_ptr(), tr.exp_avg.data_ptr(),
                                           tr.exp_avg_sq.data_ptr(), 0.0, 0.9, 0.999, 1e-8, 1.0, tr._ls.data_ptr(), s),
                'adam_guarded')

    def update():
        L.check(lib.dbsr_loss_scale_update(tr._ls.data_ptr(), 1.0, 1.0, 1 << 30, s), 'update')

    for name, fn in (('unscale_check', unscale), ('adam_step', adam), ('adam_step_guarded', adam_guarded),
                     ('loss_scale_update', update)):
        timed(fn, 10)
        res[name + '_us'] = [1e3 * timed(fn, many) for _ in range(3)]
    res['n_params'] = n
    us = min(res['unscale_check_us'])
    res['unscale_check_GBps'] = 8.0 * n / (us * 1e-6) / 1e9
    res['unscale_check_fraction_of_8TBps'] = 8.0 * n / (us * 1e-6) / HBM_PEAK
    res['scaler_added_launches_us'] = (min(res['unscale_check_us']) + min(res['adam_step_guarded_us']) -
                                       min(res['adam_step_us']) + min(res['loss_scale_update_us']))
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
