"""Timing of the real-world fine-tuning step (training.DBSRRealWorldTrainer) at the default_realworld shape
(train_settings/dbsr/default_realworld.py: batch 12, burst 8, 56x56 RAW crops -> 448x448, bf16) beside
DBSRTrainer.step (the synthetic recipe's L1 objective) at the same shape in the same process, and of the
objective's parts on the step's own buffers:

  alignment   SpatialColorAlignment.align: PWC-Net on B pairs at 448^2 (fp32), flow / gt x1/8, base-frame warp,
              two smoothings, colour fit, validity mask
  loss        dbsr_aligned_l1_forward  (pixel pass + the one-block reduction)
  backward    dbsr_aligned_l1_backward (zero + scatter-add + the scale / gate / cast pass writing dP)

Times are HIP-event times over `--reps` back-to-back runs after `--warmup` runs (the steps replay their HIP
graphs from the second run on).  The two calls' achieved bytes/s are their algorithmic bytes (from the shape,
below) over their event time -- call-level figures, not a share of peak of one kernel.  Prints one JSON line.

Run it under a time limit, e.g.  timeout -k 10 600 python tools/bench_realworld.py > profiles/realworld_bench.json
Usage: python tools/bench_realworld.py [--batch 12 --burst 8 --size 56 --reps 10 --warmup 3]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbsr_amd                                                  # noqa: E402
from dbsr_amd import _lib as L                                   # noqa: E402
from dbsr_amd import arch                                        # noqa: E402
from dbsr_amd.burst import synthetic_bursts                      # noqa: E402
from dbsr_amd.training import DBSRRealWorldTrainer, DBSRTrainer  # noqa: E402
from dbsr_amd.weights import generate_state_dict                 # noqa: E402

# algorithmic bytes per HR pixel.  forward: flow 8 + valid 1 + gt 12 + pred 12 (each tap once: neighbours share
# them through the L2) read, g_pw 12 written.  backward: 12 zeroed; flow 8 + g_pw 12 read and 4 taps x 3 planes x
# 4 B of atomic adds; then sums 12 + pred 12 read and the 8-channel bf16 dP 16 written.
FWD_BYTES = 8 + 1 + 12 + 12 + 12
BWD_ATOMIC_BYTES = 4 * 3 * 4
BWD_BYTES = 12 + (8 + 12 + BWD_ATOMIC_BYTES) + (12 + 12 + 16)


def timed(fn, reps, warmup):
    """ms per call: HIP events around `reps` back-to-back calls after `warmup` calls."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=12)
    ap.add_argument('--burst', type=int, default=8)
    ap.add_argument('--size', type=int, default=56)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_realworld: no HIP device (timings are taken on the GPU only)')
    dev = torch.device('cuda')
    B, N, H = args.batch, args.burst, args.size
    sd_np = generate_state_dict(arch.state_dict_shapes(dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)),
                                seed=0)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}

    def net():
        n = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
        n.load_state_dict(sd)
        return n.to(dev).set_compute_dtype(torch.bfloat16)

    pre = 'encoder.alignment_net.'
    pwc = dbsr_amd.PWCNet(load_pretrained=False)
    pwc.load_state_dict({k[len(pre):]: v for k, v in sd.items() if k.startswith(pre)})
    pwc = pwc.to(dev)
    burst, gt = synthetic_bursts(B, N, H, H, sr_factor=8, seed=1)
    burst, gt = burst.to(dev), gt.to(dev)
    res = {'shape': {'batch': B, 'burst': N, 'lr': H, 'hr': 8 * H, 'dtype': 'bf16'}, 'reps': args.reps,
           'device': torch.cuda.get_device_name(0)}

    base = DBSRTrainer(net(), boundary_ignore=40)
    res['synthetic_step_ms'] = timed(lambda: base.step(burst, gt), args.reps, args.warmup)
    del base
    torch.cuda.empty_cache()

    tr = DBSRRealWorldTrainer(net(), pwc, sr_factor=4, loss_weight=10.0, boundary_ignore=40)
    res['realworld_step_ms'] = timed(lambda: tr.step(burst, gt), args.reps, args.warmup)
    res['added_ms'] = res['realworld_step_ms'] - res['synthetic_step_ms']
    res['last_stats'] = tr.last_stats

    # the objective's parts on the step's own buffers
    plan = tr.plans[(B, N, H, H)]
    pred, gtb, rw = plan.bufs['pred'], plan.bufs['gt'], plan.rw
    HS = 8 * H
    lib, s = L.lib(), L.stream_ptr(dev)
    res['alignment_ms'] = timed(lambda: tr.sca.align(pred, gtb, plan.bufs['burst']), args.reps, args.warmup)
    flow, cmat, valid = tr.sca.last_alignment

    def fwd():
        L.check(lib.dbsr_aligned_l1_forward(B, HS, HS, 40, pred.data_ptr(), flow.data_ptr(), cmat.data_ptr(),
                                            valid.data_ptr(), gtb.data_ptr(), 10.0, rw['g_pw'].data_ptr(),
                                            tr._loss2.data_ptr(), rw['stats'].data_ptr(), rw['ws'].data_ptr(),
                                            rw['need'], s), 'fwd')

    def bwd():
        L.check(lib.dbsr_aligned_l1_backward(B, HS, HS, pred.data_ptr(), flow.data_ptr(), rw['g_pw'].data_ptr(), None,
                                             tr._loss2.data_ptr() + 4, None, plan.dP.d(0), rw['ws'].data_ptr(),
                                             rw['need'], s), 'bwd')
    res['loss_forward_ms'] = timed(fwd, 10 * args.reps, args.warmup)
    res['loss_backward_ms'] = timed(bwd, 10 * args.reps, args.warmup)
    px = B * HS * HS
    res['valid_in_crop'] = float(valid[..., 40:-40, 40:-40].float().mean())
    res['loss_forward_algorithmic_MB'] = px * FWD_BYTES / 1e6
    res['loss_backward_algorithmic_MB'] = px * BWD_BYTES / 1e6
    res['loss_backward_atomic_MB'] = px * BWD_ATOMIC_BYTES / 1e6
    res['loss_forward_GBps'] = px * FWD_BYTES / (res['loss_forward_ms'] * 1e-3) / 1e9
    res['loss_backward_GBps'] = px * BWD_BYTES / (res['loss_backward_ms'] * 1e-3) / 1e9
    res['objective_kernels_share_of_added'] = (res['loss_forward_ms'] + res['loss_backward_ms']) / max(res['added_ms'], 1e-9)
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
