"""Timing of the synthetic-data generator at the default_synthetic recipe's shape: B = 16 crops of 432 x 432 (384 plus
the 24-pixel border on each side), N = 8 frames, downsample factor 4 -> RAW bursts [16,8,4,48,48] and ground truth
[16,3,384,384].

Timed, all on the same GPU:
  hip_unprocess_ms        dbsr_unprocess_rgb on the uint8 batch
  hip_burst_ms            dbsr_burst_synth with noise, RAW burst only (what training needs)
  hip_burst_rgb_flow_ms   the same with burst_rgb and flow written too
  processing_ms           the whole SyntheticBurstProcessing call from a list of host uint8 images: crops, host
                          sampling, one upload, torch.randn, the two kernels (wall clock, ends in a synchronise)
  torch_generator_ms      a torch restatement of the two kernels (elementwise ops and gathers, batched over B and N)
  train_step_ms           one DBSRTrainer.step (bf16, HIP graphs) on the generated batch
and generator_share_of_step = processing_ms / train_step_ms.

Kernel times are HIP-event times over `--reps` back-to-back calls after `--warmup` calls; every figure is the median
of `--trials` such windows, with the lowest and highest beside it (the machine is shared).  Prints one JSON line.

Run it under a time limit, e.g.  timeout -k 10 400 python tools/bench_datagen.py > profiles/datagen_bench.json
Usage: python tools/bench_datagen.py [--reps 1000 --warmup 10 --trials 5 --batch 16 --frames 8]"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dbsr_amd  # noqa: E402
from dbsr_amd import ops  # noqa: E402
from dbsr_amd import synthetic as S  # noqa: E402

BTP = {'max_translation': 24.0, 'max_rotation': 1.0, 'max_shear': 0.0, 'max_scale': 0.0, 'border_crop': 24}


def event_ms(fn, reps, warmup):
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


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def trials(timer, fn, reps, warmup, n):
    t = [timer(fn, reps, warmup if i == 0 else 1) for i in range(n)]
    return {'median': statistics.median(t), 'min': min(t), 'max': max(t)}


def torch_unprocess(x, params):
    """dbsr_unprocess_rgb as batched torch ops (x float [B,3,H,W], params [B,16] with both flags on)."""
    x = 0.5 - torch.sin(torch.asin(1.0 - 2.0 * x.clamp(0.0, 1.0)) / 3.0)
    x = x.clamp(1e-8) ** 2.2
    B = x.shape[0]
    x = torch.bmm(params[:, :9].view(B, 3, 3), x.view(B, 3, -1)).view_as(x)
    rgb, red, blue = params[:, 9], params[:, 10], params[:, 11]
    gains = torch.stack([1.0 / red / rgb, 1.0 / rgb, 1.0 / blue / rgb], 1).view(B, 3, 1, 1)
    mask = ((x.mean(1, keepdim=True) - 0.9).clamp(0.0) / 0.1) ** 2
    return (x * torch.max(mask + (1.0 - mask) * gains, gains)).clamp(0.0, 1.0)


def torch_burst(lin, ainv, bc, f, levels, z):
    """dbsr_burst_synth (RAW burst only) as batched torch ops: index gathers, outside taps contribute 0."""
    B, N = ainv.shape[:2]
    Hc, Wc = lin.shape[-2:]
    H2, W2 = (Hc - 2 * bc) // f, (Wc - 2 * bc) // f
    dev = lin.device
    taps = [f // 2 - 1, f // 2] if f % 2 == 0 else [(f - 1) // 2]
    Y, X = torch.meshgrid(torch.arange(H2, device=dev), torch.arange(W2, device=dev), indexing='ij')
    a = ainv.view(B, N, 6, 1, 1)
    flat = lin.reshape(B, 3, Hc * Wc)
    acc = torch.zeros(B, 3, N, H2, W2, device=dev)
    for j in taps:
        for i in taps:
            px, py = (bc + f * X + i).float(), (bc + f * Y + j).float()
            sx = a[:, :, 0] * px + a[:, :, 1] * py + a[:, :, 2]
            sy = a[:, :, 3] * px + a[:, :, 4] * py + a[:, :, 5]
            x0, y0 = torch.floor(sx), torch.floor(sy)
            fx, fy = sx - x0, sy - y0
            xi, yi = x0.long(), y0.long()
            for (dy, dx), w in (((0, 0), (1 - fx) * (1 - fy)), ((0, 1), fx * (1 - fy)), ((1, 0), (1 - fx) * fy),
                                ((1, 1), fx * fy)):
                xx, yy = xi + dx, yi + dy
                ok = ((xx >= 0) & (xx < Wc) & (yy >= 0) & (yy < Hc)).float()
                idx = (yy.clamp(0, Hc - 1) * Wc + xx.clamp(0, Wc - 1)).view(B, 1, -1).expand(-1, 3, -1)
                acc = acc + (w * ok).unsqueeze(1) * torch.gather(flat, 2, idx).view(B, 3, N, H2, W2)
    rgb = (acc * (1.0 / len(taps) ** 2)).transpose(1, 2)
    raw = S.mosaic(rgb)
    var = raw * levels[:, 0].view(B, 1, 1, 1, 1) + levels[:, 1].view(B, 1, 1, 1, 1)
    return (raw + z * var.sqrt()).clamp(0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=1000)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--trials', type=int, default=5)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--crop', type=int, default=384)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_datagen: no HIP device (timings are taken on the GPU only)')
    dev = torch.device('cuda')
    B, N, f, bc = args.batch, args.frames, 4, BTP['border_crop']
    Hc = args.crop + 2 * bc
    random.seed(1)
    torch.manual_seed(1)
    gen = torch.Generator().manual_seed(1)
    images = [torch.randint(0, 256, (Hc + 40, Hc + 60, 3), generator=gen, dtype=torch.uint8).numpy() for _ in range(B)]
    proc = S.SyntheticBurstProcessing(args.crop, N, f, burst_transformation_params=BTP, device=dev)
    data = proc(images)
    assert data['burst'].shape == (B, N, 4, args.crop // 8, args.crop // 8)

    # fixed device inputs for the kernel timings
    ipp = S._image_processing_params(None)
    samples = [S._sample_one((Hc, Hc), N, f, BTP, ipp) for _ in range(B)]
    params = S._pack_params([s['rgb2cam'] for s in samples], [s['rgb_gain'] for s in samples],
                            [s['red_gain'] for s in samples], [s['blue_gain'] for s in samples], [True] * B,
                            [True] * B).to(dev)
    u8 = torch.stack([torch.from_numpy(im[:Hc, :Hc]) for im in images]).contiguous().to(dev)
    ainv = torch.from_numpy(np.stack([s['ainv'] for s in samples])).float().to(dev)
    levels = torch.tensor([[s['shot_noise_level'], s['read_noise_level']] for s in samples]).float().to(dev)
    z = torch.randn(B, N, 4, args.crop // 8, args.crop // 8, device=dev)
    lin = ops.unprocess_rgb(u8, params)
    xf = u8.permute(0, 3, 1, 2).float() / 255.0

    res = {'device': torch.cuda.get_device_name(0), 'shape': {'B': B, 'N': N, 'crop': Hc, 'factor': f, 'border': bc},
           'reps': args.reps, 'trials': args.trials}
    t = lambda fn, timer=event_ms, reps=args.reps: trials(timer, fn, reps, args.warmup, args.trials)    # noqa: E731
    res['hip_unprocess_ms'] = t(lambda: ops.unprocess_rgb(u8, params))
    res['hip_burst_ms'] = t(lambda: ops.burst_synth(lin, ainv, bc, f, levels, z, want_rgb=False, want_flow=False))
    res['hip_burst_rgb_flow_ms'] = t(lambda: ops.burst_synth(lin, ainv, bc, f, levels, z))
    res['processing_ms'] = t(lambda: proc(images), wall_ms, max(5, args.reps // 20))
    with torch.no_grad():
        res['torch_generator_ms'] = t(lambda: torch_burst(torch_unprocess(xf, params), ainv, bc, f, levels, z),
                                      event_ms, max(5, args.reps // 20))
        ref = torch_burst(torch_unprocess(xf, params), ainv, bc, f, levels, z)
    hip = ops.burst_synth(lin, ainv, bc, f, levels, z, want_rgb=False, want_flow=False)[0]
    res['hip_vs_torch_max_abs_diff'] = float((hip - ref).abs().max())

    from dbsr_amd.training import DBSRTrainer
    net = dbsr_amd.build_synthetic_net(seed=0).to(dev).set_compute_dtype(torch.bfloat16)
    tr = DBSRTrainer(net)
    res['train_step_ms'] = t(lambda: tr.step(data['burst'], data['frame_gt']), wall_ms, max(5, args.reps // 20))
    res['generator_kernels_ms'] = res['hip_unprocess_ms']['median'] + res['hip_burst_ms']['median']
    res['generator_share_of_step'] = res['processing_ms']['median'] / res['train_step_ms']['median']
    res['kernels_share_of_step'] = res['generator_kernels_ms'] / res['train_step_ms']['median']
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
