"""Timing of the SSIM metric kernels (csrc/metrics.hip: dbsr_ssim_forward, dbsr_ssim_backward) beside the torch
restatement of the reference arithmetic (evaluation.ssim_map + the masked mean: five depthwise 11x11
convolutions, the elementwise map and a reduction; its backward is torch autograd) on the same GPU.

Shapes: the BurstSR scoring shape, 1x3x640x640 with boundary_ignore 40 (evaluation/burstsr/compute_score.py:53),
and a batch of 12 of them.  The mask is random (60 % valid); the inputs are smooth images plus noise.

Times are HIP-event times over `--reps` back-to-back calls after `--warmup` calls, on preallocated buffers for the
kernels (the C entry points, as a scorer would hold them) and through the Python module for torch.  Prints one
JSON line.

Run it under a time limit, e.g.  timeout -k 10 300 python tools/bench_metrics.py > profiles/ssim_bench.json
Usage: python tools/bench_metrics.py [--reps 50 --warmup 5]"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbsr_amd import _lib as L                                   # noqa: E402
from dbsr_amd import evaluation as ev                            # noqa: E402


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


def bench_shape(B, C, H, W, bi, reps, warmup):
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(B)
    gt = F.avg_pool2d(torch.rand(B, C, H + 4, W + 4, generator=gen), 5, 1).to(dev)
    pred = (gt + 0.02 * torch.randn(gt.shape, generator=gen).to(dev)).clamp(0.0, 1.0)
    valid = (torch.rand(B, 1, H, W, generator=gen) > 0.4).to(dev)
    v8 = valid.to(torch.uint8)
    lib, s = L.lib(), L.stream_ptr(dev)
    need = lib.dbsr_ssim_workspace_bytes(B, C, H, W, bi)
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    sums = torch.empty(B, 2, device=dev)
    result = torch.empty(2, device=dev)
    gpred = torch.empty_like(pred)

    def fwd():
        L.check(lib.dbsr_ssim_forward(B, C, H, W, bi, pred.data_ptr(), gt.data_ptr(), v8.data_ptr(), 1.0, None,
                                      sums.data_ptr(), result.data_ptr(), ws.data_ptr(), need, s), 'fwd')

    def bwd():
        L.check(lib.dbsr_ssim_backward(B, C, H, W, bi, pred.data_ptr(), gt.data_ptr(), v8.data_ptr(), 1.0,
                                       result.data_ptr() + 4, gpred.data_ptr(), None, 0, s), 'bwd')

    crop = lambda t: t[..., bi:-bi, bi:-bi]                                            # noqa: E731
    vf = crop(valid)[..., 5:-5, 5:-5].float()

    def torch_fwd(p=pred):
        smap = ev.ssim_map(crop(p), crop(gt), 1.0)
        return (smap * vf).sum() / (vf.sum() * C + 1e-12)

    def torch_fwd_bwd():
        p = pred.detach().requires_grad_(True)
        torch_fwd(p).backward()
        return p.grad

    res = {'shape': [B, C, H, W], 'boundary_ignore': bi, 'valid_fraction': float(vf.mean())}
    res['hip_forward_ms'] = timed(fwd, reps, warmup)
    res['hip_backward_ms'] = timed(bwd, reps, warmup)
    with torch.no_grad():
        res['torch_forward_ms'] = timed(torch_fwd, reps, warmup)
    fb = timed(torch_fwd_bwd, reps, warmup)
    res['torch_forward_backward_ms'] = fb
    res['torch_backward_ms'] = fb - res['torch_forward_ms']
    res['ssim_hip'] = float(result[0])
    with torch.no_grad():
        res['ssim_torch'] = float(torch_fwd())
    res['grad_max_abs_diff'] = float((gpred - torch_fwd_bwd()).abs().max())
    res['forward_speedup'] = res['torch_forward_ms'] / res['hip_forward_ms']
    res['backward_speedup'] = res['torch_backward_ms'] / res['hip_backward_ms']
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_metrics: no HIP device (timings are taken on the GPU only)')
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps,
           'cases': [bench_shape(B, 3, 640, 640, 40, args.reps, args.warmup) for B in (1, 12)]}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
