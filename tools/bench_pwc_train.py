"""Timing of PWC-Net training on one GPU, one process:

  pwc_fwd_bwd   the differentiable PWC-Net forward + backward (pwcnet.PWCNet(differentiable=True), fp32, torch.ops.dbsr.*
                with the HIP backwards of csrc/pwc_grad.hip) at P pairs of S x S (default 104 pairs of 48 x 48: a batch
                of 8 bursts of 14 frames at the synthetic training crop)
  step          a DBSRTrainer step at (B, N, H, H) (default (2, 14, 128, 128), bf16) without alignment_grad (PWC-Net
                frozen: the step as it was) and with it (the differentiable PWC forward, the external-flow plan with
                dL/d(offsets), the PWC backward, Adam on both flat buffers)

Each figure is the median of `--iters` (>= 20) single iterations timed with HIP events after `--warmup` untimed
ones; min and max are reported beside it.  There is no target: the package could not do this before, so the numbers
are recorded, not gated.  --torch-baseline also times torch autograd of the same network (F.conv2d and friends on the
device, the package's correlation and backwarp ops) for a ratio.

Run it under a time limit, e.g.  timeout -k 10 900 python tools/bench_pwc_train.py
Usage: python tools/bench_pwc_train.py [--pairs 104 --size 48 --batch 2 --burst 14 --lr-size 128 --dtype bf16
                                        --iters 20 --warmup 3 --torch-baseline --out profiles/pwc_train_bench.json]"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import dbsr_amd                                                  # noqa: E402
from dbsr_amd import arch                                        # noqa: E402
from dbsr_amd.burst import synthetic_bursts                      # noqa: E402
from dbsr_amd.training import DBSRTrainer                        # noqa: E402
from dbsr_amd.weights import generate_state_dict                 # noqa: E402

DTYPES = {'bf16': torch.bfloat16, 'fp32': torch.float32}


def timed(fn, iters, warmup):
    """{'ms' (median), 'min_ms', 'max_ms', 'iters'} of single calls, each between two HIP events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {'ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'iters': iters}


def torch_pwc(pwc, src, tgt):
    """The same network under torch autograd on the device (the conv, ConvTranspose and resize of ATen; correlation
    and backwarp have no torch equivalent on the device and stay the package's ops)."""
    import torch.nn.functional as F
    ops = torch.ops.dbsr
    H, W = src.shape[-2:]
    Hp, Wp = (H + 63) // 64 * 64, (W + 63) // 64 * 64
    P = src.shape[0]
    x = F.interpolate(torch.cat([tgt, src], 0), size=(Hp, Wp), mode='bilinear', align_corners=False)
    net = pwc.net
    feats = []
    for name in ['netOne', 'netTwo', 'netThr', 'netFou', 'netFiv', 'netSix']:
        x = getattr(net.netExtractor, name)(x)
        feats.append(x)
    est = None
    scale = {5: 0.625, 4: 1.25, 3: 2.5, 2: 5.0}
    for level, name in [(6, 'netSix'), (5, 'netFiv'), (4, 'netFou'), (3, 'netThr'), (2, 'netTwo')]:
        dec = getattr(net, name)
        first, second = feats[level - 1][:P].contiguous(), feats[level - 1][P:].contiguous()
        if est is None:
            feat = ops.correlation(first, second, True)
        else:
            flow, upfeat = dec.netUpflow(est[0]), dec.netUpfeat(est[1])
            warped = ops.backwarp(second, (flow * scale[level]).contiguous())
            feat = torch.cat([ops.correlation(first, warped.contiguous(), True), first, flow, upfeat], 1)
        for sub in ['netOne', 'netTwo', 'netThr', 'netFou', 'netFiv']:
            feat = torch.cat([getattr(dec, sub)(feat), feat], 1)
        est = (dec.netSix(feat), feat)
    flow = est[0] + net.netRefiner.netMain(est[1])
    flow = 20.0 * F.interpolate(flow, size=(H, W), mode='bilinear', align_corners=False)
    return torch.stack((flow[:, 0] * (W / Wp), flow[:, 1] * (H / Hp)), 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=104)
    ap.add_argument('--size', type=int, default=48)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--burst', type=int, default=14)
    ap.add_argument('--lr-size', type=int, default=128)
    ap.add_argument('--dtype', choices=sorted(DTYPES), default='bf16')
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-baseline', action='store_true')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'pwc_train_bench.json'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_pwc_train: no HIP device (timings are taken on the GPU only)')
    if args.iters < 20:
        sys.exit('bench_pwc_train: --iters must be >= 20 (the figure is a median)')
    dev = torch.device('cuda')
    kw = dict(dbsr_amd.DBSR_SYNTHETIC_KWARGS, train_alignmentnet=True)
    sd_np = generate_state_dict(arch.state_dict_shapes(dbsr_amd.dbsrnet_cvpr2021(**kw)), seed=0)
    sd = {k: torch.from_numpy(v) for k, v in sd_np.items()}

    def build(train_alignmentnet, dtype=torch.float32):
        n = dbsr_amd.dbsrnet_cvpr2021(**dict(kw, train_alignmentnet=train_alignmentnet))
        n.load_state_dict(sd)
        return n.to(dev).set_compute_dtype(dtype).train()

    res = {'device': torch.cuda.get_device_name(0), 'iters': args.iters, 'warmup': args.warmup}

    # ---- the differentiable PWC-Net alone
    P, S = args.pairs, args.size
    g = torch.Generator().manual_seed(0)
    src, tgt = torch.rand(P, 3, S, S, generator=g).to(dev), torch.rand(P, 3, S, S, generator=g).to(dev)
    G = torch.randn(P, 2, S, S, generator=g).to(dev)
    pwc = build(True).encoder.alignment_net
    params = list(pwc.parameters())

    def fwd_bwd(forward):
        flow = forward()
        torch.autograd.grad(flow, params, G, allow_unused=True)

    res['pwc_fwd_bwd'] = dict(timed(lambda: fwd_bwd(lambda: pwc(src, tgt)), args.iters, args.warmup),
                              pairs=P, size=S, dtype='fp32')
    with torch.no_grad():
        pwc.differentiable = False
        res['pwc_fwd_engine'] = dict(timed(lambda: pwc(src, tgt), args.iters, args.warmup), pairs=P, size=S)
        pwc.differentiable = True
    if args.torch_baseline:
        res['pwc_fwd_bwd_torch'] = dict(timed(lambda: fwd_bwd(lambda: torch_pwc(pwc, src, tgt)), args.iters, args.warmup),
                                        pairs=P, size=S, dtype='fp32')
        res['hip_over_torch'] = res['pwc_fwd_bwd']['ms'] / res['pwc_fwd_bwd_torch']['ms']
    del pwc, params

    # ---- the trainer step with and without alignment_grad
    B, N, H = args.batch, args.burst, args.lr_size
    dt = DTYPES[args.dtype]
    burst, gt = synthetic_bursts(B, N, H, H, sr_factor=8, seed=1)
    burst, gt = burst.to(dev), gt.to(dev)
    off = DBSRTrainer(build(False, dt), boundary_ignore=40)
    res['step_alignment_grad_off'] = dict(timed(lambda: off.step(burst, gt), args.iters, args.warmup),
                                          shape=[B, N, H, H], dtype=args.dtype)
    del off
    on = DBSRTrainer(build(True, dt), boundary_ignore=40, alignment_grad=True)
    res['step_alignment_grad_on'] = dict(timed(lambda: on.step(burst, gt), args.iters, args.warmup),
                                         shape=[B, N, H, H], dtype=args.dtype)
    res['on_minus_off_ms'] = res['step_alignment_grad_on']['ms'] - res['step_alignment_grad_off']['ms']
    text = json.dumps(res, indent=1)
    print(text, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
