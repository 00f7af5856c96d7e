"""Where a resblock32_kernel launch spends its cycles (diagnostic stamp build, see tools/pipe_stamps.py).

Build:  make exp EXP_FLAGS=-DDBSR_PIPE_STAMPS EXP_NAME=stamps
Run:    DBSR_HIP_LIB=deep-rawburst-sr_amd/libdbsr_hip_stamps.so python tools/rb32_stamps.py [--head]
Slots: 0 start, 2 weights loaded + first halo landed, per tile t: 3+5t before the first barrier, 4+5t past it,
5+5t conv1 done (with the next halo's DMA issue in front of it), 6+5t past the second barrier, 7+5t conv2 done;
1 end.  Printed per wave (the waves of a block do different shares of conv1), medians over the blocks, the first tile
(prologue) apart from the steady ones."""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from dbsr_amd import _lib as L                     # noqa: E402
from dbsr_amd.engine import NHWC, PackedConv, Plan  # noqa: E402

SLOTS = 24 * 5 + 2
MAXT = 23


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=8)
    ap.add_argument('--size', type=int, default=384)
    ap.add_argument('--head', action='store_true')
    args = ap.parse_args()
    B, H, W, C = args.frames, args.size, args.size, 32
    dev, dt = torch.device('cuda'), torch.float16
    s = torch.cuda.current_stream().cuda_stream
    fn = L.lib().dbsr_diag_pipe_stamps
    fn.argtypes = [ctypes.c_void_p, ctypes.c_longlong]
    pcs = [PackedConv(torch.nn.Conv2d(C, C, 3, padding=1).to(dev), dt, dev, s) for _ in range(2)]
    X, M, Y = (NHWC(B, H, W, C, dt, dev) for _ in range(3))
    X.t.normal_()
    plan = Plan()
    kw = {}
    if args.head:
        pred = torch.zeros(B, 3, H, W, dtype=torch.float32, device=dev)
        kw['head'] = ('predictor', torch.randn(3, C, device=dev), torch.randn(3, device=dev),
                      L.tensor_desc(pred, 1, 0, img_stride=3 * H * W, dtype=torch.float32))
    assert plan.resblock('rb', pcs[0], pcs[1], B, X, M, Y, (H, W), **kw)
    plan.finalize_workspace(dev)
    for _ in range(20):
        plan.run(s)
    torch.cuda.synchronize()
    fn(None, 0)
    plan.run(s)
    torch.cuda.synchronize()
    buf = np.zeros(256 * 8 * SLOTS, dtype=np.uint64)
    fn(buf.ctypes.data, buf.size)
    st = buf.reshape(256, 8, SLOTS).astype(np.int64)
    live = st[:, :, 0] > 0
    life = (st[:, :, 1] - st[:, :, 0])[live]
    print('resblock32%s %dx%dx%d: wave life median %.0f (min %d max %d) ticks of s_memtime' % (
        ' + head' if args.head else '', B, H, W, np.median(life), life.min(), life.max()))
    print('prologue (weights, first halo) median %.0f' % np.median((st[:, :, 2] - st[:, :, 0])[live]))

    def phases(t):
        a, b0, c1, b1, c2 = (st[:, :, 3 + 5 * t + i] for i in range(5))
        prev = st[:, :, 2] if t == 0 else st[:, :, 3 + 5 * (t - 1) + 4]
        ok = (a > 0) & (c2 > 0)
        return ok, (a - prev, b0 - a, c1 - b0, b1 - c1, c2 - b1, c2 - a)

    nt = max(t + 1 for t in range(MAXT) if (st[:, :, 3 + 5 * t] > 0).any())
    print('%d tiles per block; per wave, medians over blocks: gap  B0-wait  conv1  B1-wait  conv2  | tile' % nt)
    for name, tiles in (('first tile', [0]), ('steady tiles', list(range(1, nt)))):
        if not tiles:
            continue
        print(name)
        for w in range(8):
            cols = [[] for _ in range(6)]
            for t in tiles:
                ok, ph = phases(t)
                for c, p in zip(cols, ph):
                    c.extend(p[:, w][ok[:, w]].tolist())
            if cols[0]:
                print('  wave %d  %6.0f %6.0f %6.0f %6.0f %6.0f  | %6.0f' % ((w,) + tuple(np.median(c) for c in cols)))
    last = np.array([st[b, w, 3 + 5 * max(t for t in range(MAXT) if st[b, w, 3 + 5 * t] > 0) + 4]
                     for b, w in zip(*np.nonzero(live))])
    print('after the last tile (final stores, drain) median %.0f' % np.median(st[:, :, 1][live] - last))


if __name__ == '__main__':
    main()
