"""Generate tests/golden/conv_dispatch.npz: what the host queries of dbsr_conv2d's dispatch answer for a fixed
synthetic grid of descriptors (host logic only: no GPU, no reference code).

Recorded per descriptor, through the public C ABI alone: dbsr_conv_kernel_for, dbsr_conv_dispatch_variant,
dbsr_conv_workspace_bytes, dbsr_conv_lane_reach for which = 0, 1, 2 and dbsr_conv_head_ok.  The file pins the
dispatch across refactors of csrc/conv2d.hip: it is written from a library built at the commit whose decisions are
to be kept and tests/test_conv_dispatch_table.py asks the current library for the same answers.  Without a device
the library plans for 256 CUs, an MI355X's count, so the table is the same with and without one.

Left out of the grid: precise descriptors with an fp32 input.  For those the queries of the commit this table was
recorded at reported the precise pixel tile and no workspace while dbsr_conv2d launched the generic kernel on
pick_generic_tile's tile, split where the workspace allows; the launch is what the queries follow since.

Usage:  DBSR_HIP_LIB=<that commit's libdbsr_hip.so> PYTHONDONTWRITEBYTECODE=1 \
            python tests/golden/make_golden_conv_dispatch.py
"""
import ctypes
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))

import numpy as np  # noqa: E402

F32, BF16, F16 = 0, 1, 2
# (n_frames, in_h, in_w)
FRAMES = [(104, 1, 1), (1, 8, 8), (1, 16, 16), (104, 16, 16), (8, 48, 48), (112, 48, 48), (1, 256, 256),
          (8, 128, 128), (1, 384, 384)]
# (k, stride, pad, dil)
K3, K3D2, K3D4, K3D8, K3S2, K1 = (3, 1, 1, 1), (3, 1, 2, 2), (3, 1, 4, 4), (3, 1, 8, 8), (3, 2, 1, 1), (1, 1, 0, 1)
SHAPES = [K3, K3D2, K3D4, K3D8, K3S2, K1]
CINS = [8, 16, 32, 64, 96, 128, 256, 512]
COUTS = [4, 16, 24, 32, 64, 80, 128, 512]
# output modes: NHWC, fp32 NCHW, PixelShuffle(4) / (8) of 32 channels (cout = 32 s^2), precise (fp32 NCHW)
NHWC, NCHW, SHUF4, SHUF8, PRECISE = range(5)
# epilogues: plain, residual + post-ReLU, gate
PLAIN, RES, GATE = range(3)
# plan_h: unset, out_h, a whole image twice the slab's rows, a whole image 4 rows taller than the slab (the slab's
# rows then do not tile: a misfit wherever the tile chosen for the whole image is taller than 4 rows)
PLAN_0, PLAN_SELF, PLAN_X2, PLAN_ODD = range(4)
# y / residual / gate slices: [0, cout) of a pixel as wide; an aligned slice inside a wider pixel; a misaligned one
TIGHT, WIDE, SKEW = range(3)
# (epilogue, max_blocks, plan, slice) beside the base grid's (PLAIN, 0, PLAN_0, TIGHT)
SIDE = [(e, mb, pl, sl) for e in (PLAIN, RES, GATE)
        for mb, pl, sl in ((0, PLAN_0, TIGHT), (128, PLAN_0, TIGHT), (0, PLAN_SELF, TIGHT), (0, PLAN_X2, TIGHT),
                           (0, PLAN_ODD, TIGHT), (128, PLAN_X2, TIGHT), (0, PLAN_0, WIDE), (128, PLAN_ODD, WIDE),
                           (0, PLAN_0, SKEW))][1:]
COLS = ('dtype', 'k', 'stride', 'pad', 'dil', 'cin', 'cout', 'n', 'h', 'w', 'mode', 'epi', 'max_blocks', 'plan',
        'slice', 'algo')
OUT = ('kernel_for', 'dispatch_variant', 'workspace_bytes', 'reach_y', 'reach_res', 'reach_gate', 'head_ok')


def rows():
    """The grid, one tuple of COLS per descriptor, in a fixed order."""
    r = []

    def add(dt, shape, cin, cout, frame, mode=NHWC, epi=PLAIN, mb=0, plan=PLAN_0, sl=TIGHT, algo=2):
        r.append((dt,) + shape + (cin, cout) + frame + (mode, epi, mb, plan, sl, algo))

    # every dtype, conv shape, channel count and frame under the default selection
    for dt in (BF16, F16, F32):
        for shape in SHAPES:
            for cin in CINS:
                for cout in COUTS:
                    for fr in FRAMES:
                        add(dt, shape, cin, cout, fr)
    # epilogues, the CU cap, plan_h and the slices: the 16-bit kernels' shapes (fp16 on every third descriptor) ...
    i = 0
    for shape in (K3, K1):
        for cin in CINS:
            for cout in COUTS:
                for fr in FRAMES:
                    for side in SIDE:
                        i += 1
                        for dt in (BF16, F16) if i % 3 == 0 else (BF16,):
                            add(dt, shape, cin, cout, fr, NHWC, *side)
    # ... and plan_h for the LDS-tiled and generic kernels' tiles and splits (fp32; a dilated 16-bit conv)
    for dt, shape in ((F32, K3), (BF16, K3D2)):
        for cin in CINS:
            for cout in COUTS:
                for fr in FRAMES:
                    for plan in (PLAN_SELF, PLAN_X2, PLAN_ODD):
                        add(dt, shape, cin, cout, fr, plan=plan)
    # fp32 NCHW output; precise heads (16-bit inputs only: see the module docstring); the PixelShuffle upsampler
    for dt in (BF16, F16, F32):
        for shape in SHAPES:
            for cin in CINS:
                for cout in (4, 16, 32):
                    for fr in FRAMES:
                        add(dt, shape, cin, cout, fr, NCHW)
    for dt in (BF16, F16):
        for shape in (K3, K1):
            for cin in CINS:
                for cout in (4, 16):
                    for fr in FRAMES:
                        for plan in (PLAN_0, PLAN_X2):
                            add(dt, shape, cin, cout, fr, PRECISE, plan=plan)
    for dt in (BF16, F16, F32):
        for mode, cout in ((SHUF4, 512), (SHUF8, 2048)):
            for cin in (32, 64, 128, 256):
                for fr in FRAMES:
                    add(dt, K1, cin, cout, fr, mode)
    # the other dbsr_set_conv_algo settings
    for algo in (0, 1, 3, 4, 5):
        for shape in (K3, K3D2, K1):
            for cin in CINS:
                for cout in COUTS:
                    for fr in FRAMES:
                        for epi in (PLAIN, RES):
                            add(BF16, shape, cin, cout, fr, epi=epi, algo=algo)
    return r


def desc(L, row):
    """The dbsr_conv_desc of a row.  The queries read no memory, so every pointer is a dummy."""
    c = dict(zip(COLS, row))
    ident = L.FrameMap(1, 1, 0, 1)
    cinp = (c['cin'] + 7) // 8 * 8 if c['cin'] <= 16 else (c['cin'] + 31) // 32 * 32
    d = L.ConvDesc()
    d.n_frames, d.in_h, d.in_w = c['n'], c['h'], c['w']
    d.cin, d.cout, d.kh, d.kw = c['cin'], c['cout'], c['k'], c['k']
    d.stride, d.pad, d.dil = c['stride'], c['pad'], c['dil']
    d.out_h = (c['h'] + 2 * c['pad'] - c['dil'] * (c['k'] - 1) - 1) // c['stride'] + 1
    d.out_w = (c['w'] + 2 * c['pad'] - c['dil'] * (c['k'] - 1) - 1) // c['stride'] + 1
    if c['plan'] == PLAN_ODD:                 # the slab: all but the whole image's last 4 rows
        d.plan_h = d.out_h
        d.out_h -= 4
        d.in_h -= 4 * c['stride']
    elif c['plan'] != PLAN_0:
        d.plan_h = d.out_h * (2 if c['plan'] == PLAN_X2 else 1)
    d.x = L.Tensor(1, c['dtype'], c['h'] * c['w'] * cinp, cinp, 0, ident)
    d.w = 1
    cout8 = (c['cout'] + 7) // 8 * 8
    c0, ld = {TIGHT: (0, cout8), WIDE: (8, (c['cout'] + 63) // 64 * 64 + 64), SKEW: (4, cout8 + 4)}[c['slice']]
    ydt = F32 if c['mode'] in (NCHW, PRECISE) else c['dtype']
    if c['mode'] in (SHUF4, SHUF8):
        ld = 32
        d.shuffle = 4 if c['mode'] == SHUF4 else 8
    d.out_mode = {NHWC: L.OUT_NHWC, NCHW: L.OUT_NCHW_F32, PRECISE: L.OUT_NCHW_F32}.get(c['mode'], L.OUT_SHUFFLE)
    d.precise = 1 if c['mode'] == PRECISE else 0
    npx = max(d.out_h, 1) * max(d.out_w, 1) * max(d.shuffle, 1) ** 2
    d.y = L.Tensor(1, ydt, npx * ld, ld, c0, ident)
    if c['epi'] == RES:
        d.res = L.Tensor(1, ydt, npx * ld, ld, c0, ident)
        d.act, d.post_act = L.ACT_NONE, L.ACT_RELU
    elif c['epi'] == GATE:
        d.gate = L.Tensor(1, ydt, npx * ld, ld, c0, ident)
    d.max_blocks = c['max_blocks']
    return d


def valid(row):
    """Rows whose geometry exists (the odd slab needs rows to drop)."""
    c = dict(zip(COLS, row))
    out_h = (c['h'] + 2 * c['pad'] - c['dil'] * (c['k'] - 1) - 1) // c['stride'] + 1
    return c['plan'] != PLAN_ODD or out_h > 4


def table(L):
    """(rows [N, len(COLS)] int32, answers [N, len(OUT)] int64) of the loaded library, the selection left at 2."""
    lib = L.lib()
    rs = [r for r in rows() if valid(r)]
    out = np.zeros((len(rs), len(OUT)), np.int64)
    algo = 2
    try:
        for i, r in enumerate(rs):
            if r[-1] != algo:
                algo = r[-1]
                assert lib.dbsr_set_conv_algo(algo) == 0
            d = ctypes.byref(desc(L, r))
            out[i] = (lib.dbsr_conv_kernel_for(d), lib.dbsr_conv_dispatch_variant(d),
                      lib.dbsr_conv_workspace_bytes(d), lib.dbsr_conv_lane_reach(d, 0),
                      lib.dbsr_conv_lane_reach(d, 1), lib.dbsr_conv_lane_reach(d, 2), lib.dbsr_conv_head_ok(d))
    finally:
        lib.dbsr_set_conv_algo(2)
    return np.array(rs, np.int32), out


def check_coverage(rs, out):
    """The table exercises every kernel, tile and fallback the dispatch can choose."""
    col = {n: rs[:, i] for i, n in enumerate(COLS)}
    kf, var, wsb = out[:, 0], out[:, 1] % 1000000, out[:, 2]
    plain = col['mode'] != PRECISE
    assert set(kf.tolist()) == set(range(9)), sorted(set(kf.tolist()))
    assert set(var[kf == 2].tolist()) == {1, 2, 3, 4}, 'pipelined tile configs'
    assert set(var[kf == 4].tolist()) == {6408, 1608, 1616}, 'weight-stationary variants'
    tiled = var[kf == 1]
    assert set((tiled % 100000).tolist()) == {64064, 32128, 32064, 32016}, 'LDS tiles'
    assert (tiled >= 200000).any() and (wsb[kf == 1] > 0).any(), 'a tiled K split'
    gen = var[(kf == 0) & plain]
    assert (gen % 1000 > 1).any() and (wsb[(kf == 0) & plain] > 0).any(), 'a generic K split'
    assert set(var[~plain].tolist()) == {1, 2, 4}, 'precise pixel tiles'
    sl = col['slice']
    c0 = np.where(sl == WIDE, 8, np.where(sl == SKEW, 4, 0))
    for which in range(3):
        assert (out[:, 3 + which] != c0 + col['cout'] - 1).any(), which
    assert (out[:, 4] > c0 + col['cout'] - 1).any(), 'a residual run past cout (weight-stationary partial tile)'
    assert (out[:, 6] == 1).any() and (col['plan'] == PLAN_ODD).any()
    assert set(col['algo'].tolist()) == set(range(6))


def main():
    sys.path.insert(0, REPO)
    from dbsr_amd import _lib as L
    rs, out = table(L)
    check_coverage(rs, out)
    path = os.path.join(HERE, 'conv_dispatch.npz')
    np.savez_compressed(path, rows=rs, out=out)
    assert os.path.getsize(path) <= 997059, 'larger than the largest fixture here (variants.part0.npz): thin the grid'
    print('%d descriptors from %s -> %s (%d bytes)' % (len(rs), L.LIB_PATH, path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
