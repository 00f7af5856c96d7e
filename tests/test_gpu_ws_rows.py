"""The row-rolling body of the weight-stationary kernel's 64-cout tiles (csrc/conv2d.hip ws_rows_body, kernel 4,
schedule csrc/ws_sched.hpp): a wave reads each halo-row fragment once, feeds the three output rows it touches and
finishes every row under the MFMAs of the rows below it.  Exact impulse responses pin the tap-to-row mapping, the
row-group seams between waves and the tile seams; the other cases -- one chunk and two, two cout tiles, a zero-padded
cin, every epilogue, long tile walks with a capped grid, a partial last round, one-tile-high frames -- are held to the
tolerance of tests/test_gpu_ks128.py against torch fp32 on the same 16-bit-rounded operands."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float16, torch.bfloat16]
V1616, V1608 = 4001616, 4001608


def _ulp(dt):
    return 2.0 ** (-10 if dt == torch.float16 else -7)


def _check(out, ref, dt):
    ulp = _ulp(dt)
    err = (out - ref).abs()
    print('max err %.3g ulp, mean err %.4g ulp' % (err.max() / ulp, err.mean() / ulp))
    np.testing.assert_allclose(out.numpy(), ref.numpy(), atol=4 * ulp, rtol=2 * ulp)
    assert err.mean() < 0.25 * ulp


def _ran(variant):
    from dbsr_amd import ops
    assert ops.conv2d.last_kernel == 4 and ops.conv2d.last_variant == variant, \
        (ops.conv2d.last_kernel, ops.conv2d.last_variant)


@functools.lru_cache(maxsize=None)
def _int_weights():
    """Distinct small integers per (cout, cin, tap) neighbourhood, |w| <= 64: exact in fp16 and in bf16, and so is
    every product with a 1.0 input; a one-hot input puts exactly one product into each output."""
    co = torch.arange(64).view(64, 1, 1)
    ci = torch.arange(64).view(1, 64, 1)
    tap = torch.arange(9).view(1, 1, 9)
    w = (co * 37 + ci * 11 + tap * 5) % 129 - 64
    assert int(w.abs().max()) <= 64
    # taps differ at every (cout, cin); neighbouring couts and cins differ at every tap
    assert all(len(set(w[c, k].tolist())) == 9 for c in (0, 33, 63) for k in (0, 31, 32, 63))
    return w.view(64, 64, 3, 3).float()


# 48 x 48 frames: 16 x 16 tiles have seams at rows / columns 16, 32 and a wave's 4-row groups at rows 4, 8, 12;
# 16 x 8 tiles have seams at rows 8, 16, ... and 2-row groups
IMPULSES_1616 = [
    ('corner', (0, 0, 0, 0)),              # frame corner: both halos out of frame
    ('corner_far', (15, 63, 47, 47)),
    ('interior', (3, 41, 21, 27)),         # inside tile (1, 1)
    ('tile_row15', (5, 32, 15, 30)),       # last row of a tile: feeds the tile below through its halo row 0
    ('tile_row16_col16', (9, 31, 16, 16)),  # first row and first column of the next tile
    ('wave_seam_row3', (7, 5, 3, 9)),      # last row of wave row-group 0: feeds group 1 through its halo row 0
    ('wave_seam_row4', (11, 60, 4, 40)),   # first row of group 1: feeds group 0 through its halo row RPW + 1
]
IMPULSES_1608 = [
    ('corner', (0, 0, 0, 0)),
    ('corner_far', (7, 63, 47, 47)),
    ('interior', (3, 41, 21, 27)),
    ('tile_row7', (5, 32, 7, 30)),
    ('tile_row8_col16', (6, 31, 8, 16)),
    ('wave_seam_row1', (2, 5, 1, 9)),
    ('wave_seam_row2', (4, 60, 2, 40)),
]


def _impulse(dt, N, pos, variant):
    from dbsr_amd import ops
    f, c, y, x0 = pos
    x = torch.zeros(N, 64, 48, 48)
    x[f, c, y, x0] = 1.0
    w = _int_weights()
    ref = F.conv2d(x, w, None, padding=1)
    out = ops.conv2d(x.to(DEV), w.to(DEV), None, padding=1, compute_dtype=dt).float().cpu()
    _ran(variant)
    assert int((ref != 0).sum()) > 0
    assert torch.equal(out, ref), (out != ref).nonzero()[:8].tolist()


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name,pos', IMPULSES_1616, ids=[i[0] for i in IMPULSES_1616])
def test_impulse_exact_16x16(dt, name, pos):
    """64 -> 64 on 16 frames of 48 x 48: 144 tiles of 16 x 16."""
    _impulse(dt, 16, pos, V1616)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name,pos', IMPULSES_1608, ids=[i[0] for i in IMPULSES_1608])
def test_impulse_exact_16x8(dt, name, pos):
    """64 -> 64 on 8 frames of 48 x 48: under 128 tiles of 16 x 16, so 144 tiles of 16 x 8."""
    _impulse(dt, 8, pos, V1608)


@functools.lru_cache(maxsize=None)
def _operands(N, cin, cout, H, W, seed, res_frames=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=gen)
    w = torch.randn(cout, cin, 3, 3, generator=gen) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=gen) * 0.1
    res = torch.randn(res_frames, cout, H, W, generator=gen) if res_frames else None
    return x, w, b, res


def _conv_ref(x, w, b, dt):
    return F.conv2d(x.to(dt).float(), w.to(dt).float(), b, padding=1)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('cin,cout,variant', [(32, 64, V1616), (64, 128, V1616), (40, 64, V1608)],
                         ids=['one_chunk', 'two_cout_tiles', 'cin40_padded'])
def test_chunks_and_couts(dt, cin, cout, variant):
    """16 frames of 32 x 32: cin 32 is one 32-channel chunk (NCH 1); cout 128 is two cout tiles (128 tiles of
    16 x 16); cin 40 is zero-padded to two chunks (64 tiles of 16 x 16, so the 16 x 8 tile)."""
    from dbsr_amd import ops
    x, w, b, _ = _operands(16, cin, cout, 32, 32, 100 + cin + cout)
    ref = F.relu(_conv_ref(x, w, b, dt))
    out = ops.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1, act=1, compute_dtype=dt).float().cpu()
    _ran(variant)
    _check(out, ref, dt)


EPILOGUES = ['bias_relu', 'res_relu', 'plain', 'leaky_res_leaky']


def _epilogue_case(dt, N, variant, epi, max_blocks=0, seed=7):
    from dbsr_amd import ops
    x, w, b, res = _operands(N, 64, 64, 48, 48, seed, res_frames=N)
    c = _conv_ref(x, w, b, dt)
    r = res.to(dt).float()
    kw = dict(padding=1, compute_dtype=dt)
    if max_blocks:
        kw['max_blocks'] = max_blocks
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    if epi == 'bias_relu':
        ref, out = F.relu(c), ops.conv2d(xd, wd, bd, act=1, **kw)
    elif epi == 'res_relu':
        ref, out = F.relu(c + r), ops.conv2d(xd, wd, bd, act=0, residual=res.to(DEV), post_act=1, **kw)
    elif epi == 'plain':
        ref, out = c, ops.conv2d(xd, wd, bd, **kw)
    else:
        ref = F.leaky_relu(F.leaky_relu(c, 0.1) + r, 0.1)
        out = ops.conv2d(xd, wd, bd, act=2, residual=res.to(DEV), post_act=2, **kw)
    _ran(variant)
    _check(out.float().cpu(), ref, dt)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('epi', EPILOGUES)
@pytest.mark.parametrize('N,variant', [(16, V1616), (8, V1608)], ids=['16x16', '16x8'])
def test_epilogues(dt, epi, N, variant):
    _epilogue_case(dt, N, variant, epi)


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('epi', ['bias_relu', 'res_relu'])
def test_long_walk(dt, epi):
    """144 tiles on 16 blocks: 9 tiles per block, so both halo buffers and the residual path are reused."""
    _epilogue_case(dt, 16, V1616, epi, max_blocks=16)


@pytest.mark.parametrize('dt', DTYPES)
def test_partial_last_round(dt):
    """17 frames: 153 tiles on 16 blocks, nine blocks walk 10 tiles and seven walk 9."""
    _epilogue_case(dt, 17, V1616, 'res_relu', max_blocks=16, seed=17)


def test_broadcast_residual():
    """One residual frame per group of frames through the residual's frame map: Plan.conv(..., rmap=(G, 1, 0, 0))."""
    from dbsr_amd import _lib as L
    from dbsr_amd import ops
    from dbsr_amd.engine import NHWC, PackedConv, Plan
    dt = torch.float16
    N, H, W, G = 16, 48, 48, 4
    R = N // G
    x, w, b, res = _operands(N, 64, 64, H, W, 44, res_frames=R)
    conv = torch.nn.Conv2d(64, 64, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    dev = torch.device(DEV)
    s = torch.cuda.current_stream().cuda_stream
    pc = PackedConv(conv.to(dev), dt, dev, s)
    X, RS, Y = NHWC(N, H, W, 64, dt, dev), NHWC(R, H, W, 64, dt, dev), NHWC(N, H, W, 64, dt, dev)
    X.t.copy_(x.permute(0, 2, 3, 1).to(dt))
    RS.t.copy_(res.permute(0, 2, 3, 1).to(dt))
    plan = Plan()
    d = plan.conv('bcast', pc, N, X, 0, (H, W), Y, 0, L.ACT_NONE, res=RS, rmap=(G, 1, 0, 0), post_act=L.ACT_RELU)
    assert L.lib().dbsr_conv_kernel_for(d) == 4 and L.lib().dbsr_conv_dispatch_variant(d) == V1616
    plan.finalize_workspace(dev)
    plan.run(s)
    torch.cuda.synchronize()
    out = Y.t.float().cpu().permute(0, 3, 1, 2)
    rr = res.to(dt).float()[torch.arange(N) // G]
    _check(out, F.relu(_conv_ref(x, w, b, dt) + rr), dt)
    # the same conv through ops.conv2d with the residual expanded: the same kernel, the same bytes
    out2 = ops.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1, act=0, residual=rr.to(DEV), post_act=1,
                      compute_dtype=dt).float().cpu()
    _ran(V1616)
    assert torch.equal(out, out2)


@pytest.mark.parametrize('dt', DTYPES)
def test_one_tile_high_frames(dt):
    """48 frames of 16 x 48: 144 tiles of 16 x 16, both vertical halo rows out of frame for every tile."""
    from dbsr_amd import ops
    N, H, W = 48, 16, 48
    x, w, b, res = _operands(N, 64, 64, H, W, 5, res_frames=N)
    ref = F.relu(_conv_ref(x, w, b, dt) + res.to(dt).float())
    out = ops.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1, act=0, residual=res.to(DEV), post_act=1,
                     compute_dtype=dt).float().cpu()
    _ran(V1616)
    _check(out, ref, dt)
