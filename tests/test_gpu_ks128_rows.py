"""The row-rolling body of the 128 -> 128 weight-stationary kernel (csrc/conv128.hip, kernel 7): every wave holds 16
couts over the whole K, reads each halo-row fragment once and feeds the three output rows it touches.  Exact impulse
responses pin the tap-to-row mapping and the cout gather; degenerate frames, a long tile walk (every halo buffer
reused, plain and broadcast residual) and the zero-padded cin of pwc.dec2.dense0 are held to the tolerance of
tests/test_gpu_ks128.py against torch fp32 on the same 16-bit-rounded operands."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DTYPES = [torch.float16, torch.bfloat16]


def _ulp(dt):
    return 2.0 ** (-10 if dt == torch.float16 else -7)


def _check(out, ref, dt):
    ulp = _ulp(dt)
    err = (out - ref).abs()
    print('max err %.3g ulp, mean err %.4g ulp' % (err.max() / ulp, err.mean() / ulp))
    np.testing.assert_allclose(out.numpy(), ref.numpy(), atol=4 * ulp, rtol=2 * ulp)
    assert err.mean() < 0.25 * ulp


def _int_weights():
    """Distinct small integers per (cout, cin, tap) neighbourhood, |w| <= 64: exact in fp16 and in bf16, and so is
    every product with a 1.0 input; a one-hot input puts exactly one product into each output."""
    co = torch.arange(128).view(128, 1, 1)
    ci = torch.arange(128).view(1, 128, 1)
    tap = torch.arange(9).view(1, 1, 9)
    w = (co * 37 + ci * 11 + tap * 5) % 129 - 64
    assert int(w.abs().max()) <= 64
    # taps differ at every (cout, cin); neighbouring couts and cins differ at every tap
    assert all(len(set(w[c, k].tolist())) == 9 for c in (0, 77, 127) for k in (0, 50, 127))
    return w.view(128, 128, 3, 3).float()


# (N, H, W) = (16, 32, 64): 256 tiles of 16 x 8, tile seams at rows 8, 16, 24 and columns 16, 32, 48
IMPULSES = [
    ('corner', (0, 0, 0, 0)),              # frame corner: both halos out of frame
    ('corner_far', (15, 127, 31, 63)),
    ('interior', (3, 41, 11, 21)),         # inside tile (1, 1)
    ('seam_row7', (5, 64, 7, 30)),         # last row of a tile: feeds the tile below through its halo row 0
    ('seam_row8', (9, 101, 8, 16)),        # first row and first column of a tile
]


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('name,pos', IMPULSES, ids=[i[0] for i in IMPULSES])
def test_impulse_exact(dt, name, pos):
    from dbsr_amd import ops
    N, H, W = 16, 32, 64
    f, c, y, x0 = pos
    x = torch.zeros(N, 128, H, W)
    x[f, c, y, x0] = 1.0
    w = _int_weights()
    ref = F.conv2d(x, w, None, padding=1)
    out = ops.conv2d(x.to(DEV), w.to(DEV), None, padding=1, compute_dtype=dt).float().cpu()
    assert ops.conv2d.last_kernel == 7 and ops.conv2d.last_variant == 7001608
    assert int((ref != 0).sum()) > 0
    assert torch.equal(out, ref), (name, (out != ref).nonzero()[:8].tolist())


def _operands(N, cin, H, W, seed, res_frames=0):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(N, cin, H, W, generator=gen)
    w = torch.randn(128, cin, 3, 3, generator=gen) / (cin * 9) ** 0.5
    b = torch.randn(128, generator=gen) * 0.1
    res = torch.randn(res_frames, 128, H, W, generator=gen) if res_frames else None
    return x, w, b, res


@pytest.mark.parametrize('dt', DTYPES)
@pytest.mark.parametrize('shape', [(32, 8, 64), (64, 16, 16)], ids=['one_tile_row', 'one_tile_column'])
def test_degenerate_frames(dt, shape):
    """128 tiles each, the smallest the selector accepts: a single tile row (both vertical halos out of frame) and
    a single tile column."""
    from dbsr_amd import ops
    N, H, W = shape
    x, w, b, _ = _operands(N, 128, H, W, 5 + H)
    ref = F.relu(F.conv2d(x.to(dt).float(), w.to(dt).float(), b, padding=1))
    out = ops.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1, act=1, compute_dtype=dt).float().cpu()
    assert ops.conv2d.last_kernel == 7 and ops.conv2d.last_variant == 7001608
    _check(out, ref, dt)


@pytest.mark.parametrize('dt', DTYPES)
def test_long_tile_walk_residual(dt):
    """774 tiles: three full rounds and a partial one on 256 CUs, so both halo buffers are reused."""
    from dbsr_amd import ops
    N, H, W = 43, 48, 48
    x, w, b, res = _operands(N, 128, H, W, 43, res_frames=N)
    ref = F.relu(F.conv2d(x.to(dt).float(), w.to(dt).float(), b, padding=1) + res.to(dt).float())
    out = ops.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1, act=0, residual=res.to(DEV), post_act=1,
                     compute_dtype=dt).float().cpu()
    assert ops.conv2d.last_kernel == 7 and ops.conv2d.last_variant == 7001608
    _check(out, ref, dt)


def test_long_tile_walk_broadcast_residual():
    """merge.wp.init's form: one residual frame per group of frames, Plan.conv(..., res=..., rmap=(G, 1, 0, 0))."""
    from dbsr_amd import _lib as L
    from dbsr_amd import ops
    from dbsr_amd.engine import NHWC, PackedConv, Plan
    dt = torch.float16
    N, H, W, G = 43, 48, 48, 7
    R = (N + G - 1) // G
    x, w, b, res = _operands(N, 128, H, W, 44, res_frames=R)
    conv = torch.nn.Conv2d(128, 128, 3, padding=1)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(b)
    dev = torch.device(DEV)
    s = torch.cuda.current_stream().cuda_stream
    pc = PackedConv(conv.to(dev), dt, dev, s)
    X, RS, Y = NHWC(N, H, W, 128, dt, dev), NHWC(R, H, W, 128, dt, dev), NHWC(N, H, W, 128, dt, dev)
    X.t.copy_(x.permute(0, 2, 3, 1).to(dt))
    RS.t.copy_(res.permute(0, 2, 3, 1).to(dt))
    plan = Plan()
    d = plan.conv('init', pc, N, X, 0, (H, W), Y, 0, L.ACT_NONE, res=RS, rmap=(G, 1, 0, 0), post_act=L.ACT_RELU)
    assert L.lib().dbsr_conv_kernel_for(d) == 7 and L.lib().dbsr_conv_dispatch_variant(d) == 7001608
    plan.finalize_workspace(dev)
    plan.run(s)
    torch.cuda.synchronize()
    out = Y.t.float().cpu().permute(0, 3, 1, 2)
    rr = res.to(dt).float()[torch.arange(N) // G]
    ref = F.relu(F.conv2d(x.to(dt).float(), w.to(dt).float(), b, padding=1) + rr)
    _check(out, ref, dt)
    # the same conv through ops.conv2d with the residual expanded: the same kernel, the same bytes
    out2 = ops.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1, act=0, residual=rr.to(DEV), post_act=1,
                      compute_dtype=dt).float().cpu()
    assert ops.conv2d.last_kernel == 7
    assert torch.equal(out, out2)


@pytest.mark.parametrize('dt', DTYPES)
def test_cin_117_leaky(dt):
    """pwc.dec2.dense0's shape: cin 117 (the packer zero-pads to 128), 104 frames of 16 x 16 (208 tiles), the
    run-time leaky-ReLU epilogue."""
    from dbsr_amd import ops
    N, H, W = 104, 16, 16
    x, w, b, _ = _operands(N, 117, H, W, 117)
    ref = F.leaky_relu(F.conv2d(x.to(dt).float(), w.to(dt).float(), b, padding=1), 0.1)
    out = ops.conv2d(x.to(DEV), w.to(DEV), b.to(DEV), padding=1, act=2, compute_dtype=dt).float().cpu()
    assert ops.conv2d.last_kernel == 7 and ops.conv2d.last_variant == 7001608
    _check(out, ref, dt)
