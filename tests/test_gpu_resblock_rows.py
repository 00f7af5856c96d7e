"""The row-rolling body of the fused 32-channel ResBlock (resblock32_kernel, csrc/rb32_sched.hpp) at the smallest
shapes at which it can go wrong: one tile whose every edge is a frame edge (conv1's zero padding, the zeroing of the
intermediate outside the frame), 2 x 2 tiles per frame (interior tile edges on all four sides; uncapped, and under a
block cap that leaves a partial last round), channel slices, the HEAD variant -- against the two dbsr_conv2d launches
the kernel replaces (bitwise where those ran conv3x3_ws, else atol = rtol = 1e-2) -- and one exact case that does not
depend on them: unit impulses at the frame corners, a tile corner and the strip and band seams, weights in {-1, 0, 1}
and integer biases, every intermediate and output an integer of magnitude <= 256 (exact in fp16 and bf16), required
equal to the fp32 torch reference."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

DEV = 'cuda'
pytestmark = pytest.mark.gpu
DTYPES = [torch.float16, torch.bfloat16]
C = 32


class _Slice:
    def __init__(self, t, c0):
        self.nhwc, self.c0 = t, c0

    def d(self, c0=0, fmap=None):
        return self.nhwc.d(self.c0 + c0) if fmap is None else self.nhwc.d(self.c0 + c0, fmap)


def _convs(gen):
    convs = []
    for _ in range(2):
        c = torch.nn.Conv2d(C, C, 3, padding=1)
        with torch.no_grad():
            c.weight.copy_(torch.randn(C, C, 3, 3, generator=gen) * (2.0 / (9 * C)) ** 0.5)
            c.bias.copy_(torch.randn(C, generator=gen) * 0.1)
        convs.append(c)
    return convs


def _pair(B, H, W, dt, seed, x_ld=C, x_c0=0, y_ld=C, y_c0=0, cap=0, head_cout=0):
    """(fused, two launches, kernels of the two launches): the block's output slice tensor, or with head_cout the
    head's fp32 NCHW output."""
    from dbsr_amd import _lib as L
    from dbsr_amd.engine import NHWC, PackedConv, Plan
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen)
    convs = _convs(gen)
    hw = torch.randn(max(head_cout, 1), C, generator=gen) * 0.2
    hb = torch.randn(max(head_cout, 1), generator=gen) * 0.1
    dev = torch.device(DEV)
    s = torch.cuda.current_stream().cuda_stream
    pcs = [PackedConv(c.to(dev), dt, dev, s) for c in convs]
    X = NHWC(B, H, W, x_ld, dt, dev)
    X.t[..., x_c0:x_c0 + C].copy_(x.permute(0, 2, 3, 1).to(dt))
    Xs = _Slice(X, x_c0)
    outs = {}
    for fused in (True, False):
        Y = NHWC(B, H, W, y_ld, dt, dev)
        Y.t.fill_(7.0)                                  # channels outside the slice stay untouched
        M = NHWC(B, H, W, C, dt, dev)
        kw = {}
        if head_cout:
            pred = torch.zeros(B, head_cout, H, W, dtype=torch.float32, device=dev)
            pdesc = L.tensor_desc(pred, 1, 0, img_stride=head_cout * H * W, dtype=torch.float32)
            kw['head'] = ('predictor', hw.to(dev), hb.to(dev), pdesc)
        plan = Plan()
        plan.max_blocks = cap
        # the conv head is the pipelined kernel's, which the default selection takes from 256 tiles on: the two
        # launches that carry it run under "pipelined wherever the shape allows" (algo 3; 2 is the default)
        pipelined = bool(head_cout) and not fused
        try:
            if pipelined:
                L.lib().dbsr_set_conv_algo(3)
            if fused:
                assert plan.resblock('rb', pcs[0], pcs[1], B, Xs, M, _Slice(Y, y_c0), (H, W), **kw), \
                    'dbsr_resblock_ok rejected'
            else:
                plan.conv('c1', pcs[0], B, Xs, 0, (H, W), M, 0, L.ACT_RELU)
                d = plan.conv('c2', pcs[1], B, M, 0, (H, W), _Slice(Y, y_c0), 0, L.ACT_NONE, res=Xs,
                              post_act=L.ACT_RELU, **kw)
                assert not head_cout or d.fused_head, 'the two-launch path did not carry the head'
                outs['kernels'] = set(plan.kernel.values())
            plan.finalize_workspace(dev)
            plan.run(s)
            torch.cuda.synchronize()
        finally:
            if pipelined:
                L.lib().dbsr_set_conv_algo(2)
        outs[fused] = pred.cpu() if head_cout else Y.t.cpu()
    return outs[True], outs[False], outs['kernels']


def _compare(f, t, kernels):
    if f.dtype != torch.float32 and kernels == {'conv3x3_ws'}:
        nd = int((f.view(torch.int16) != t.view(torch.int16)).sum())
        assert nd == 0, 'fused ResBlock differs from the two dbsr_conv2d launches at %d elements' % nd
    else:
        np.testing.assert_allclose(f.float().numpy(), t.float().numpy(), atol=1e-2, rtol=1e-2)


@pytest.mark.parametrize('dt', DTYPES)
def test_one_tile_frame(dt):
    """One frame of 16 x 32: one tile, every edge a frame edge."""
    f, t, kernels = _pair(1, 16, 32, dt, seed=1)
    _compare(f, t, kernels)


@pytest.mark.parametrize('cap', [0, 3])
@pytest.mark.parametrize('dt', DTYPES)
def test_two_by_two_tiles(dt, cap):
    """Two frames of 32 x 64: 8 tiles with interior edges on all four sides; under a cap of 3 blocks the last round
    is partial (3 + 3 + 2 tiles)."""
    f, t, kernels = _pair(2, 32, 64, dt, seed=2, cap=cap)
    _compare(f, t, kernels)


@pytest.mark.parametrize('dt', DTYPES)
def test_one_tile_channel_slices(dt):
    """The one-tile frame with x at channels 8 .. 39 of 48 and y at channels 8 .. 39 of 40."""
    f, t, kernels = _pair(1, 16, 32, dt, seed=3, x_ld=48, x_c0=8, y_ld=40, y_c0=8)
    _compare(f, t, kernels)
    mask = torch.ones(40, dtype=torch.bool)
    mask[8:8 + C] = False
    assert torch.all(f[..., mask].float() == 7.0)


@pytest.mark.parametrize('dt', DTYPES)
def test_head(dt):
    """The HEAD variant at 1 x 32 x 64 against conv1 + the conv carrying the fused head."""
    f, t, kernels = _pair(1, 32, 64, dt, seed=4, head_cout=3)
    _compare(f, t, kernels)


# (frame, row, column) of the unit impulses in two frames of 32 x 64 (2 x 2 tiles of 32 x 16), pairwise at least 5
# pixels apart inside a frame: the frame corners, the tile corner, the strip seams (tile columns 15 / 16 and 31 / 32,
# 33 -- the latter two are conv1's edge columns of the tile to the left) and the band seams (rows 3 / 4 and 4 / 5)
IMPULSES = [(0, 0, 0), (0, 0, 63), (0, 31, 0), (0, 31, 63), (0, 16, 32), (1, 15, 31),
            (0, 8, 15), (1, 8, 16), (0, 24, 31), (1, 24, 32), (1, 2, 33),
            (0, 3, 40), (0, 4, 46), (0, 5, 52), (1, 19, 8), (1, 20, 14), (1, 21, 20)]


def _exact_case():
    """x, the two integer convs and the fp32 reference (mid, out), all integers of magnitude <= 256."""
    for a, b in zip(IMPULSES, IMPULSES[1:] + IMPULSES[:1]):
        assert a != b
    for i, a in enumerate(IMPULSES):
        for b in IMPULSES[i + 1:]:
            assert a[0] != b[0] or max(abs(a[1] - b[1]), abs(a[2] - b[2])) >= 5, (a, b)
    x = torch.zeros(2, C, 32, 64)
    for i, (fr, r, c) in enumerate(IMPULSES):
        x[fr, (5 * i) % C, r, c] = 1.0
    density = 8
    while True:
        gen = torch.Generator().manual_seed(50 + density)
        convs = []
        for _ in range(2):
            c = torch.nn.Conv2d(C, C, 3, padding=1)
            with torch.no_grad():
                nz = torch.randint(0, density, (C, C, 3, 3), generator=gen) == 0
                sign = torch.randint(0, 2, (C, C, 3, 3), generator=gen) * 2 - 1
                c.weight.copy_((nz * sign).float())
                c.bias.copy_(torch.randint(-2, 3, (C,), generator=gen).float())
            convs.append(c)
        with torch.no_grad():
            mid = F.relu(convs[0](x))
            out = F.relu(convs[1](mid) + x)
        ok = all(bool(torch.all(v == v.round())) and float(v.abs().max()) <= 256 for v in (mid, out))
        if ok:
            return x, convs, mid, out
        density *= 2                                     # fewer nonzero weights
        assert density <= 256


@pytest.mark.parametrize('dt', DTYPES)
def test_exact_impulses(dt):
    from dbsr_amd.engine import NHWC, PackedConv, Plan
    x, convs, mid, ref = _exact_case()
    assert float(mid.abs().max()) > 0 and float(ref.abs().max()) > 1      # the case is not trivially zero
    dev = torch.device(DEV)
    s = torch.cuda.current_stream().cuda_stream
    pcs = [PackedConv(c.to(dev), dt, dev, s) for c in convs]
    X, M, Y = (NHWC(2, 32, 64, C, dt, dev) for _ in range(3))
    X.t.copy_(x.permute(0, 2, 3, 1).to(dt))
    plan = Plan()
    assert plan.resblock('rb', pcs[0], pcs[1], 2, X, M, Y, (32, 64)), 'dbsr_resblock_ok rejected'
    plan.finalize_workspace(dev)
    plan.run(s)
    torch.cuda.synchronize()
    got = Y.t.float().cpu()
    want = ref.permute(0, 2, 3, 1)
    nd = int((got != want).sum())
    assert nd == 0, 'resblock32 differs from the exact reference at %d elements, max |diff| %g' % (
        nd, float((got - want).abs().max()))
