"""Op-level tests of the per-op PWC-Net kernels (csrc/pwc_ops.hip: dbsr_correlation, dbsr_backwarp,
dbsr_conv_transpose_k4s2, dbsr_pwc_assemble -- what every frame size whose padded size is not 64x64 runs, in 16 bit)
and of the glue ops at either end of the alignment path and around the merge (dbsr_pack_burst, dbsr_flow_finalize,
dbsr_merge_prep forward, dbsr_burst_mean), each against plain torch on the CPU in float64 on the same rounded
operands with the single-rounding bound of tests/pwc_ref.py (0.5 u + A in 16 bit, A alone in fp32; n_r is read off
each kernel and written next to its test), bitwise where the op is a copy or a single rounding.

Output buffers are prefilled with 3.0 and everything an op does not write must still be 3.0; input pad channels that
a kernel must not read, or reads against zero-padded weights, hold 1.5 (never NaN)."""
import types

import pytest
import torch
import torch.nn.functional as F

from tests.pwc_ref import (SENTINEL, assert_bitwise, assert_sentinel, assert_single_rounding, backwarp64,
                           correlation64, lrelu, mask_ambiguous, nchw)

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DT = [torch.float16, torch.bfloat16, torch.float32]
IDS = ['fp16', 'bf16', 'fp32']
PAD_VALUE = 1.5


def _seed(*key):
    s = 0
    for ch in '|'.join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _lib():
    from dbsr_amd import _lib as L
    return L, L.lib(), L.stream_ptr(DEV)


def _put(x, dtype, ld, c0=0, fill=PAD_VALUE):
    """x [n, h, w, c] (CPU) as channels [c0, c0 + c) of a device buffer [n, h, w, ld] of dtype, `fill` elsewhere."""
    buf = torch.full(x.shape[:-1] + (ld,), fill, dtype=dtype, device=DEV)
    buf[..., c0:c0 + x.shape[-1]] = x.to(DEV)
    return buf


def _out(shape, dtype):
    return torch.full(shape, SENTINEL, dtype=dtype, device=DEV)


def _desc(L, buf, c0=0, fmap=(1, 1, 0, 1)):
    return L.tensor_desc(buf, buf.shape[-1], c0, fmap=fmap)


def _untouched(buf, lo, hi, what):
    """Channels outside [lo, hi) of an output buffer are still the sentinel."""
    b = buf.cpu()
    if lo > 0:
        assert_sentinel(b[..., :lo], what + ': channels in front')
    if hi < b.shape[-1]:
        assert_sentinel(b[..., hi:], what + ': channels behind')


def _feat(shape, dtype, g):
    """Seeded features rounded to dtype, as [n, h, w, c] fp32 on the CPU."""
    n, c, h, w = shape
    return torch.randn(n, h, w, c, generator=g).to(dtype).float()


# ----------------------------------------------------------------------------------------------------
# dbsr_correlation
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('leaky', [0, 1], ids=['plain', 'leaky'])
@pytest.mark.parametrize('aligned', [True, False], ids=['vec', 'scalar'])
@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('shape', [(3, 196, 1, 1), (2, 128, 2, 2), (2, 32, 16, 16), (1, 20, 5, 7)])
def test_correlation(shape, dtype, aligned, leaky):
    """n_r = C fmaf (one chain over the channels, 8-wide loads when ld and c0 are multiples of 8, scalar otherwise;
    C = 20 takes 16 channels 8-wide and 4 one by one) + the division by C + the LeakyReLU (0.1f and the product).
    Pad channels of the inputs hold 1.5 and must not be read; only the 81 output channels are written."""
    L, lib, stream = _lib()
    n, C, h, w = shape
    g = _seed('corr', shape, dtype)
    a, b = _feat(shape, dtype, g), _feat(shape, dtype, g)
    ld = (C + 7) // 8 * 8 + (8 if aligned else 3)
    c0 = 0 if aligned else 1
    A_, B_ = _put(a, dtype, ld, c0), _put(b, dtype, ld, c0)
    oc0 = 0 if aligned else 5
    out = _out((n, h, w, 88 + oc0), dtype)
    L.check(lib.dbsr_correlation(n, h, w, C, _desc(L, A_, c0), _desc(L, B_, c0), _desc(L, out, oc0), leaky, stream),
            'dbsr_correlation')
    torch.cuda.synchronize()
    _untouched(out, oc0, oc0 + 81, 'correlation')
    vol, S = correlation64(nchw(a), nchw(b))
    assert_single_rounding(nchw(out[..., oc0:oc0 + 81]), lrelu(vol) if leaky else vol, S / C, C + 1 + 2 * leaky, dtype,
                           'correlation %s %s' % (shape, dtype))


# ----------------------------------------------------------------------------------------------------
# dbsr_backwarp
# ----------------------------------------------------------------------------------------------------
def _flows(kind, n, h, w, scale, g):
    """[n, h, w, 2] fp32 flows: 'rand' a few pixels; 'far' +-1.5 x the level size (most samples outside, mask 0);
    'ident' zero; 'shift' the exact integer shift (2, -3): backwarp normalises by (W - 1) / 2 and grid_sample maps
    back by W / 2, so a flow f moves the sample by f W / (W - 1) pixels and the integer shift needs
    f = 2 (W - 1) / W (exact in fp32 for the power-of-two sizes used, scale 1)."""
    if kind == 'ident':
        return torch.zeros(n, h, w, 2)
    if kind == 'shift':
        return torch.tensor([2.0 * (w - 1) / w, -3.0 * (h - 1) / h]).expand(n, h, w, 2).contiguous()
    amp = torch.tensor([w, h]) * (0.25 if kind == 'rand' else 1.5) / scale
    fl = torch.randn(n, h, w, 2, generator=g) * amp
    if kind == 'far':
        # each component: +-1.5 x the size, or (half of them) a sixth of that, so some samples stay inside
        fl = torch.where(torch.rand(n, h, w, 2, generator=g) < 0.5, fl / 6.0, amp * torch.sign(fl))
    return fl


def _backwarp_case(shape, dtype, kind, scale):
    # (the seed key carries a salt: seeds are chosen so that no case's float64 reference has a weight mass within
    # 1e-4 of the mask threshold)
    g = _seed('backwarp', BACKWARP_SALT, shape, dtype, kind, scale)
    n, _, h, w = shape
    return _feat(shape, dtype, g), _flows(kind, n, h, w, scale, g)


BACKWARP_SALT = 0


@pytest.mark.parametrize('kind,scale', [('rand', 1.0), ('rand', 2.5), ('far', 1.0), ('far', 2.5), ('ident', 2.5),
                                        ('shift', 1.0)])
@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('shape', [(2, 64, 8, 8), (2, 32, 16, 16), (1, 96, 4, 4), (1, 64, 8, 16)])
def test_backwarp(shape, dtype, kind, scale):
    """Against the float64 bilinear gather at the float64 sample position.  The kernel computes the position in
    fp32: 8 roundings (flow * scale, (2x + 1) / W, - 1, flow / ((W - 1) / 2), the sum, + 1, * W, - 1) of
    intermediates of at most Mx = W + 2 + 2 |f| W / (W - 1) pixels, so the position is off by at most 8 2^-24 Mx,
    which moves the bilinear value by at most that times V = the sum of |v| over the in-frame neighbours (the
    interpolant is continuous; its slope in x is a weighted difference of neighbours).  The weights (1 - w, the
    product) and the four multiply-adds are 12 roundings of partial sums of at most S = sum w |v|.  So
    A = 2^-24 (8 (Mx + My) V + 12 S), and the stored value is within 0.5 u + A.  The mask (weight mass > 0.999) is
    the only discontinuity: pixels whose float64 mass is within 1e-4 of 0.999 are left out, at most 1 % (one pixel, in
    one case, here).  For the identity and the integer shift the result is the copied pixel or an exact zero."""
    L, lib, stream = _lib()
    n, C, h, w = shape
    x, fl = _backwarp_case(shape, dtype, kind, scale)
    ld = (C + 7) // 8 * 8
    X = _put(x, dtype, ld)
    FL = _put(fl, torch.float32, 8)
    out = _out((n, h, w, ld + 8), dtype)
    L.check(lib.dbsr_backwarp(n, h, w, C, _desc(L, X), _desc(L, FL), scale, _desc(L, out, 8), stream), 'dbsr_backwarp')
    torch.cuda.synchronize()
    _untouched(out, 8, 8 + C, 'backwarp')
    ref, mass, S, V, Mx, My = backwarp64(nchw(x), nchw(fl) * scale)
    amb = mask_ambiguous(mass)
    assert amb.double().mean().item() <= 0.01
    A = 2.0 ** -24 * (8.0 * (Mx + My) * V + 12.0 * S)
    got = nchw(out[..., 8:8 + C])
    if kind in ('ident', 'shift'):
        assert torch.equal(got, ref), 'exact warp: %d elements differ' % int((got != ref).sum())
    assert_single_rounding(got, ref, S, 12, dtype, 'backwarp %s %s %s x%g' % (shape, dtype, kind, scale),
                           mask=~amb.expand_as(ref), A=A)


# ----------------------------------------------------------------------------------------------------
# dbsr_conv_transpose_k4s2
# ----------------------------------------------------------------------------------------------------
def _convt_sg(ng):
    """Lanes per output pixel of the dispatch in dbsr_conv_transpose_k4s2."""
    return 1 if ng <= 1 else 4 if ng <= 8 else 8 if ng <= 24 else 32 if ng <= 96 else 64


@pytest.mark.parametrize('layout', ['c8', 'unaligned'])
@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('cin', [2, 8, 64, 192, 529, 661])
def test_conv_transpose_k4s2(cin, dtype, layout):
    """cin 2 and 8 (one 8-channel group), 64 (8 groups), 192 (24), 529 and 661 (67 and 83) take the 1-, 4-, 8- and
    32-lane variants of the dispatch (the 64-lane one needs more than 96 groups: test_conv_transpose_k4s2_wide).
    Input slice at c0 = 8 (16-byte loads) or c0 = 3 with an odd ld (the scalar
    path); the channels from cin to round_up(cin, 8) are read against zero-padded weights and hold 1.5.  Inputs of
    1x1, 2x2 and 8x8 pixels, n = 3, cout = 2, fp32 output at c0 = 3 of ld 8.  n_r: each lane's chain is 8 fmaf per
    8-channel group, ceil(groups / SG) groups, up to 4 taps; log2(SG) shuffle adds; the bias.  The reference is
    float64 conv_transpose2d on pack_convt's own weights, unpacked."""
    _run_convt(cin, dtype, layout)


@pytest.mark.parametrize('dtype', [torch.float16, torch.float32], ids=['fp16', 'fp32'])
def test_conv_transpose_k4s2_wide(dtype):
    """More than 96 channel groups (cin = 800): the 64-lane variant, which no PWC-Net level reaches (the widest
    upfeat input has 661 channels) but the dispatch has."""
    _run_convt(800, dtype, 'c8')


def test_conv_transpose_k4s2_flow():
    """The upflow call: the fp32 2-channel flow in an ld-8 buffer at c0 = 0."""
    _run_convt(2, torch.float32, 'flow')


def _run_convt(cin, dtype, layout):
    from dbsr_amd.engine import pack_convt
    L, lib, stream = _lib()
    g = _seed('convt', cin, dtype, layout)
    cin8 = (cin + 7) // 8 * 8
    c0, ld = {'c8': (8, cin8 + 16), 'unaligned': (3, cin8 + 8 + 5), 'flow': (0, 8)}[layout]
    wt = torch.randn(cin, 2, 4, 4, generator=g) * (1.0 / cin) ** 0.5
    bs = torch.randn(2, generator=g) * 0.1
    wp, bp = pack_convt(types.SimpleNamespace(weight=wt, bias=bs), DEV)
    assert tuple(wp.shape) == (4, 4, 2, cin8)
    w64 = wp.cpu()[..., :cin].permute(3, 2, 0, 1).double()
    assert not bool(wp[..., cin:].any())
    ng = cin8 // 8
    sg = _convt_sg(ng)
    n_r = 4 * 8 * -(-ng // sg) + (sg.bit_length() - 1) + 1
    for h in (1, 2, 8):
        x = torch.randn(3, h, h, cin, generator=g).to(dtype).float()
        X = _put(F.pad(x, (0, cin8 - cin), value=PAD_VALUE), dtype, ld, c0)
        out = _out((3, 2 * h, 2 * h, 8), torch.float32)
        L.check(lib.dbsr_conv_transpose_k4s2(3, h, h, cin, 2, _desc(L, X, c0), wp.data_ptr(), bp.data_ptr(),
                                             _desc(L, out, 3), stream), 'dbsr_conv_transpose_k4s2')
        torch.cuda.synchronize()
        _untouched(out, 3, 5, 'conv_transpose')
        xr = nchw(x)
        ref = F.conv_transpose2d(xr, w64, bs.double(), stride=2, padding=1)
        S = F.conv_transpose2d(xr.abs(), w64.abs(), bs.double().abs(), stride=2, padding=1)
        assert_single_rounding(nchw(out[..., 3:5]), ref, S, n_r, torch.float32,
                               'conv_transpose cin %d %s %s %dx%d (SG %d)' % (cin, dtype, layout, h, h, sg))


# ----------------------------------------------------------------------------------------------------
# dbsr_pwc_assemble
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('shape', [(2, 96, 4, 4), (1, 20, 5, 7), (3, 196, 1, 1)])
def test_pwc_assemble(shape, dtype):
    """Channels [c0 + 81, c0 + 81 + C + 4) = [first | upflow | upfeat]: the copy of `first` and the 16-bit roundings
    of the fp32 upflow and upfeat are bitwise; the 81 cost-volume channels in front and the pad behind stay."""
    L, lib, stream = _lib()
    n, C, h, w = shape
    g = _seed('assemble', shape, dtype)
    first = _feat(shape, dtype, g)
    flow, feat = torch.randn(n, h, w, 2, generator=g) * 3.0, torch.randn(n, h, w, 2, generator=g)
    c0 = 448
    out = _out((n, h, w, c0 + (81 + C + 4 + 31) // 32 * 32), dtype)
    FI, FL, FE = _put(first, dtype, (C + 7) // 8 * 8 + 8), _put(flow, torch.float32, 8), _put(feat, torch.float32, 2)
    L.check(lib.dbsr_pwc_assemble(n, h, w, C, _desc(L, FI), _desc(L, FL), _desc(L, FE), _desc(L, out, c0), stream),
            'dbsr_pwc_assemble')
    torch.cuda.synchronize()
    _untouched(out, c0 + 81, c0 + 81 + C + 4, 'assemble')
    o = out.cpu()
    assert_bitwise(o[..., c0 + 81:c0 + 81 + C], first.to(dtype), 'first')
    assert_bitwise(o[..., c0 + 81 + C:c0 + 83 + C], flow.to(dtype), 'upflow')
    assert_bitwise(o[..., c0 + 83 + C:c0 + 85 + C], feat.to(dtype), 'upfeat')


# ----------------------------------------------------------------------------------------------------
# dbsr_pack_burst
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('size', [(48, 48, 64, 64), (40, 56, 64, 64), (64, 64, 64, 64), (80, 72, 128, 128)])
def test_pack_burst(size, dtype):
    """raw: the four Bayer planes of every frame as an NHWC 4-channel slice, one rounding each (bitwise).  rgb:
    (R, (G1 + G2) / 2, B) resized to Hp x Wp against float64 F.interpolate(bilinear, align_corners=False).  The
    kernel's source index is scale * (dst + 0.5) - 0.5 in fp32: 3 roundings (the scale, the product, the difference)
    of at most W (or H) pixels, and the interpolant's slope is at most 1 for values in [0, 1]; the weights, the two
    lerps and the green mean are at most 12 roundings of partial sums of at most 1: A = 2^-24 (3 (H + W) + 12).  At
    64 -> 64 the source index is the destination index, so rgb is exactly the rounding of (R, (G1 + G2) / 2, B).
    The header describes rgb as a 3-channel slice: channels 3..7 of the packed frame are not written.  raw alone,
    rgb alone (the engine's PWC call passes a null raw) and both give the same bits."""
    L, lib, stream = _lib()
    H, W, Hp, Wp = size
    B, N = 2, 3
    g = _seed('pack', size, dtype)
    burst = torch.rand(B, N, 4, H, W, generator=g)
    bd = burst.to(DEV)
    runs = {}
    for mode in ('raw', 'rgb', 'both'):
        raw, rgb = _out((B * N, H, W, 8), dtype), _out((B * N, Hp, Wp, 8), dtype)
        L.check(lib.dbsr_pack_burst(B, N, H, W, bd.data_ptr(), _desc(L, raw, 4) if mode != 'rgb' else L.NULL_TENSOR,
                                    Hp, Wp, _desc(L, rgb) if mode != 'raw' else L.NULL_TENSOR, stream), 'pack_burst')
        torch.cuda.synchronize()
        runs[mode] = (raw.cpu(), rgb.cpu())
    assert_sentinel(runs['rgb'][0], 'raw of the rgb-only run')
    assert_sentinel(runs['raw'][1], 'rgb of the raw-only run')
    assert_bitwise(runs['both'][0], runs['raw'][0], 'raw: both against alone')
    assert_bitwise(runs['both'][1], runs['rgb'][1], 'rgb: both against alone')
    raw, rgb = runs['both']
    assert_sentinel(raw[..., :4], 'raw: channels in front')
    assert_bitwise(raw[..., 4:], burst.reshape(B * N, 4, H, W).permute(0, 2, 3, 1).to(dtype).contiguous(), 'raw')
    assert_sentinel(rgb[..., 3:], 'rgb pad channels 3..7')
    fr = burst.reshape(B * N, 4, H, W)
    green32 = (fr[:, 1] + fr[:, 2]) / 2.0
    if (H, W) == (Hp, Wp):
        assert_bitwise(rgb[..., :3], torch.stack([fr[:, 0], green32, fr[:, 3]], -1).to(dtype), 'identity resize')
    src = torch.stack([fr[:, 0].double(), (fr[:, 1].double() + fr[:, 2].double()) / 2.0, fr[:, 3].double()], 1)
    ref = F.interpolate(src, size=(Hp, Wp), mode='bilinear', align_corners=False)
    A = torch.full_like(ref, 2.0 ** -24 * (3.0 * (H + W) + 12.0))
    assert_single_rounding(nchw(rgb[..., :3]), ref, None, 12, dtype, 'pack_burst rgb %s %s' % (size, dtype), A=A)


# ----------------------------------------------------------------------------------------------------
# dbsr_flow_finalize
# ----------------------------------------------------------------------------------------------------
FF_SIZES = [(16, 16, 48, 48, 64, 64), (16, 16, 64, 64, 64, 64), (32, 32, 80, 72, 128, 128)]


def _ff_flow(kind, P, hf, wf, g):
    if kind == 'zero':
        return torch.zeros(P, hf, wf, 2)
    if kind == 'negative':
        return -(torch.rand(P, hf, wf, 2, generator=g) * 0.4 + 0.01)
    if kind == 'tiny':
        return torch.full((P, hf, wf, 2), -1e-9)
    return torch.randn(P, hf, wf, 2, generator=g) * 0.3


@pytest.mark.parametrize('modulo', [4.0, 0.0], ids=['mod4', 'nomod'])
@pytest.mark.parametrize('kind', ['rand', 'zero', 'negative', 'tiny'])
@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('BN', [(2, 3), (4, 2)], ids=['B2N3', 'P4N2'])
@pytest.mark.parametrize('size', FF_SIZES)
def test_flow_finalize(size, BN, dtype, kind, modulo):
    """offsets = 20 * bilinear(flow -> H x W) * (W / Wp, H / Hp), fp32, against float64 within A: the source index
    takes 3 roundings of at most wf (hf) pixels and the interpolant's slope is at most 2 M (M = max |flow|); the
    weights, the lerps, the factor 20, the rounded W / Wp and the product are at most 15 roundings of at most M:
    A = 20 max(W / Wp, H / Hp) 2^-24 M (6 (hf + wf) + 15).  offs_mod is teacher-forced: torch.remainder in fp32 of the
    kernel's own offsets (fmodf is exact, the sign shift is the same single fp32 add), rounded to the dtype, bitwise;
    frame 0 of every burst is exactly +0; modulo 0 stores the offsets themselves.  The -1e-9 flow has a remainder
    that rounds up to the modulus itself.  (B, N) = (2, 3) and the PWC module's own call, B = P, N = 2."""
    L, lib, stream = _lib()
    hf, wf, H, W, Hp, Wp = size
    B, N = BN
    P = B * (N - 1)
    g = _seed('ff', size, BN, dtype, kind)
    flow = _ff_flow(kind, P, hf, wf, g)
    FL = _put(flow, torch.float32, 2)
    offs = _out((P, 2, H, W), torch.float32)
    om = _out((B * N, H, W, 6), dtype)
    L.check(lib.dbsr_flow_finalize(B, N, hf, wf, _desc(L, FL), H, W, Hp, Wp, offs.data_ptr(), modulo, _desc(L, om, 3),
                                   stream), 'dbsr_flow_finalize')
    torch.cuda.synchronize()
    _untouched(om, 3, 5, 'offs_mod')
    o = offs.cpu()
    sc = torch.tensor([W / Wp, H / Hp], dtype=torch.float64).view(1, 2, 1, 1)
    ref = 20.0 * F.interpolate(nchw(flow), size=(H, W), mode='bilinear', align_corners=False) * sc
    M = flow.abs().max().item()
    A = torch.full_like(ref, 20.0 * max(W / Wp, H / Hp) * 2.0 ** -24 * M * (6.0 * (hf + wf) + 15.0))
    assert_single_rounding(o, ref, None, 15, torch.float32, 'flow_finalize %s %s' % (size, kind), A=A)
    exp = torch.remainder(o, modulo) if modulo != 0.0 else o
    exp = exp.permute(0, 2, 3, 1).reshape(B, N - 1, H, W, 2)
    exp = torch.cat([torch.zeros(B, 1, H, W, 2), exp], 1).reshape(B * N, H, W, 2).to(dtype)
    assert_bitwise(om.cpu()[..., 3:5], exp, 'offs_mod')
    if kind == 'tiny' and modulo != 0.0:
        assert bool((exp.reshape(B, N, H, W, 2)[:, 1:].float() == modulo).all())


def test_flow_finalize_without_offs_mod():
    """The PWC module's call passes no offs_mod: the offsets are the same bits."""
    L, lib, stream = _lib()
    hf, wf, H, W, Hp, Wp = FF_SIZES[0]
    flow = _ff_flow('rand', 4, hf, wf, _seed('ff-null'))
    FL = _put(flow, torch.float32, 2)
    a, b = _out((4, 2, H, W), torch.float32), _out((4, 2, H, W), torch.float32)
    om = _out((8, H, W, 2), torch.float16)
    L.check(lib.dbsr_flow_finalize(4, 2, hf, wf, _desc(L, FL), H, W, Hp, Wp, a.data_ptr(), 0.0, L.NULL_TENSOR, stream),
            'dbsr_flow_finalize')
    L.check(lib.dbsr_flow_finalize(4, 2, hf, wf, _desc(L, FL), H, W, Hp, Wp, b.data_ptr(), 4.0, _desc(L, om), stream),
            'dbsr_flow_finalize')
    torch.cuda.synchronize()
    assert_bitwise(a.cpu(), b.cpu(), 'offsets with and without offs_mod')


# ----------------------------------------------------------------------------------------------------
# dbsr_merge_prep (forward), dbsr_burst_mean
# ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('c', [16, 64])
@pytest.mark.parametrize('N', [1, 3, 14])
def test_merge_prep(N, c, dtype):
    """out[f] = [proj[b, 0] | proj[b, n] - proj[b, 0]] at channels [c0, c0 + 2c): the base is bitwise frame 0 of the
    burst, the difference one rounding of the fp32 difference (bitwise).  hw = 35 (ragged), B = 2, c0 = 8."""
    L, lib, stream = _lib()
    B, hw = 2, 35
    g = _seed('merge_prep', N, c, dtype)
    proj = torch.randn(B * N, 5, 7, c, generator=g).to(dtype)
    out = _out((B * N, 5, 7, 8 + 2 * c + 8), dtype)
    PR = _put(proj, dtype, c + 8)
    L.check(lib.dbsr_merge_prep(B, N, hw, c, _desc(L, PR), _desc(L, out, 8), stream), 'dbsr_merge_prep')
    torch.cuda.synchronize()
    _untouched(out, 8, 8 + 2 * c, 'merge_prep')
    base = proj.reshape(B, N, 5, 7, c)[:, :1].expand(B, N, 5, 7, c).reshape(B * N, 5, 7, c).contiguous()
    o = out.cpu()
    assert_bitwise(o[..., 8:8 + c], base, 'base')
    assert_bitwise(o[..., 8 + c:8 + 2 * c], (proj.float() - base.float()).to(dtype), 'diff')


@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('c', [16, 64])
@pytest.mark.parametrize('N', [1, 3, 14])
def test_burst_mean(N, c, dtype):
    """out[b] = (sum_n in[b * N + n]) / N: an fp32 sum in frame order from 0, one IEEE division, one rounding to the
    dtype -- each step is what torch's fp32 ops do, so the result is bitwise.  hw = 35, B = 2, output at c0 = 4."""
    L, lib, stream = _lib()
    B, hw = 2, 35
    g = _seed('burst_mean', N, c, dtype)
    x = torch.randn(B * N, 5, 7, c, generator=g).to(dtype)
    out = _out((B, 5, 7, 4 + c + 4), dtype)
    X = _put(x, dtype, c + 4)
    L.check(lib.dbsr_burst_mean(B, N, hw, c, _desc(L, X), _desc(L, out, 4), stream), 'dbsr_burst_mean')
    torch.cuda.synchronize()
    _untouched(out, 4, 4 + c, 'burst_mean')
    acc = torch.zeros(B, 5, 7, c)
    xs = x.float().reshape(B, N, 5, 7, c)
    for n in range(N):
        acc = acc + xs[:, n]
    assert_bitwise(out.cpu()[..., 4:4 + c], (acc / float(N)).to(dtype), 'burst mean')
