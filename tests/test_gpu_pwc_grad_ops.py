"""Op-level tests of the PWC-Net training kernels (csrc/pwc_grad.hip) and of the operators built on them, against
float64 on the CPU (F.conv2d / F.conv_transpose2d / F.interpolate under autograd) on the same rounded operands, with
the single-rounding bound of tests/pwc_ref.py: |out - ref| <= A for fp32 outputs, 0.5 u + A for 16-bit stores,
A = n_r 2^-24 S, S the same op on absolute values, n_r the number of terms of that output's sum (any summation
order of n terms stays within (n - 1) 2^-24 S; the 16-bit products are exact in fp32).  No torch convolution runs
on the device."""
import pytest
import torch
import torch.nn.functional as F

from tests.pwc_ref import SENTINEL, assert_bitwise, assert_single_rounding, spacing

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DT = [torch.float16, torch.bfloat16, torch.float32]
IDS = ['fp16', 'bf16', 'fp32']
PAD_VALUE = 1.5
F64 = torch.float64


def _seed(*key):
    s = 0
    for ch in '|'.join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def _lib():
    from dbsr_amd import _lib as L
    return L, L.lib(), L.stream_ptr(DEV)


def _epp(dtype):
    return 4 if dtype == torch.float32 else 8


def _ld(c, dtype, extra=1):
    """A pixel pitch that holds c channels rounded up to 16 bytes plus `extra` further 16-byte pieces."""
    e = _epp(dtype)
    return (c + e - 1) // e * e + extra * e


def _put(x_nchw, dtype, ld, c0=0, fill=PAD_VALUE):
    """float64 [n, c, h, w] (values exact in dtype) as channels [c0, c0 + c) of a device buffer [n, h, w, ld]."""
    n, c, h, w = x_nchw.shape
    buf = torch.full((n, h, w, ld), fill, dtype=dtype, device=DEV)
    buf[..., c0:c0 + c] = x_nchw.permute(0, 2, 3, 1).to(dtype).to(DEV)
    return buf


def _desc(L, buf, c0=0):
    return L.tensor_desc(buf, buf.shape[-1], c0)


def _rand(shape, dtype, g, scale=1.0):
    """Seeded values rounded to dtype, float64 on the CPU."""
    return (torch.randn(*shape, generator=g) * scale).to(dtype).double()


def _conv_out(i, k, s, d, pad):
    return (i + 2 * pad - d * (k - 1) - 1) // s + 1


def _wgrad64(x, dy, cout, k, s, d, pad):
    w = torch.zeros(cout, x.shape[1], k, k, dtype=F64, requires_grad=True)
    (F.conv2d(x, w, None, s, pad, d) * dy).sum().backward()
    return w.grad


def _dgrad64(dy, w, in_h, in_w, s, d, pad):
    x = torch.zeros(dy.shape[0], w.shape[1], in_h, in_w, dtype=F64, requires_grad=True)
    (F.conv2d(x, w, None, s, pad, d) * dy).sum().backward()
    return x.grad


def _run_wgrad_sd(x, dy, k, s, d, pad, dtype, want_db=True, dw0=None, c0x=0, c0y=0):
    """dbsr_conv_wgrad_sd on float64 NCHW x / dy (exact in dtype); returns (dw, db) on the CPU."""
    L, lib, stream = _lib()
    n, cin, in_h, in_w = x.shape
    _, cout, oh, ow = dy.shape
    e = _epp(dtype)
    X, DY = _put(x, dtype, _ld(cin, dtype) + c0x, c0x), _put(dy, dtype, _ld(cout, dtype) + c0y, c0y)
    dw = torch.full((cout, cin, k, k), SENTINEL, dtype=torch.float32, device=DEV) if dw0 is None else dw0.float().to(DEV)
    db = torch.full((cout,), SENTINEL, dtype=torch.float32, device=DEV)
    need = lib.dbsr_conv_wgrad_sd_workspace_bytes(n, oh, ow, cin, cout, k)
    assert need > 0
    ws = torch.full((need // 4 + 4,), float('nan'), dtype=torch.float32, device=DEV)    # nothing relies on zeros
    L.check(lib.dbsr_conv_wgrad_sd(n, in_h, in_w, _desc(L, X, c0x), cin, oh, ow, _desc(L, DY, c0y), cout, k, s, d, pad,
                                   dw.data_ptr(), db.data_ptr() if want_db else None, 0 if dw0 is None else 1,
                                   ws.data_ptr(), need, stream), 'dbsr_conv_wgrad_sd')
    torch.cuda.synchronize()
    assert e in (4, 8)
    return dw.cpu(), db.cpu()


# (n, cin, cout, h, w, k, s, d, pad)
WGRAD_CASES = [(2, 3, 16, 6, 10, 3, 2, 1, 1), (1, 16, 32, 5, 7, 3, 2, 1, 1), (2, 128, 196, 2, 2, 3, 2, 1, 1),
               (1, 40, 24, 16, 16, 3, 1, 16, 16), (1, 32, 32, 9, 12, 3, 1, 2, 2), (1, 32, 32, 9, 12, 3, 1, 4, 4),
               (1, 32, 32, 9, 12, 3, 1, 8, 8), (2, 72, 2, 4, 4, 3, 1, 1, 1), (1, 8, 8, 1, 1, 1, 1, 1, 0)]


@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('case', WGRAD_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_wgrad_sd(case, dtype):
    """dw and db against float64 autograd of F.conv2d; n_r = n oh ow terms per weight.  Input pad channels hold 1.5,
    the workspace NaN and the outputs a sentinel: every dw / db element is written and nothing else is summed.  A
    dilation-16 conv on a 16 x 16 image reads only padding off centre: those eight taps are exactly 0.  Two runs are
    bitwise equal; accumulate adds onto a nonzero dw (one more rounding)."""
    n, cin, cout, h, w, k, s, d, pad = case
    oh, ow = _conv_out(h, k, s, d, pad), _conv_out(w, k, s, d, pad)
    g = _seed('wgrad_sd', case, dtype)
    x, dy = _rand((n, cin, h, w), dtype, g), _rand((n, cout, oh, ow), dtype, g)
    dw, db = _run_wgrad_sd(x, dy, k, s, d, pad, dtype, c0x=_epp(dtype))
    ref, S = _wgrad64(x, dy, cout, k, s, d, pad), _wgrad64(x.abs(), dy.abs(), cout, k, s, d, pad)
    n_r = n * oh * ow
    assert_single_rounding(dw, ref, S, n_r, torch.float32, 'wgrad_sd dw %s' % (case,))
    assert_single_rounding(db, dy.sum((0, 2, 3)), dy.abs().sum((0, 2, 3)), n_r, torch.float32, 'wgrad_sd db %s' % (case,))
    if d == 16:
        off = torch.ones(3, 3, dtype=torch.bool)
        off[1, 1] = False
        assert bool((dw[:, :, off] == 0).all()), 'off-centre taps of the dilation-16 conv'
        assert bool((S[:, :, off] == 0).all())
    dw2, db2 = _run_wgrad_sd(x, dy, k, s, d, pad, dtype, c0x=_epp(dtype))
    assert_bitwise(dw2, dw, 'wgrad_sd dw, second run')
    assert_bitwise(db2, db, 'wgrad_sd db, second run')
    dw0 = _rand((cout, cin, k, k), torch.float32, g)
    dwa, _ = _run_wgrad_sd(x, dy, k, s, d, pad, dtype, want_db=False, dw0=dw0)
    assert_single_rounding(dwa, dw0 + ref, dw0.abs() + S, n_r + 1, torch.float32, 'wgrad_sd accumulate %s' % (case,))


@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('shape', [((2, 40, 3, 5), 2), ((1, 2, 1, 1), 2)], ids=['40x3x5', '2x1x1'])
def test_conv_transpose_wgrad_by_role_swap(shape, dtype):
    """ConvTranspose2d(k4, s2, p1)'s weight gradient is dbsr_conv_wgrad_sd with the roles swapped: "input" = dy
    [n][2h][2w] (cout channels), "output gradient" = x [n][h][w] (cin channels); the result is torch's
    [cin][cout][4][4].  n_r = n h w."""
    (n, cin, h, w), cout = shape
    g = _seed('convt_wgrad', shape, dtype)
    x, dy = _rand((n, cin, h, w), dtype, g), _rand((n, cout, 2 * h, 2 * w), dtype, g)
    dw, _ = _run_wgrad_sd(dy, x, 4, 2, 1, 1, dtype, want_db=False)

    def ref64(a, b):
        wt = torch.zeros(cin, cout, 4, 4, dtype=F64, requires_grad=True)
        (F.conv_transpose2d(a, wt, None, 2, 1) * b).sum().backward()
        return wt.grad
    assert dw.shape == (cin, cout, 4, 4)
    assert_single_rounding(dw, ref64(x, dy), ref64(x.abs(), dy.abs()), n * h * w, torch.float32,
                           'convT wgrad %s' % (shape,))


def _run_dgrad_sd(dy, w, in_h, in_w, s, d, pad, dtype):
    """dbsr_conv_dgrad_sd on float64 NCHW dy and torch-layout w (exact in dtype); returns the whole dx buffer
    [n, in_h, in_w, ld] on the CPU, its slice at c0 = one 16-byte piece."""
    L, lib, stream = _lib()
    n, cout, oh, ow = dy.shape
    cin, k = w.shape[1], w.shape[2]
    e = _epp(dtype)
    DY = _put(dy, dtype, _ld(cout, dtype), 0, fill=0.0)         # (the pad up to 16 bytes meets zero weights: finite)
    DY[..., (cout + e - 1) // e * e:] = PAD_VALUE
    W32 = w.float().contiguous().to(DEV)
    wp = torch.full((lib.dbsr_dgrad_sd_packed_elems(cout, cin, k),), SENTINEL, dtype=dtype, device=DEV)
    L.check(lib.dbsr_dgrad_sd_pack(W32.data_ptr(), cout, cin, k, L.dtype_code(dtype), wp.data_ptr(), stream),
            'dbsr_dgrad_sd_pack')
    DX = torch.full((n, in_h, in_w, _ld(cin, dtype) + e), SENTINEL, dtype=dtype, device=DEV)
    L.check(lib.dbsr_conv_dgrad_sd(n, in_h, in_w, _desc(L, DX, e), cin, oh, ow, _desc(L, DY), cout, k, s, d, pad,
                                   wp.data_ptr(), stream), 'dbsr_conv_dgrad_sd')
    torch.cuda.synchronize()
    return DX.cpu()


def _check_dgrad(DX, dy, w, in_h, in_w, s, d, pad, dtype, what):
    cin = w.shape[1]
    e = _epp(dtype)
    own = (cin + e - 1) // e * e
    ref = _dgrad64(dy, w, in_h, in_w, s, d, pad)
    S = _dgrad64(dy.abs(), w.abs(), in_h, in_w, s, d, pad)
    cnt = _dgrad64(torch.ones_like(dy), torch.ones_like(w), in_h, in_w, s, d, pad)     # terms per output
    out = DX[..., e:e + cin].permute(0, 3, 1, 2)
    assert_single_rounding(out, ref, S, int(cnt.max()), dtype, what, A=cnt * 2.0 ** -24 * S)
    # every owned element is written (the pad up to 16 bytes as zeros), nothing else is
    assert not bool((DX[..., e:e + cin] == SENTINEL).all(-1).any()), what + ': an unwritten pixel'
    assert bool((DX[..., e + cin:e + own] == 0).all()), what + ': pad channels are zeros'
    assert bool((DX[..., :e] == SENTINEL).all()) and bool((DX[..., e + own:] == SENTINEL).all()), what + ': stray store'


# (n, cin, cout, in_h, in_w) at k3 s2 p1
DGRAD_CASES = [(2, 3, 16, 6, 10), (1, 16, 32, 5, 7), (2, 128, 196, 2, 2), (1, 96, 128, 4, 4)]


@pytest.mark.parametrize('dtype', DT, ids=IDS)
@pytest.mark.parametrize('case', DGRAD_CASES, ids=lambda c: 'x'.join(str(v) for v in c))
def test_dgrad_sd_stride2(case, dtype):
    """The stride-2 input gradient against float64 autograd; n_r per element = its live taps x cout (1, 2, 2 or 4
    taps by parity class, fewer at the border).  dx is prefilled with a sentinel: none survives in the owned
    channels, none is overwritten outside."""
    n, cin, cout, in_h, in_w = case
    oh, ow = _conv_out(in_h, 3, 2, 1, 1), _conv_out(in_w, 3, 2, 1, 1)
    g = _seed('dgrad_sd', case, dtype)
    dy, w = _rand((n, cout, oh, ow), dtype, g), _rand((cout, cin, 3, 3), dtype, g, 0.2)
    DX = _run_dgrad_sd(dy, w, in_h, in_w, 2, 1, 1, dtype)
    _check_dgrad(DX, dy, w, in_h, in_w, 2, 1, 1, dtype, 'dgrad_sd %s' % (case,))


@pytest.mark.parametrize('dtype', DT, ids=IDS)
def test_dgrad_sd_stride1_matches_conv2d_route(dtype):
    """s = 1, d = 2: the gather kernel and the op layer's route (dbsr_conv2d with dbsr_dgrad_weights) both stay within
    the same bound of the float64 gradient."""
    from dbsr_amd import torch_ops
    ops = torch_ops.load()
    n, cin, cout, h, w_, d = 1, 24, 40, 9, 12, 2
    g = _seed('dgrad_sd s1', dtype)
    dy, w = _rand((n, cout, h, w_), dtype, g), _rand((cout, cin, 3, 3), dtype, g, 0.2)
    DX = _run_dgrad_sd(dy, w, h, w_, 1, d, d, dtype)
    _check_dgrad(DX, dy, w, h, w_, 1, d, d, dtype, 'dgrad_sd s1 d2')
    x = torch.zeros(n, cin, h, w_, dtype=dtype, device=DEV)
    dx, dw, db = ops.conv2d_backward(dy.to(dtype).to(DEV), x, w.float().to(DEV), dy.to(dtype).to(DEV), 1, d, d, 0, True,
                                     False, False)
    assert dw.numel() == 0 and db.numel() == 0
    ref, S = _dgrad64(dy, w, h, w_, 1, d, d), _dgrad64(dy.abs(), w.abs(), h, w_, 1, d, d)
    cnt = _dgrad64(torch.ones_like(dy), torch.ones_like(w), h, w_, 1, d, d)
    assert_single_rounding(dx.cpu(), ref, S, int(cnt.max()), dtype, 'conv2d route s1 d2', A=cnt * 2.0 ** -24 * S)


def _round_once(q, dtype):
    """float64 q rounded ONCE to dtype (torch's float64 -> 16-bit cast goes through float32): the nearest of the
    representable values around the double-rounded candidate.  No ties occur for q = dy * float32(0.1): the odd part
    of the product has at least 24 bits."""
    c = q.float().to(dtype).double()
    u = spacing(c, dtype)
    best, bd = c, (q - c).abs()
    for cand in (c + u, c - u, c + u / 2, c - u / 2):
        ok = cand.to(dtype).double() == cand
        dist = (q - cand).abs()
        take = ok & (dist < bd)
        best, bd = torch.where(take, cand, best), torch.where(take, dist, bd)
    return best


@pytest.mark.parametrize('act', ['relu', 'lrelu'])
@pytest.mark.parametrize('dtype', DT, ids=IDS)
def test_act_backward_exact(dtype, act):
    """dpre = dy where y > 0, else 0 (ReLU) or float32(0.1) * dy rounded once (LeakyReLU), exactly, including
    y = 0, y = -0.0 and subnormal dy; pad channels of the slice are zeros, the rest of the buffer is untouched."""
    L, lib, stream = _lib()
    n, h, w, c = 2, 5, 7, 20
    g = _seed('act_bwd', dtype, act)
    dy = _rand((n, c, h, w), dtype, g)
    y = _rand((n, c, h, w), dtype, g)
    tiny = float(spacing(torch.zeros(()), dtype))                     # the smallest subnormal
    dy[0, :, 0, 0] = tiny * torch.arange(1, c + 1, dtype=F64)         # subnormal dy, both signs of y below
    dy[0, :, 0, 1] = -tiny * torch.arange(1, 2 * c, 2, dtype=F64)
    dy[0, :, 0, 2] = 2.0 ** -20 * torch.arange(1, c + 1, dtype=F64)
    y[0, ::2, 0, :3] = -1.0
    y[0, 1::2, 0, :3] = 1.0
    y[1, :, 1, 0] = 0.0
    y[1, :, 1, 1] = -0.0
    ld, e = 48, 8                                                      # the slice [8, 28) of 48, its pad up to 32
    DY, Y = _put(dy, dtype, ld, e), _put(y, dtype, ld, e)
    Y[1, 1, 1, e:e + c] = torch.tensor(-0.0, dtype=dtype)
    OUT = torch.full((n, h, w, ld), SENTINEL, dtype=dtype, device=DEV)
    code = L.ACT_RELU if act == 'relu' else L.ACT_LRELU
    L.check(lib.dbsr_act_backward(n, h * w, c, code, _desc(L, DY, e), _desc(L, Y, e), _desc(L, OUT, e), stream),
            'dbsr_act_backward')
    torch.cuda.synchronize()
    out = OUT.cpu()
    slope = torch.tensor(0.1, dtype=torch.float32).double()
    neg = torch.zeros_like(dy) if act == 'relu' else _round_once(dy * slope, dtype)
    exp = torch.where(y > 0, dy, neg).permute(0, 2, 3, 1)
    got = out[..., e:e + c].double()
    bad = got != exp
    assert not bool(bad.any()), '%d of %d differ, first at %s' % (int(bad.sum()), bad.numel(), torch.nonzero(bad)[0])
    c8 = (c + 7) // 8 * 8
    assert bool((out[..., e + c:e + c8] == 0).all()), 'pad channels are zeros'
    assert bool((out[..., :e] == SENTINEL).all()) and bool((out[..., e + c8:] == SENTINEL).all()), 'stray store'


def _interp_counts(coarse, fine):
    """Fine indices with a nonzero weight on each coarse index (1-D, align_corners=False)."""
    m = F.interpolate(torch.eye(coarse, dtype=F64).view(coarse, 1, coarse, 1), size=(fine, 1), mode='bilinear',
                      align_corners=False)
    return (m.view(coarse, fine) > 0).sum(1)


@pytest.mark.parametrize('size', [(16, 16, 24, 32), (16, 16, 64, 64), (32, 32, 80, 80), (16, 16, 8, 12)],
                         ids=lambda s: 'x'.join(str(v) for v in s))
def test_flow_finalize_backward(size):
    """dflow against float64 autograd of 20 * F.interpolate(flow, (H, W)) * (W / Wp, H / Hp); n_r = the fine pixels
    that touch the coarse pixel + 3.  Up- and down-sampling (an 8 x 12 burst's 16 x 16 flow is downsampled: a
    coarse pixel is then touched by one fine pixel per axis, or none).  Channels beside the two written ones keep the
    sentinel."""
    L, lib, stream = _lib()
    hf, wf, H, W = size
    P, Hp, Wp = 2, 4 * hf, 4 * wf
    g = _seed('ff_bwd', size)
    doff = _rand((P, 2, H, W), torch.float32, g)
    G = doff.float().contiguous().to(DEV)
    OUT = torch.full((P, hf, wf, 4), SENTINEL, dtype=torch.float32, device=DEV)
    L.check(lib.dbsr_flow_finalize_backward(P, hf, wf, H, W, Hp, Wp, G.data_ptr(), _desc(L, OUT, 1), stream),
            'dbsr_flow_finalize_backward')
    torch.cuda.synchronize()
    out = OUT.cpu()
    sc = torch.tensor([W / Wp, H / Hp], dtype=F64).view(1, 2, 1, 1)

    def ref64(gr):
        fl = torch.zeros(P, 2, hf, wf, dtype=F64, requires_grad=True)
        (20.0 * F.interpolate(fl, size=(H, W), mode='bilinear', align_corners=False) * sc * gr).sum().backward()
        return fl.grad
    ref, S = ref64(doff), ref64(doff.abs())
    cnt = (_interp_counts(hf, H).view(hf, 1) * _interp_counts(wf, W).view(1, wf)).double().view(1, 1, hf, wf)
    assert_single_rounding(out[..., 1:3].permute(0, 3, 1, 2), ref, S, int(cnt.max()) + 3, torch.float32,
                           'flow_finalize_backward %s' % (size,), A=(cnt + 3.0) * 2.0 ** -24 * S)
    assert bool((out[..., 0] == SENTINEL).all()) and bool((out[..., 3] == SENTINEL).all())


# ----------------------------------------------------------------------------------------------------
# autograd of the operators (fp32, one small shape each).  The reference takes the LeakyReLU's branch from the
# op's own forward output (the same numbers: a pre-activation within rounding of 0 may land on either side).
# n_r: the terms of each gradient's sum plus the activation's product and the store.
# ----------------------------------------------------------------------------------------------------
def _conv_autograd_case(n, cin, cout, h, w, k, s, d, pad, act):
    from dbsr_amd import _lib as L, torch_ops
    ops = torch_ops.load()
    g = _seed('conv autograd', n, cin, cout, h, w, k, s, d, pad, act)
    x, wt, b = _rand((n, cin, h, w), torch.float32, g), _rand((cout, cin, k, k), torch.float32, g, 0.2), \
        _rand((cout,), torch.float32, g)
    oh, ow = _conv_out(h, k, s, d, pad), _conv_out(w, k, s, d, pad)
    G = _rand((n, cout, oh, ow), torch.float32, g)
    xd, wd, bd = [t.float().to(DEV).requires_grad_(True) for t in (x, wt, b)]
    code = {'none': L.ACT_NONE, 'lrelu': L.ACT_LRELU}[act]
    y = ops.conv2d_fused(xd, wd, bd, s, pad, d, code, None, 0)
    assert y.grad_fn is not None and y.shape == (n, cout, oh, ow)
    (y * G.float().to(DEV)).sum().backward()
    slope = torch.tensor(0.1, dtype=torch.float32).double()
    dpre = G if act == 'none' else G * torch.where(y.detach().cpu().double() > 0, torch.ones((), dtype=F64), slope)
    terms = n * oh * ow
    assert_single_rounding(wd.grad.cpu(), _wgrad64(x, dpre, cout, k, s, d, pad),
                           _wgrad64(x.abs(), dpre.abs(), cout, k, s, d, pad), terms + 2, torch.float32, 'dw')
    assert_single_rounding(bd.grad.cpu(), dpre.sum((0, 2, 3)), dpre.abs().sum((0, 2, 3)), terms + 2, torch.float32, 'db')
    cnt = _dgrad64(torch.ones_like(dpre), torch.ones_like(wt), h, w, s, d, pad)
    assert_single_rounding(xd.grad.cpu(), _dgrad64(dpre, wt, h, w, s, d, pad), _dgrad64(dpre.abs(), wt.abs(), h, w, s, d, pad),
                           int(cnt.max()) + 2, torch.float32, 'dx', A=(cnt + 2.0) * 2.0 ** -24 *
                           _dgrad64(dpre.abs(), wt.abs(), h, w, s, d, pad))


@pytest.mark.parametrize('case', [(2, 16, 24, 7, 10, 3, 2, 1, 1, 'lrelu'), (1, 24, 16, 9, 12, 3, 1, 4, 4, 'lrelu'),
                                  (2, 40, 2, 6, 5, 3, 1, 1, 1, 'none')], ids=['s2-lrelu', 'd4-lrelu', 'none-cout2'])
def test_conv2d_fused_autograd(case):
    _conv_autograd_case(*case)


def test_conv_transpose2d_k4s2_autograd():
    from dbsr_amd import torch_ops
    ops = torch_ops.load()
    n, cin, cout, h, w = 2, 20, 2, 3, 5
    g = _seed('convt autograd')
    x, wt, b = _rand((n, cin, h, w), torch.float32, g), _rand((cin, cout, 4, 4), torch.float32, g, 0.2), \
        _rand((cout,), torch.float32, g)
    G = _rand((n, cout, 2 * h, 2 * w), torch.float32, g)
    xd, wd, bd = [t.float().to(DEV).requires_grad_(True) for t in (x, wt, b)]
    y = ops.conv_transpose2d_k4s2(xd, wd, bd)
    (y * G.float().to(DEV)).sum().backward()

    def ref64(xa, wa, ba, Ga):
        xa, wa, ba = [t.clone().requires_grad_(True) for t in (xa, wa, ba)]
        out = F.conv_transpose2d(xa, wa, ba, 2, 1)
        (out * Ga).sum().backward()
        return out.detach(), xa.grad, wa.grad, ba.grad
    yr, dx, dw, db = ref64(x, wt, b, G)
    ys, sx, sw, sb = ref64(x.abs(), wt.abs(), b.abs(), G.abs())
    assert_single_rounding(y.detach().cpu(), yr, ys, 4 * cin + 2, torch.float32, 'convT forward')
    assert_single_rounding(xd.grad.cpu(), dx, sx, 16 * cout + 1, torch.float32, 'convT dx')
    assert_single_rounding(wd.grad.cpu(), dw, sw, n * h * w + 1, torch.float32, 'convT dw')
    assert_single_rounding(bd.grad.cpu(), db, sb, 4 * n * h * w + 1, torch.float32, 'convT db')


def test_flow_finalize_autograd():
    from dbsr_amd import torch_ops
    ops = torch_ops.load()
    P, hf, wf, H, W = 2, 16, 16, 24, 32
    g = _seed('ff autograd')
    fl, G = _rand((P, 2, hf, wf), torch.float32, g), _rand((P, 2, H, W), torch.float32, g)
    fd = fl.float().to(DEV).requires_grad_(True)
    off = ops.flow_finalize(fd, H, W)
    assert off.shape == (P, 2, H, W) and off.grad_fn is not None
    (off * G.float().to(DEV)).sum().backward()
    sc = torch.tensor([W / 64.0, H / 64.0], dtype=F64).view(1, 2, 1, 1)

    def ref64(gr):
        f = torch.zeros(P, 2, hf, wf, dtype=F64, requires_grad=True)
        (20.0 * F.interpolate(f, size=(H, W), mode='bilinear', align_corners=False) * sc * gr).sum().backward()
        return f.grad
    cnt = (_interp_counts(hf, H).view(hf, 1) * _interp_counts(wf, W).view(1, wf)).double().view(1, 1, hf, wf)
    S = ref64(G.abs())
    assert_single_rounding(fd.grad.cpu(), ref64(G), S, int(cnt.max()) + 3, torch.float32, 'flow_finalize autograd',
                           A=(cnt + 3.0) * 2.0 ** -24 * S)


def test_needs_input_grad_is_respected(monkeypatch):
    """A frozen input's gradient is not computed: the backward op sees need_x / need_w / need_b as autograd has
    them, and is not called at all when nothing upstream needs a gradient."""
    from dbsr_amd import _lib as L, torch_ops
    ops = torch_ops.load()
    calls = []
    real = torch.ops.dbsr.conv2d_backward

    class Spy:
        def __call__(self, *a):
            calls.append(a[-3:])
            return real(*a)
    monkeypatch.setattr(torch.ops.dbsr, 'conv2d_backward', Spy())
    x = torch.randn(1, 8, 6, 6, device=DEV)
    w = torch.randn(8, 8, 3, 3, device=DEV, requires_grad=True)
    b = torch.randn(8, device=DEV)
    y = ops.conv2d_fused(x, w, b, 2, 1, 1, L.ACT_LRELU, None, 0)
    y.sum().backward()
    assert calls == [(False, True, False)], calls
    assert w.grad is not None and x.grad is None and b.grad is None
    calls.clear()
    y = ops.conv2d_fused(x, w.detach(), b, 2, 1, 1, L.ACT_LRELU, None, 0)
    assert y.grad_fn is None and calls == []


def test_residual_refused_while_recording():
    from dbsr_amd import _lib as L, torch_ops
    ops = torch_ops.load()
    x = torch.randn(1, 8, 6, 6, device=DEV, requires_grad=True)
    w = torch.randn(8, 8, 3, 3, device=DEV)
    with pytest.raises(RuntimeError, match='residual=None and post_act=0'):
        ops.conv2d_fused(x, w, None, 1, 1, 1, L.ACT_RELU, x.detach(), 0)
    with pytest.raises(RuntimeError, match='residual=None and post_act=0'):
        ops.conv2d_fused(x, w, None, 1, 1, 1, L.ACT_NONE, None, L.ACT_RELU)
    # without a grad-requiring input the epilogues still run
    assert ops.conv2d_fused(x.detach(), w, None, 1, 1, 1, L.ACT_RELU, x.detach(), 0).shape == x.shape
