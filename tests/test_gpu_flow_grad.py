"""Flow gradients on the HIP kernels (csrc/flow_grad.hip): dbsr_warp_flow_backward, dbsr_backwarp_backward, the
operators' autograd formulas on top of them, and dL/d(offsets) from DBSRTrainer (flow_grad=True, external flows).

Reference: float64 torch autograd on the CPU through oracle.warp / oracle.backwarp, on the rounded operands the
kernel reads (16-bit inputs converted back to float64).

Sample positions.  Warp flows lie on a 1/8 grid plus 1/16 (backwarp flows are chosen so that the sample POSITIONS
do: the W/(W-1) factor of its grid would otherwise move them off it), so every position is at least 1/16 from an
integer in both axes: an fp32-versus-float64 difference in the position cannot flip the cell or backwarp's mask (the
mass is 1 inside and at most 15/16 where a corner is out).  No pixel is excluded.

Bounds (fp32 outputs; the style of tests/pwc_ref.py): |out - ref| <= n_r 2^-24 S + dpos S2.
  S    float64 sum of the absolute values of the terms of that output.
  n_r  fp32 roundings in the chain.  A term d * (wa * (va - vb) + wb * (vc - vd)) passes two subtractions (one each
       on its way), a product, an fma and the accumulating fma: 4 roundings; the sum of c terms adds at most c more
       in any order (lane-serial, then the shuffle tree); dflow of the warp with accumulate adds 1, backwarp's factor
       scale * (W / (W - 1)) and its product 3.  So n_r = c + 4 (+ 1, + 3).  din sums at most h*w atomic adds of
       w * d, w = wy * wx: n_r = h*w + 2.
  dpos the fp32 position error: the warp's ix takes 6 roundings (the add of x + 0.5 and the flow, the division by W,
       - 1, + 1, the product with W, - 1; the products with 2 and the division by 2 are exact), each at most 2^-24
       of a magnitude <= M = max(h, w) + max|flow| + 2 once carried to pixel units, so dpos = 6 * 2^-24 * M;
       backwarp's takes 8 (flow * scale, (2x + 1) / W, the add to -1, the division by (W - 1) / 2, the add, + 1, the
       product with W, - 1): dpos = 8 * 2^-24 * M.  A weight moves by at most dpos, so the output by at most
       dpos * S2, S2 = sum |d| (|v00| + |v01| + |v10| + |v11|) (din: 2 dpos * sum of the |d| that reach the pixel).
Nothing here is stored in 16 bits (dflow and din are fp32), so no 0.5 u term appears at op level."""
import pytest
import torch
import torch.nn.functional as F

from tests.pwc_ref import assert_single_rounding

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SENT = 3.0
U = 2.0 ** -24
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


@pytest.fixture(scope='module')
def L():
    from dbsr_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope='module')
def ops():
    from dbsr_amd import ops as O
    return O


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def grid_values(shape, lo, hi, g):
    """k / 8 + 1 / 16 for random integers k, values in [lo, hi)."""
    k = torch.randint(int(lo * 8), int(hi * 8), shape, generator=g)
    return k.double() / 8.0 + 1.0 / 16.0


def _xy(h, w):
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing='ij')
    return xs, ys


def positions_to_flow(tx, ty, h, w):
    """Warp flow [n,2,h,w] (float64) whose sample positions are (tx, ty) [n,h,w]."""
    xs, ys = _xy(h, w)
    return torch.stack((tx - xs, ty - ys), dim=1)


def flow_set(kind, n, h, w, g):
    """Warp flows [n,2,h,w] float32 on the 1/8 grid + 1/16 (integers for 'integer')."""
    if kind == 'random':
        return grid_values((n, 2, h, w), -2.5, 2.5 - 0.125, g).float()
    if kind == 'integer':
        return torch.randint(-2, 3, (n, 2, h, w), generator=g).float()
    frac = grid_values((n, h, w), 0.0, 1.0, g)                      # in (0, 1), 1/16 from both ends
    tx = grid_values((n, h, w), 0.0, float(w - 1), g)               # inside, all corners in bounds
    ty = grid_values((n, h, w), 0.0, float(h - 1), g)
    sel = torch.arange(n * h * w).view(n, h, w)
    if kind == 'far':           # more than one pixel outside on the left / right / top / bottom
        side = sel % 4
        tx = torch.where(side == 0, -1.0 - frac, torch.where(side == 1, w + frac, tx))
        ty = torch.where(side == 2, -1.0 - frac, torch.where(side == 3, h + frac, ty))
    elif kind == 'band':        # the one-pixel bands just outside and just inside each edge
        side = sel % 8
        for s, v in ((0, -1.0 + frac), (1, frac), (2, w - 2 + frac), (3, w - 1 + frac)):
            tx = torch.where(side == s, v, tx)
        for s, v in ((4, -1.0 + frac), (5, frac), (6, h - 2 + frac), (7, h - 1 + frac)):
            ty = torch.where(side == s, v, ty)
    else:
        raise ValueError(kind)
    return positions_to_flow(tx, ty, h, w).float()


def corners(feat, ix, iy):
    """Zero-padded corner values v00, v01, v10, v11 [n,c,h,w] and weights wx0, wx1, wy0, wy1 [n,1,h,w] of bilinear
    sampling feat (float64) at (ix, iy) [n,h,w], plus the flat corner indices and validity (for the transpose)."""
    n, c, h, w = feat.shape
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = (ix - x0).unsqueeze(1), (iy - y0).unsqueeze(1)
    flat = feat.flatten(2)
    vals, idxs, oks = [], [], []
    for dy in (0, 1):
        for dx in (0, 1):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
            idx = (yi.clamp(0, h - 1) * w + xi.clamp(0, w - 1)).flatten(1)
            v = flat.gather(2, idx.unsqueeze(1).expand(-1, c, -1)).view(n, c, h, w) * ok.unsqueeze(1)
            vals.append(v)
            idxs.append(idx)
            oks.append(ok.flatten(1))
    return vals, (1 - wx1, wx1, 1 - wy1, wy1), idxs, oks


def flow_terms(feat, dout, ix, iy):
    """(gx, gy, Sx, Sy, S2): the two position gradients sum_c d * d(sample)/d{ix, iy} and the bound's sums."""
    (v00, v01, v10, v11), (wx0, wx1, wy0, wy1), _, _ = corners(feat, ix, iy)
    gx = (dout * (wy0 * (v01 - v00) + wy1 * (v11 - v10))).sum(1)
    gy = (dout * (wx0 * (v10 - v00) + wx1 * (v11 - v01))).sum(1)
    a = dout.abs()
    sx = (a * (wy0 * (v01.abs() + v00.abs()) + wy1 * (v11.abs() + v10.abs()))).sum(1)
    sy = (a * (wx0 * (v10.abs() + v00.abs()) + wx1 * (v11.abs() + v01.abs()))).sum(1)
    s2 = (a * (v00.abs() + v01.abs() + v10.abs() + v11.abs())).sum(1)
    return gx, gy, sx, sy, s2


# ----------------------------------------------------------------------------------------------------
# dbsr_warp_flow_backward
# ----------------------------------------------------------------------------------------------------
def run_warp_flow_backward(L, feat, dout, flow, sliced=False, framed=False, padded=False, base=None):
    """The kernel on feat / dout [n,c,h,w] (device dtype) and flow [n,2,h,w]: a packed tensor or a slice (ld > c,
    c0 = 8, NaN in the other channels), the identity map or the trainer's (N-1, N, 1, 1) map on feat (frame 0 NaN),
    flow / dflow image strides of 2hw or more.  base None: accumulate 0 into a sentinel-filled buffer; else
    accumulate 1 onto base.  Checks that nothing outside the result was written; returns it [n,2,h,w] on the CPU."""
    n, c, h, w = feat.shape
    dt = feat.dtype
    ld, c0 = (c + 16, 8) if sliced else (c, 0)
    f0 = 1 if framed else 0
    fb = torch.full((n + f0, h, w, ld), float('nan'), dtype=dt, device=DEV)
    fb[f0:, ..., c0:c0 + c] = feat.permute(0, 2, 3, 1).to(DEV)
    db = torch.full((n, h, w, ld), float('nan'), dtype=dt, device=DEV)
    db[..., c0:c0 + c] = dout.permute(0, 2, 3, 1).to(DEV)
    hw2 = 2 * h * w
    fis, dis = (hw2 + 7, hw2 + 5) if padded else (hw2, hw2)
    flb = torch.full((n, fis), float('nan'), dtype=torch.float32, device=DEV)
    flb[:, :hw2] = flow.reshape(n, hw2).to(DEV)
    G = 32
    ob = torch.full((G + n * dis + G,), SENT, dtype=torch.float32, device=DEV)
    view = ob[G:G + n * dis].view(n, dis)
    if base is not None:
        view[:, :hw2] = base.reshape(n, hw2).to(DEV)
    fmap = (n, n + 1, 1, 1) if framed else L.IDENTITY
    rc = L.lib().dbsr_warp_flow_backward(n, h, w, c, L.tensor_desc(fb, ld, c0, img_stride=h * w * ld, fmap=fmap),
                                         L.tensor_desc(db, ld, c0, img_stride=h * w * ld), flb.data_ptr(), fis,
                                         view.data_ptr(), dis, 0 if base is None else 1, L.stream_ptr(DEV))
    L.check(rc, 'dbsr_warp_flow_backward')
    torch.cuda.synchronize()
    assert bool((ob[:G] == SENT).all()) and bool((ob[G + n * dis:] == SENT).all()), 'wrote outside dflow'
    assert bool((view[:, hw2:] == SENT).all()), 'wrote between the dflow images'
    return view[:, :hw2].reshape(n, 2, h, w).cpu()


def warp_reference(feat64, dout64, flow64):
    """float64 autograd through oracle.warp, and the bound's sums."""
    from oracle import dbsr_oracle as orc
    n, c, h, w = feat64.shape
    fl = flow64.clone().requires_grad_()
    (orc.warp(feat64, fl) * dout64).sum().backward()
    xs, ys = _xy(h, w)
    gx, gy, sx, sy, s2 = flow_terms(feat64, dout64, xs + flow64[:, 0], ys + flow64[:, 1])
    manual = torch.stack((gx, gy), 1)
    # the two float64 computations of the same thing agree (the closed form in the header is the autograd result)
    assert float((manual - fl.grad).abs().max()) <= 1e-9 * max(1.0, float(fl.grad.abs().max()))
    return fl.grad, torch.stack((sx, sy), 1), torch.stack((s2, s2), 1)


def warp_bound(S, S2, c, h, w, flow, extra_roundings=0, base=None):
    dpos = 6 * U * (max(h, w) + float(flow.abs().max()) + 2.0)
    n_r = c + 4 + extra_roundings
    A = n_r * U * S + dpos * S2
    if base is not None:
        A = A + n_r * U * base.double().abs()
    return n_r, A


def _operands(n, c, h, w, dtype, seed):
    g = _gen(seed)
    feat = torch.randn(n, c, h, w, generator=g).to(dtype)
    dout = torch.randn(n, c, h, w, generator=g).to(dtype)
    return feat, dout, g


WARP_SHAPES = [(3, 5, 7, 8), (2, 4, 8, 24), (2, 9, 6, 512),
               (1, 5, 7, 512), (1, 3, 5, 1024)]     # 35 pixels: a wave of the 512-channel kernel partly past the end; 2 lane passes


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', WARP_SHAPES)
def test_warp_flow_backward(L, shape, dtype):
    """Every layout (packed / slice, identity / trainer frame map, padded strides, accumulate 0 / 1) on the random
    flows, and the far-outside (exactly 0) and edge-band (zero-padding gradient) flow sets."""
    n, h, w, c = shape
    feat, dout, g = _operands(n, c, h, w, dtype, 11)
    f64, d64 = feat.double(), dout.double()
    flow = flow_set('random', n, h, w, g)
    ref, S, S2 = warp_reference(f64, d64, flow.double())
    n_r, A = warp_bound(S, S2, c, h, w, flow)
    for sliced in (False, True):
        for framed in (False, True):
            for padded in (False, True):
                out = run_warp_flow_backward(L, feat, dout, flow, sliced, framed, padded)
                assert_single_rounding(out, ref, S, n_r, torch.float32,
                                       'warp_flow_backward %s %s slice %d map %d pad %d' % (shape, dtype, sliced, framed, padded), A=A)
    base = torch.randn(n, 2, h, w, generator=g)
    n_ra, Aa = warp_bound(S, S2, c, h, w, flow, extra_roundings=1, base=base)
    for sliced, framed, padded in ((False, False, False), (True, True, True)):
        out = run_warp_flow_backward(L, feat, dout, flow, sliced, framed, padded, base=base)
        assert_single_rounding(out, ref + base.double(), S, n_ra, torch.float32,
                               'warp_flow_backward accumulate %s %s' % (shape, dtype), A=Aa)
    # every sample more than one pixel outside, on each of the four sides: exactly 0, whatever was there before
    far = flow_set('far', n, h, w, g)
    ref_far, _, _ = warp_reference(f64, d64, far.double())
    assert float(ref_far.abs().max()) == 0.0
    out = run_warp_flow_backward(L, feat, dout, far, sliced=True, framed=True, padded=True)
    assert bool((out == 0).all()), 'far outside: dflow must be exactly 0'
    # the bands just outside / inside the edges: some corners out of bounds, the gradient comes from the padding
    band = flow_set('band', n, h, w, g)
    ref_b, Sb, S2b = warp_reference(f64, d64, band.double())
    assert float(ref_b.abs().max()) > 0.0
    n_rb, Ab = warp_bound(Sb, S2b, c, h, w, band)
    for sliced, framed in ((False, False), (True, True)):
        out = run_warp_flow_backward(L, feat, dout, band, sliced, framed, False)
        assert_single_rounding(out, ref_b, Sb, n_rb, torch.float32, 'warp_flow_backward band %s %s' % (shape, dtype), A=Ab)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', [(2, 4, 8, 8), (1, 16, 16, 24)])
def test_warp_flow_backward_integer_flows(L, shape, dtype):
    """Integer flows at power-of-two sizes: the position arithmetic is exact in fp32, the sample sits on a pixel and
    the kernel must take floor's cell (weights 1 and 0) as grid_sample does."""
    n, h, w, c = shape
    feat, dout, g = _operands(n, c, h, w, dtype, 12)
    flow = flow_set('integer', n, h, w, g)
    ref, S, S2 = warp_reference(feat.double(), dout.double(), flow.double())
    n_r, A = warp_bound(S, S2, c, h, w, flow)
    out = run_warp_flow_backward(L, feat, dout, flow)
    assert_single_rounding(out, ref, S, n_r, torch.float32, 'warp_flow_backward integer %s %s' % (shape, dtype), A=A)


# ----------------------------------------------------------------------------------------------------
# dbsr_backwarp_backward
# ----------------------------------------------------------------------------------------------------
def backwarp_positions(flow64, scale, h, w):
    """The sample positions (ix, iy) [n,h,w] of backwarp(input, flow * scale) in float64."""
    xs, ys = _xy(h, w)
    return xs + flow64[:, 0] * scale * (w / (w - 1.0)), ys + flow64[:, 1] * scale * (h / (h - 1.0))


def backwarp_flow(n, h, w, scale, g, kind='random'):
    """fp32 flows [n,2,h,w] whose sample positions lie on the 1/8 grid + 1/16 (to fp32 rounding of the flow, ~1e-7
    px): 'random' within about +-2.5 px of the pixel (so some leave the image), 'out': every sample in the band just
    outside the left edge (mask 0 everywhere)."""
    xs, ys = _xy(h, w)
    if kind == 'out':
        tx = -1.0 + grid_values((n, h, w), 0.0, 1.0, g)
        ty = grid_values((n, h, w), 0.0, float(h - 1), g)
    else:
        tx = xs + grid_values((n, h, w), -2.5, 2.5 - 0.125, g)
        ty = ys + grid_values((n, h, w), -2.5, 2.5 - 0.125, g)
    fx = (tx - xs) * ((w - 1.0) / w) / scale
    fy = (ty - ys) * ((h - 1.0) / h) / scale
    return torch.stack((fx, fy), 1).float()


def run_backwarp_backward(L, inp, flow, dout, scale, want_in=True, want_flow=True):
    """The kernel on inp / dout [n,c,h,w] (device dtype) and flow [n,2,h,w] fp32: (din [n,c,h,w], dflow [n,2,h,w])
    on the CPU, None for the one not asked for.  Output buffers are sentinel-filled; pad channels must stay."""
    n, c, h, w = inp.shape
    dt = inp.dtype
    ld = (c + 7) // 8 * 8 + 8
    xb = torch.zeros(n, h, w, ld, dtype=dt, device=DEV)
    xb[..., :c] = inp.permute(0, 2, 3, 1).to(DEV)
    db = torch.zeros(n, h, w, ld, dtype=dt, device=DEV)
    db[..., :c] = dout.permute(0, 2, 3, 1).to(DEV)
    fb = torch.full((n, h, w, 4), float('nan'), dtype=torch.float32, device=DEV)
    fb[..., 1:3] = flow.permute(0, 2, 3, 1).to(DEV)                       # flow in channels [1, 3) of 4
    di = torch.full((n, h, w, ld), SENT, dtype=torch.float32, device=DEV)
    df = torch.full((n, h, w, 4), SENT, dtype=torch.float32, device=DEV)
    rc = L.lib().dbsr_backwarp_backward(n, h, w, c, L.tensor_desc(xb, ld), L.tensor_desc(fb, 4, 1), float(scale),
                                        L.tensor_desc(db, ld), L.tensor_desc(di, ld) if want_in else L.NULL_TENSOR,
                                        L.tensor_desc(df, 4, 2) if want_flow else L.NULL_TENSOR, L.stream_ptr(DEV))
    L.check(rc, 'dbsr_backwarp_backward')
    torch.cuda.synchronize()
    assert bool((di[..., c:] == SENT).all()) and bool((df[..., :2] == SENT).all()), 'wrote outside the slices'
    if not want_in:
        assert bool((di == SENT).all())
    if not want_flow:
        assert bool((df == SENT).all())
    return (di[..., :c].permute(0, 3, 1, 2).cpu() if want_in else None,
            df[..., 2:].permute(0, 3, 1, 2).cpu() if want_flow else None)


def backwarp_reference(inp64, flow64, dout64, scale):
    """float64 autograd through oracle.backwarp(input, flow * scale), the mask, and the bounds' sums."""
    from oracle import dbsr_oracle as orc
    n, c, h, w = inp64.shape
    x = inp64.clone().requires_grad_()
    fl = flow64.clone().requires_grad_()
    (orc.backwarp(x, fl * scale) * dout64).sum().backward()
    ix, iy = backwarp_positions(flow64, scale, h, w)
    gx, gy, sx, sy, s2 = flow_terms(inp64, dout64, ix, iy)
    _, (wx0, wx1, wy0, wy1), idxs, oks = corners(inp64, ix, iy)
    wts = [wy0 * wx0, wy0 * wx1, wy1 * wx0, wy1 * wx1]
    mass = sum(wt.flatten(1).squeeze(1) * ok for wt, ok in zip(wts, oks)).view(n, h, w)
    mask = (mass > 0.999).double()
    fac = torch.tensor([scale * w / (w - 1.0), scale * h / (h - 1.0)], dtype=torch.float64).view(1, 2, 1, 1)
    m1 = mask.unsqueeze(1)
    S = torch.stack((sx, sy), 1) * m1 * fac.abs()
    S2 = torch.stack((s2, s2), 1) * m1 * fac.abs()
    # din: S = the transpose on absolute values; T = the sum of the |d| that reach a pixel
    a = (dout64.abs() * m1).flatten(2)
    Sd = torch.zeros(n, c, h * w, dtype=torch.float64)
    T = torch.zeros(n, c, h * w, dtype=torch.float64)
    for wt, idx, ok in zip(wts, idxs, oks):
        k = (wt.flatten(2) * ok.unsqueeze(1)).expand(-1, c, -1)
        Sd.scatter_add_(2, idx.unsqueeze(1).expand(-1, c, -1).contiguous(), a * k)
        T.scatter_add_(2, idx.unsqueeze(1).expand(-1, c, -1).contiguous(), a * ok.unsqueeze(1))
    raw = torch.stack((gx, gy), 1)
    return dict(din=x.grad, dflow=fl.grad, mask=mask, S=S, S2=S2, Sd=Sd.view(n, c, h, w), T=T.view(n, c, h, w),
                raw=raw, ix=ix, iy=iy)


BACKWARP_SHAPES = [(2, 4, 4, 16), (3, 6, 10, 32), (1, 8, 8, 128)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('scale', [1.0, 0.625, 5.0])
@pytest.mark.parametrize('shape', BACKWARP_SHAPES)
def test_backwarp_backward(L, shape, scale, dtype):
    n, h, w, c = shape
    inp, dout, g = _operands(n, c, h, w, dtype, 21)
    flow = backwarp_flow(n, h, w, scale, g)
    r = backwarp_reference(inp.double(), flow.double(), dout.double(), scale)
    assert 0 < int(r['mask'].sum()) < r['mask'].numel(), 'the case needs kept and masked pixels'
    M = max(h, w) + float(max(r['ix'].abs().max(), r['iy'].abs().max())) + 2.0
    dpos = 8 * U * M
    n_rf, Af = c + 4 + 3, (c + 4 + 3) * U * r['S'] + dpos * r['S2']
    n_rd, Ad = h * w + 2, (h * w + 2) * U * r['Sd'] + 2 * dpos * r['T']
    what = 'backwarp_backward %s scale %g %s' % (shape, scale, dtype)
    din, dfl = run_backwarp_backward(L, inp, flow, dout, scale)
    assert_single_rounding(dfl, r['dflow'], r['S'], n_rf, torch.float32, what + ' dflow', A=Af)
    assert_single_rounding(din, r['din'], r['Sd'], n_rd, torch.float32, what + ' din', A=Ad)
    # where the mask is 0 the flow gradient is exactly 0 (and the reference's is)
    gone = (r['mask'] == 0).unsqueeze(1).expand(-1, 2, -1, -1)
    assert bool((dfl[gone] == 0).all()) and bool((r['dflow'][gone] == 0).all())
    # each output alone, the other a null tensor: the same values (dflow bitwise: it is owner-computes)
    din1, none = run_backwarp_backward(L, inp, flow, dout, scale, want_flow=False)
    assert none is None
    assert_single_rounding(din1, r['din'], r['Sd'], n_rd, torch.float32, what + ' din alone', A=Ad)
    none, dfl1 = run_backwarp_backward(L, inp, flow, dout, scale, want_in=False)
    assert none is None and torch.equal(dfl1, dfl)
    # the factor scale * W / (W - 1) at an interior pixel (all four corners in bounds), against a central finite
    # difference of the float64 reference: bilinear sampling is linear inside the cell, so the difference quotient
    # is the derivative up to float64 rounding, and a missing factor is a 1 / (W - 1) relative error
    from oracle import dbsr_oracle as orc
    inside = (r['ix'] > 0) & (r['ix'] < w - 1) & (r['iy'] > 0) & (r['iy'] < h - 1)
    p, y, x = [int(v) for v in torch.nonzero(inside)[0]]
    i64, d64, f64 = inp.double(), dout.double(), flow.double()
    eps = 2.0 ** -12 / scale
    for ch, (size, name) in enumerate(((w, 'x'), (h, 'y'))):
        def loss(delta):
            f = f64.clone()
            f[p, ch, y, x] += delta
            return float((orc.backwarp(i64, f * scale) * d64).sum())
        fd = (loss(eps) - loss(-eps)) / (2 * eps)
        want = float(r['raw'][p, ch, y, x]) * scale * size / (size - 1.0)
        print('%s d%s at (%d,%d,%d): kernel %.9g, finite difference %.9g, raw * scale * %d/%d = %.9g'
              % (what, name, p, y, x, float(dfl[p, ch, y, x]), fd, size, size - 1, want))
        assert abs(fd - want) <= 1e-7 * max(1.0, abs(want))
        assert abs(float(dfl[p, ch, y, x]) - fd) <= float(Af[p, ch, y, x]) + 1e-7 * max(1.0, abs(fd))


@pytest.mark.parametrize('dtype', DTYPES)
def test_backwarp_backward_all_masked(L, dtype):
    """Every sample in the band just outside the left edge: the mask is 0 everywhere, both gradients exactly 0."""
    n, h, w, c = 2, 6, 10, 32
    inp, dout, g = _operands(n, c, h, w, dtype, 22)
    flow = backwarp_flow(n, h, w, 1.0, g, kind='out')
    r = backwarp_reference(inp.double(), flow.double(), dout.double(), 1.0)
    assert float(r['mask'].sum()) == 0 and float(r['din'].abs().max()) == 0 and float(r['dflow'].abs().max()) == 0
    din, dfl = run_backwarp_backward(L, inp, flow, dout, 1.0)
    assert bool((din == 0).all()) and bool((dfl == 0).all())


# ----------------------------------------------------------------------------------------------------
# operators
# ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tops():
    from dbsr_amd import torch_ops
    return torch_ops.load()


@pytest.mark.parametrize('dtype', DTYPES)
def test_warp_bilinear_autograd_both_inputs(tops, ops, dtype):
    """dbsr::warp_bilinear under autograd = the direct calls (the same kernels on the same operands)."""
    n, c, h, w = 2, 24, 7, 9
    feat, dout, g = _operands(n, c, h, w, dtype, 31)
    flow = flow_set('random', n, h, w, g)
    x = feat.to(DEV).requires_grad_()
    fl = flow.to(DEV).requires_grad_()
    out = tops.warp_bilinear(x, fl)
    out.backward(dout.to(DEV))
    dflow = ops.warp_flow_backward(feat.to(DEV), dout.to(DEV), flow.to(DEV))
    dfeat = ops.warp_backward(dout.to(DEV), flow.to(DEV))
    assert fl.grad.dtype == torch.float32 and torch.equal(fl.grad, dflow)               # deterministic kernel
    torch.testing.assert_close(x.grad.float(), dfeat.to(dtype).float(), rtol=2e-2 if dtype != torch.float32 else 1e-5,
                               atol=1e-5)                                              # (atomics: summation order)
    # and against float64 autograd of the reference
    ref, S, S2 = warp_reference(feat.double(), dout.double(), flow.double())
    n_r, A = warp_bound(S, S2, (c + 7) // 8 * 8, h, w, flow)
    assert_single_rounding(fl.grad.cpu(), ref, S, n_r, torch.float32, 'dbsr::warp_bilinear dflow %s' % dtype, A=A)


def test_warp_bilinear_frozen_flow_launches_nothing(tops, monkeypatch):
    """flow.requires_grad=False: no flow gradient, and the flow-backward operator is never called."""
    calls = []
    real = torch.ops.dbsr.warp_bilinear_flow_backward

    def spy(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(torch.ops.dbsr, 'warp_bilinear_flow_backward', spy)
    feat, dout, g = _operands(2, 8, 5, 6, torch.float32, 32)
    flow = flow_set('random', 2, 5, 6, g).to(DEV)
    x = feat.to(DEV).requires_grad_()
    tops.warp_bilinear(x, flow).backward(dout.to(DEV))
    assert x.grad is not None and flow.grad is None and not calls
    fl = flow.clone().requires_grad_()
    tops.warp_bilinear(feat.to(DEV), fl).backward(dout.to(DEV))        # the spy does see the call when it happens
    assert fl.grad is not None and len(calls) == 1


@pytest.mark.parametrize('dtype', DTYPES)
def test_backwarp_autograd_both_inputs(tops, ops, dtype):
    n, c, h, w = 2, 32, 6, 10
    inp, dout, g = _operands(n, c, h, w, dtype, 33)
    flow = backwarp_flow(n, h, w, 1.0, g)
    x = inp.to(DEV).requires_grad_()
    fl = flow.to(DEV).requires_grad_()
    tops.backwarp(x, fl).backward(dout.to(DEV))
    din, dfl = ops.backwarp_backward(inp.to(DEV), flow.to(DEV), dout.to(DEV))
    assert torch.equal(fl.grad, dfl)
    torch.testing.assert_close(x.grad.float(), din.to(dtype).float(), rtol=2e-2 if dtype != torch.float32 else 1e-5,
                               atol=1e-5)
    r = backwarp_reference(inp.double(), flow.double(), dout.double(), 1.0)
    torch.testing.assert_close(fl.grad.cpu().double(), r['dflow'], rtol=1e-4, atol=1e-4)
    # one input only
    x2 = inp.to(DEV).requires_grad_()
    tops.backwarp(x2, flow.to(DEV)).backward(dout.to(DEV))
    torch.testing.assert_close(x2.grad, x.grad, rtol=1e-5, atol=1e-6)
    fl2 = flow.to(DEV).requires_grad_()
    tops.backwarp(inp.to(DEV), fl2).backward(dout.to(DEV))
    assert torch.equal(fl2.grad, fl.grad)


# ----------------------------------------------------------------------------------------------------
# trainer
# ----------------------------------------------------------------------------------------------------
B, N, H, W, BI = 2, 3, 16, 16, 40            # x8: 128 x 128 predictions, a 48 x 48 crop inside boundary_ignore 40

# DBSRTrainer's op names at this shape (fp32) before the flow gradient existed: flow_grad=False must build these
PARENT_OPS = [
    'repack.all', 'pack_burst', 'pwc.ext1.0', 'pwc.ext1.2', 'pwc.ext1.4', 'pwc.ext2.0', 'pwc.ext2.2',
    'pwc.ext2.4', 'pwc.ext3.0', 'pwc.ext3.2', 'pwc.ext3.4', 'pwc.ext4.0', 'pwc.ext4.2', 'pwc.ext4.4',
    'pwc.ext5.0', 'pwc.ext5.2', 'pwc.ext5.4', 'pwc.ext6.0', 'pwc.ext6.2', 'pwc.ext6.4', 'pwc.dec6.corr',
    'pwc.dec6.dense0', 'pwc.dec6.dense1', 'pwc.dec6.dense2', 'pwc.dec6.dense3', 'pwc.dec6.dense4',
    'pwc.dec6.flow', 'pwc.dec5.upflow', 'pwc.dec5.upfeat', 'pwc.dec5.backwarp', 'pwc.dec5.assemble',
    'pwc.dec5.corr', 'pwc.dec5.dense0', 'pwc.dec5.dense1', 'pwc.dec5.dense2', 'pwc.dec5.dense3',
    'pwc.dec5.dense4', 'pwc.dec5.flow', 'pwc.dec4.upflow', 'pwc.dec4.upfeat', 'pwc.dec4.backwarp',
    'pwc.dec4.assemble', 'pwc.dec4.corr', 'pwc.dec4.dense0', 'pwc.dec4.dense1', 'pwc.dec4.dense2',
    'pwc.dec4.dense3', 'pwc.dec4.dense4', 'pwc.dec4.flow', 'pwc.dec3.upflow', 'pwc.dec3.upfeat',
    'pwc.dec3.backwarp', 'pwc.dec3.assemble', 'pwc.dec3.corr', 'pwc.dec3.dense0', 'pwc.dec3.dense1',
    'pwc.dec3.dense2', 'pwc.dec3.dense3', 'pwc.dec3.dense4', 'pwc.dec3.flow', 'pwc.dec2.upflow',
    'pwc.dec2.upfeat', 'pwc.dec2.backwarp', 'pwc.dec2.assemble', 'pwc.dec2.corr', 'pwc.dec2.dense0',
    'pwc.dec2.dense1', 'pwc.dec2.dense2', 'pwc.dec2.dense3', 'pwc.dec2.dense4', 'pwc.dec2.flow', 'pwc.refiner0',
    'pwc.refiner1', 'pwc.refiner2', 'pwc.refiner3', 'pwc.refiner4', 'pwc.refiner5', 'pwc.refiner6',
    'flow_finalize', 'ofe.init', 'ofe.res0.conv1', 'ofe.res0.conv2', 'enc.init', 'enc.res0.conv1',
    'enc.res0.conv2', 'enc.res1.conv1', 'enc.res1.conv2', 'enc.res2.conv1', 'enc.res2.conv2', 'enc.res3.conv1',
    'enc.res3.conv2', 'enc.res4.conv1', 'enc.res4.conv2', 'enc.res5.conv1', 'enc.res5.conv2', 'enc.res6.conv1',
    'enc.res6.conv2', 'enc.res7.conv1', 'enc.res7.conv2', 'enc.res8.conv1', 'enc.res8.conv2', 'enc.out',
    'proj_ref', 'warp', 'proj_oth', 'merge_prep', 'wp.init', 'wp.res0.conv1', 'wp.res0.conv2', 'wp.res1.conv1',
    'wp.res1.conv2', 'wp.res2.conv1', 'wp.res2.conv2', 'wp.out', 'fuse', 'dec.init', 'dec.pre0.conv1',
    'dec.pre0.conv2', 'dec.pre1.conv1', 'dec.pre1.conv2', 'dec.pre2.conv1', 'dec.pre2.conv2', 'dec.pre3.conv1',
    'dec.pre3.conv2', 'dec.pre4.conv1', 'dec.pre4.conv2', 'dec.upsample', 'dec.blur', 'dec.post0.conv1',
    'dec.post0.conv2', 'dec.post1.conv1', 'dec.post1.conv2', 'dec.post2.conv1', 'dec.post2.conv2',
    'dec.post3.conv1', 'dec.post3.conv2', 'dec.predictor', 'zero_grad', 'l1_loss_bwd', 'bwd.dec.predictor',
    'bwd.dec.post3.conv2', 'wgrad.dec.post3.conv2', 'bwd.dec.post3.conv1', 'wgrad.dec.post3.conv1',
    'bwd.dec.post2.conv2', 'wgrad.dec.post2.conv2', 'bwd.dec.post2.conv1', 'wgrad.dec.post2.conv1',
    'bwd.dec.post1.conv2', 'wgrad.dec.post1.conv2', 'bwd.dec.post1.conv1', 'wgrad.dec.post1.conv1',
    'bwd.dec.post0.conv2', 'wgrad.dec.post0.conv2', 'bwd.dec.post0.conv1', 'wgrad.dec.post0.conv1',
    'bwd.dec.blur', 'bwd.dec.unshuffle', 'wgrad.dec.upsample', 'bwd.dec.upsample', 'bwd.dec.pre4.conv2',
    'wgrad.dec.pre4.conv2', 'bwd.dec.pre4.conv1', 'wgrad.dec.pre4.conv1', 'bwd.dec.pre3.conv2',
    'wgrad.dec.pre3.conv2', 'bwd.dec.pre3.conv1', 'wgrad.dec.pre3.conv1', 'bwd.dec.pre2.conv2',
    'wgrad.dec.pre2.conv2', 'bwd.dec.pre2.conv1', 'wgrad.dec.pre2.conv1', 'bwd.dec.pre1.conv2',
    'wgrad.dec.pre1.conv2', 'bwd.dec.pre1.conv1', 'wgrad.dec.pre1.conv1', 'bwd.dec.pre0.conv2',
    'wgrad.dec.pre0.conv2', 'bwd.dec.pre0.conv1', 'wgrad.dec.pre0.conv1', 'wgrad.dec.init', 'bwd.dec.init',
    'bwd.fuse', 'wgrad.wp.out', 'bwd.wp.out', 'bwd.wp.res2.conv2', 'wgrad.wp.res2.conv2', 'bwd.wp.res2.conv1',
    'wgrad.wp.res2.conv1', 'bwd.wp.res1.conv2', 'wgrad.wp.res1.conv2', 'bwd.wp.res1.conv1',
    'wgrad.wp.res1.conv1', 'bwd.wp.res0.conv2', 'wgrad.wp.res0.conv2', 'bwd.wp.res0.conv1',
    'wgrad.wp.res0.conv1', 'wgrad.wp.init', 'bwd.wp.init.bd', 'bwd.wp.init.of', 'bwd.ofe.res0.conv2',
    'wgrad.ofe.res0.conv2', 'bwd.ofe.res0.conv1', 'wgrad.ofe.res0.conv1', 'wgrad.ofe.init', 'bwd.merge_prep',
    'wgrad.proj.ref', 'wgrad.proj.oth', 'bwd.proj.ref', 'bwd.proj.oth', 'bwd.warp', 'bwd.enc.gate',
    'wgrad.enc.out', 'bwd.enc.out', 'bwd.enc.res8.conv2', 'wgrad.enc.res8.conv2', 'bwd.enc.res8.conv1',
    'wgrad.enc.res8.conv1', 'bwd.enc.res7.conv2', 'wgrad.enc.res7.conv2', 'bwd.enc.res7.conv1',
    'wgrad.enc.res7.conv1', 'bwd.enc.res6.conv2', 'wgrad.enc.res6.conv2', 'bwd.enc.res6.conv1',
    'wgrad.enc.res6.conv1', 'bwd.enc.res5.conv2', 'wgrad.enc.res5.conv2', 'bwd.enc.res5.conv1',
    'wgrad.enc.res5.conv1', 'bwd.enc.res4.conv2', 'wgrad.enc.res4.conv2', 'bwd.enc.res4.conv1',
    'wgrad.enc.res4.conv1', 'bwd.enc.res3.conv2', 'wgrad.enc.res3.conv2', 'bwd.enc.res3.conv1',
    'wgrad.enc.res3.conv1', 'bwd.enc.res2.conv2', 'wgrad.enc.res2.conv2', 'bwd.enc.res2.conv1',
    'wgrad.enc.res2.conv1', 'bwd.enc.res1.conv2', 'wgrad.enc.res1.conv2', 'bwd.enc.res1.conv1',
    'wgrad.enc.res1.conv1', 'bwd.enc.res0.conv2', 'wgrad.enc.res0.conv2', 'bwd.enc.res0.conv1',
    'wgrad.enc.res0.conv1', 'wgrad.enc.init']


@pytest.fixture(scope='module')
def flow_case(synth_sd):
    """The burst, ground truth, an external flow on the 1/8 grid + 1/16 and the oracle's loss and gradients with
    oracle.pwcnet returning that flow as a float32 leaf (computed once, shared by the trainer tests)."""
    from dbsr_amd.burst import synthetic_bursts
    from oracle import dbsr_oracle as orc
    burst, gt = synthetic_bursts(B, N, H, W, sr_factor=8, seed=41)
    flow = flow_set('random', B * (N - 1), H, W, _gen(42))
    sd = {k: v.clone().requires_grad_(not k.startswith('encoder.alignment_net')) for k, v in synth_sd.items()}
    leaf = flow.clone().requires_grad_()
    real = orc.pwcnet
    orc.pwcnet = lambda *a, **k: leaf
    try:
        pred, aux = orc.dbsr_forward(burst, sd)
    finally:
        orc.pwcnet = real
    loss = F.l1_loss(pred[..., BI:-BI, BI:-BI], gt[..., BI:-BI, BI:-BI])
    loss.backward()
    return dict(burst=burst, gt=gt, flow=flow.view(B, N - 1, 2, H, W), loss=float(loss.detach()),
                gflow=leaf.grad.view(B, N - 1, 2, H, W), grads={k: v.grad for k, v in sd.items() if v.grad is not None})


def _net(synth_sd, dtype):
    import dbsr_amd
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    net.load_state_dict(synth_sd)
    return net.to(DEV).set_compute_dtype(dtype)


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-12))


def _cos(a, b):
    return 1 - float(F.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))


@pytest.mark.parametrize('dtype', DTYPES)
def test_trainer_flow_grad_vs_oracle(synth_sd, flow_case, dtype):
    """flow_grad() and the parameter gradients of the same run against autograd through the oracle, at the bars of
    test_train_step_grads_vs_oracle: fp32 1 - cos <= 1e-4 and max-rel <= 2e-2, 16-bit 1 - cos <= 3e-2 (fp16 with
    the loss scaler on: flow_grad() comes back unscaled)."""
    from dbsr_amd.training import DBSRTrainer
    fc = flow_case
    net = _net(synth_sd, dtype)
    tr = DBSRTrainer(net, boundary_ignore=BI, flow_grad=True)
    assert tr.scaling == (dtype == torch.float16)
    loss, _ = tr.forward_backward(fc['burst'].to(DEV), fc['gt'].to(DEV), flow=fc['flow'].to(DEV))
    torch.cuda.synchronize()
    assert not tr.found_inf()
    assert (B, N, H, W, 'flow') in tr.plans and (B, N, H, W) not in tr.plans        # keyed apart from the PWC plan
    names = [o[2] for o in tr.plans[(B, N, H, W, 'flow')].ops]
    assert not any(n.startswith('pwc') or n == 'flow_finalize' for n in names) and 'offsets_export' in names
    fg = tr.flow_grad()
    assert fg.shape == (B, N - 1, 2, H, W) and fg.dtype == torch.float32
    fg = fg.cpu()
    rel, cos = _rel(fg, fc['gflow']), _cos(fg, fc['gflow'])
    print('flow_grad %s: loss %.8g (oracle %.8g), max-rel %.3g, 1-cos %.3g, max|g| %.3g'
          % (dtype, float(loss), fc['loss'], rel, cos, float(fc['gflow'].abs().max())))
    mine = {k: v.cpu() for k, v in tr.grads().items()}
    assert set(mine) == set(fc['grads'])
    gmax = max(float(g.abs().max()) for g in fc['grads'].values())
    prel, pcos = [], []
    for k, g in fc['grads'].items():
        if k == 'merging.weight_predictor.4.0.bias':       # exact gradient 0 (softmax shift invariance)
            assert float(mine[k].abs().max()) <= 1e-4 * gmax
            continue
        prel.append((_rel(mine[k], g), k))
        pcos.append((_cos(mine[k], g), k))
    prel.sort(reverse=True)
    pcos.sort(reverse=True)
    print('parameters: max-rel worst', prel[:3], '1-cos worst', pcos[:3])
    if dtype == torch.float32:
        assert abs(float(loss) - fc['loss']) <= 1e-5 * max(1.0, abs(fc['loss']))
        assert cos <= 1e-4 and rel <= 2e-2, (cos, rel)
        assert prel[0][0] <= 2e-2 and pcos[0][0] <= 1e-4, (prel[:3], pcos[:3])
    else:
        assert abs(float(loss) - fc['loss']) <= 1e-2 * abs(fc['loss'])
        assert cos <= 3e-2, cos
        assert pcos[0][0] <= 3e-2, pcos[:3]


def test_trainer_op_names(synth_sd):
    """flow_grad=False builds exactly the op list the trainer built before the option existed; True adds only the
    two named ops, after bwd.ofe.res and bwd.proj.oth."""
    from dbsr_amd.training import DBSRTrainer
    net = _net(synth_sd, torch.float32)
    off = [o[2] for o in DBSRTrainer(net, boundary_ignore=BI)._build(B, N, H, W).ops]
    assert off == PARENT_OPS
    on = [o[2] for o in DBSRTrainer(net, boundary_ignore=BI, flow_grad=True)._build(B, N, H, W).ops]
    added = ['bwd.ofe.init.dgrad', 'bwd.warp.flow']
    assert [n for n in on if n not in added] == off and [n for n in on if n in added] == added
    i = on.index('bwd.ofe.init.dgrad')
    assert on[i + 1] == 'bwd.warp.flow'
    assert i > on.index('bwd.proj.oth') and i > max(k for k, n in enumerate(on) if n.startswith('bwd.ofe.res'))


def test_autograd_trains_an_alignment_module(synth_sd):
    """flow = my_alignment(burst); pred, _ = net(burst, flow=flow); loss.backward(): the alignment module's weight
    gradient is flow_grad chained through the module on the CPU."""
    from dbsr_amd.burst import synthetic_bursts
    burst, gt = synthetic_bursts(B, N, H, W, sr_factor=8, seed=43)
    torch.manual_seed(7)
    align = torch.nn.Conv2d(4, 2, 3, padding=1)
    cpu = torch.nn.Conv2d(4, 2, 3, padding=1)
    cpu.load_state_dict(align.state_dict())
    align = align.to(DEV)
    net = _net(synth_sd, torch.float32).train()
    for p in net.encoder.alignment_net.parameters():
        p.requires_grad_(False)
    b, g = burst.to(DEV), gt.to(DEV)
    flow = align(b[:, 1:].reshape(-1, 4, H, W)).view(B, N - 1, 2, H, W)
    pred, aux = net(b, flow=flow)
    assert pred.grad_fn is not None and torch.equal(aux['offsets'], flow.detach())
    F.l1_loss(pred[..., BI:-BI, BI:-BI], g[..., BI:-BI, BI:-BI]).backward()
    fg = net._train_engine.flow_grad().cpu()
    assert float(fg.abs().max()) > 0
    cpu(burst[:, 1:].reshape(-1, 4, H, W)).backward(fg.view(-1, 2, H, W))
    assert all(p.grad is not None for n, p in net.named_parameters() if not n.startswith('encoder.alignment_net'))
    torch.testing.assert_close(align.weight.grad.cpu(), cpu.weight.grad, rtol=1e-4, atol=1e-6 * float(cpu.weight.grad.abs().max()))
    torch.testing.assert_close(align.bias.grad.cpu(), cpu.bias.grad, rtol=1e-4, atol=1e-6 * float(cpu.bias.grad.abs().max()))


def test_eval_mode_refuses_external_flow(synth_sd):
    net = _net(synth_sd, torch.float32).eval()
    with pytest.raises(NotImplementedError, match='DBSRTrainer.forward_saved'):
        net(torch.zeros(1, N, 4, H, W, device=DEV), flow=torch.zeros(1, N - 1, 2, H, W, device=DEV))


def test_flow_grad_graph_replay_equals_eager(synth_sd, flow_case):
    """A flow_grad=True step replayed as a HIP graph (the second step; lr 0 keeps the weights) equals the eager
    first step bitwise: the loss and flow_grad."""
    from dbsr_amd.training import DBSRTrainer
    fc = flow_case
    net = _net(synth_sd, torch.float32)
    tr = DBSRTrainer(net, lr=0.0, boundary_ignore=BI, flow_grad=True)
    b, g, f = fc['burst'].to(DEV), fc['gt'].to(DEV), fc['flow'].to(DEV)
    l1 = tr.step(b, g, flow=f).clone()
    fg1 = tr.flow_grad().clone()
    plan = tr.plans[(B, N, H, W, 'flow')]
    assert plan.graphs is None
    l2 = tr.step(b, g, flow=f).clone()
    fg2 = tr.flow_grad().clone()
    torch.cuda.synchronize()
    assert plan.graphs is not None
    assert torch.equal(l1, l2) and torch.equal(fg1, fg2) and float(fg1.abs().max()) > 0
