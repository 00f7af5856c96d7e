"""Shared helpers of the op-level PWC-Net alignment tests (tests/test_gpu_pwc_stages.py, tests/test_gpu_pwc_ops.py):
the error unit, the single-rounding bound and the float64 references.

Error unit.  u(x) is the storage dtype's spacing at |x| (subnormal spacing below the smallest normal), floored at
the spacing at 2^-6 x the RMS of the reference tensor: a max-abs figure over a tensor hides errors in small
outputs, and small outputs are what a wrong edge tap produces.

Single-rounding bound.  A kernel that stores round16(fp32 sum) is within 0.5 u + A of the float64 value of the same
sum, A = n_r * 2^-24 * S: n_r sequential fp32 roundings (each at most 2^-24 relative to a partial sum, and every
partial sum is at most S in magnitude), S = sum |x_i * w_i| of that output (the same op on absolute values, float64).
u is taken at |ref| + A, the largest magnitude the fp32 sum can have (the spacing is monotone), so an fp32 sum that
crosses a binade boundary the float64 value does not is covered.  fp32 outputs are bounded by A alone (plus the
final fp32 store, counted in n_r)."""
import torch
import torch.nn.functional as F

MANT = {torch.float16: 10, torch.bfloat16: 7, torch.float32: 23}
EMIN = {torch.float16: -14, torch.bfloat16: -126, torch.float32: -126}
D16 = [torch.float16, torch.bfloat16]
SENTINEL = 3.0          # exact in fp16, bf16 and fp32


def rnd(t, dtype):
    """t rounded to the storage dtype, held as float64."""
    return t.to(dtype).double()


def spacing(x, dtype):
    """The dtype's spacing at |x| (float64 tensor), elementwise."""
    x = torch.as_tensor(x, dtype=torch.float64).abs()
    _, e = torch.frexp(x)                                  # |x| = m * 2^e, m in [0.5, 1): floor(log2 |x|) = e - 1
    e = torch.where(x > 0, e.double() - 1.0, torch.full_like(x, float(EMIN[dtype])))     # (frexp(0) has e = 0)
    e = torch.clamp(e, min=float(EMIN[dtype]))
    return torch.pow(torch.tensor(2.0, dtype=torch.float64), e - MANT[dtype])


def unit(ref, dtype, extra=None):
    """u per element: spacing at |ref| (+ extra), floored at the spacing at 2^-6 * rms(ref)."""
    ref = ref.double()
    mag = ref.abs() if extra is None else ref.abs() + extra
    rms = ref.pow(2).mean().sqrt()
    return torch.maximum(spacing(mag, dtype), spacing(rms * 2.0 ** -6, dtype))


def err_units(out, ref, dtype):
    """|out - ref| / u, elementwise (float64)."""
    return (out.double() - ref.double()).abs() / unit(ref, dtype)


def allowance(S, n_r):
    return n_r * 2.0 ** -24 * S.double()


def assert_single_rounding(out, ref, S, n_r, dtype, what, mask=None, A=None):
    """|out - ref| <= 0.5 u + A (16-bit storage) or A (fp32 storage).  Prints the worst ratio to the bound before
    asserting.  mask: elements compared (True) or left out.  A: the allowance itself where it has more terms than
    n_r 2^-24 S (n_r is then only printed)."""
    A = allowance(S, n_r) if A is None else A.double() + torch.zeros_like(ref.double())
    bound = A if dtype == torch.float32 else 0.5 * unit(ref, dtype, A) + A
    err = (out.double() - ref.double()).abs()
    if mask is not None:
        err = torch.where(mask, err, torch.zeros_like(err))
    # an output whose S is 0 (every product is zero) must be exact: bound 0 there, ratio taken as 0 / inf
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300),
                        torch.where(err > 0, torch.full_like(err, float('inf')), torch.zeros_like(err)))
    worst = ratio.max().item() if ratio.numel() else 0.0
    print('%s: n_r %d, worst |err| / bound %.3f, max |err| %.3g' % (what, n_r, worst, err.max().item()))
    bad = ratio > 1.0
    assert not bool(bad.any()), '%s: %d of %d elements beyond 0.5 u + A, worst %.3f x the bound at %s' % (
        what, int(bad.sum()), bad.numel(), worst, tuple(int(i) for i in torch.nonzero(bad)[0]))
    return worst


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def assert_bitwise(out, ref, what=''):
    assert out.dtype == ref.dtype and out.shape == ref.shape, (what, out.dtype, ref.dtype, out.shape, ref.shape)
    a, b = bits(out), bits(ref)
    assert torch.equal(a, b), '%s: %d of %d elements differ' % (what, int((a != b).sum()), a.numel())


def assert_sentinel(t, what=''):
    """Every element of t is bitwise the sentinel the buffer was prefilled with."""
    assert t.numel() > 0, what
    assert_bitwise(t, torch.full(t.shape, SENTINEL, dtype=t.dtype), what + ' (untouched sentinel)')


def assert_pos_zero(t, what=''):
    """Every element is exactly +0 (bitwise)."""
    assert t.numel() > 0, what
    assert_bitwise(t, torch.zeros(t.shape, dtype=t.dtype), what + ' (pad written as +0)')


def lrelu(x):
    return F.leaky_relu(x, 0.1)


def nchw(t):
    """[n, h, w, c] -> float64 [n, c, h, w] on the CPU."""
    return t.detach().cpu().double().permute(0, 3, 1, 2).contiguous()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def correlation64(first, second):
    """(cost volume, S): out[n, (dy+4)*9 + dx+4, y, x] = sum_c first[y, x] * second[y+dy, x+dx] / C, zero outside;
    S the same sum on absolute values (before the division)."""
    from oracle import dbsr_oracle as orc
    C = first.shape[1]
    return orc.correlation(first, second), orc.correlation(first.abs(), second.abs()) * C


def backwarp64(inp, flow):
    """pwcnet.py:16-38 in float64: grid_sample(bilinear, zeros, align_corners=False) at linspace(-1 + 1/W, 1 - 1/W)
    + flow / ((W - 1) / 2), times mask = (mass of the in-frame bilinear weights > 0.999).  Written out as the four
    gathers so that the bound's terms come with it: returns (warped * mask, mass [N, 1, H, W], S = sum w |v|,
    V = sum |v| over the in-frame neighbours, Mx, My = W + 2 + 2 |fx| W / (W - 1) and likewise for y: the largest
    magnitude, in pixels, of any intermediate of the sample position)."""
    N, C, H, W = inp.shape
    f64 = torch.float64
    xs, ys = torch.arange(W, dtype=f64).view(1, 1, W), torch.arange(H, dtype=f64).view(1, H, 1)
    gx = (-1.0 + (2.0 * xs + 1.0) / W) + flow[:, 0] / ((W - 1.0) / 2.0)
    gy = (-1.0 + (2.0 * ys + 1.0) / H) + flow[:, 1] / ((H - 1.0) / 2.0)
    ix, iy = ((gx + 1.0) * W - 1.0) / 2.0, ((gy + 1.0) * H - 1.0) / 2.0
    x0, y0 = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - x0, iy - y0
    flat = inp.reshape(N, C, H * W)
    out, S, V = torch.zeros_like(inp), torch.zeros_like(inp), torch.zeros_like(inp)
    mass = torch.zeros(N, H, W, dtype=f64)
    for dy, dx, wgt in [(0, 0, (1 - wy1) * (1 - wx1)), (0, 1, (1 - wy1) * wx1), (1, 0, wy1 * (1 - wx1)),
                        (1, 1, wy1 * wx1)]:
        xx, yy = x0 + dx, y0 + dy
        valid = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)).double()
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).long().view(N, 1, H * W).expand(N, C, H * W)
        v = flat.gather(2, idx).view(N, C, H, W) * valid.unsqueeze(1)
        wv = (wgt * valid).unsqueeze(1)
        out, S, V, mass = out + wv * v, S + wv * v.abs(), V + v.abs(), mass + wgt * valid
    m = (mass > 0.999).double().unsqueeze(1)
    Mx = (W + 2.0 + 2.0 * flow[:, 0].abs() * W / (W - 1.0)).unsqueeze(1)
    My = (H + 2.0 + 2.0 * flow[:, 1].abs() * H / (H - 1.0)).unsqueeze(1)
    return out * m, mass.unsqueeze(1), S * m, V * m, Mx, My


def mask_ambiguous(mass):
    """Pixels whose float64 weight mass is within 1e-4 of the mask threshold 0.999 (the kernels compute the sample
    position in fp32; the threshold is the only discontinuity)."""
    return (mass - 0.999).abs() <= 1e-4
