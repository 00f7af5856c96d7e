"""Op-level tests of the training backward: every op of the plan against plain torch on the CPU (fp32 / fp64 on
the same dtype-rounded operands), never against another kernel of this library.

  * direct tests of the ops that had none (unshuffle_gate, merge_prep_backward, gate_copy, enc_grad_gate,
    relu_grad, dgrad_weights, adam_step) -- bitwise wherever the op is a select, a copy or one rounding;
  * scaled-gradient magnitudes: the fp16 trainer's gradients are 65536 x the true ones and sit in and below fp16's
    subnormal range (< 2^-14), as MFMA operands (wgrad, dgrad) and as conversion results;
  * an overflow cannot be hidden: a 16-bit store of a finite fp32 value beyond 65504 is +-inf (never 65504, never
    NaN), and an inf / NaN in the upstream gradient reaches exactly the outputs it reaches in torch -- closed
    ReLU gates stay exactly 0 (a select, not a multiply), nothing else turns non-finite.  This is what
    dbsr_grad_unscale_check's found_inf relies on ('fp16 training').

Planted infs sit on interior pixels: at a border a zero-padded tap times inf is NaN or nothing depending on how an
implementation pads, in torch as much as here."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = 'cuda'
DT = [torch.float32, torch.bfloat16, torch.float16]
D16 = [torch.bfloat16, torch.float16]
F16_MAX = 65504.0
# the half-ulp of one round-to-nearest store, relative
RND = {torch.float32: 0.0, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
# dgrad cases (N, Cout, H, W, Cin, k, kernel id as dbsr_conv_kernel_for reports it), one per gated epilogue.
# FAST: the gated fast conv kernels of the training step, one per kernel id (tests/test_gpu_train.py GATED:
# weight-stationary, pipelined, K-split 128).  SLOW: the kernels every other shape falls to (the shapes of
# test_conv_dgrad_gate_residual and two more) -- LDS-tiled with the per-element epilogue (4 output channels), LDS-tiled
# with the staged 16-byte epilogue (40 channels, ragged 9x11), generic MFMA (8 input channels), generic 1x1 with
# 512 output channels, and the LDS-tiled kernel's split-K over 512 input channels (fp32 partials, gated in the
# finalize pass)
FAST = [(40, 64, 32, 16, 96, 3, 4), (48, 128, 48, 48, 64, 3, 2), (64, 128, 32, 32, 128, 3, 7)]
SLOW = [(2, 64, 12, 16, 4, 3, 1), (2, 64, 9, 11, 40, 3, 1), (2, 8, 9, 11, 24, 3, 0), (2, 64, 8, 16, 512, 1, 0),
        (2, 512, 12, 12, 64, 3, 1)]


@pytest.fixture(scope='module')
def ops():
    from dbsr_amd import ops as O
    return O


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.element_size() == 4 else torch.int16)


def _assert_bitwise(out, ref):
    assert out.dtype == ref.dtype and out.shape == ref.shape, (out.dtype, ref.dtype, out.shape, ref.shape)
    a, b = _bits(out), _bits(ref)
    assert torch.equal(a, b), '%d of %d elements differ' % (int((a != b).sum()), a.numel())


def _nan_buf(*shape, dtype):
    """A device buffer of NaNs: padding that an op must neither read (the result would be NaN) nor write."""
    return torch.full(shape, float('nan'), dtype=dtype, device=DEV)


def _assert_padding_untouched(buf, lo, hi=None):
    pad = buf[..., lo:hi]
    assert pad.numel() > 0
    _assert_bitwise(pad, _nan_buf(*pad.shape, dtype=buf.dtype))


def _signed(shape, gen, dtype, zero_frac=0.1):
    """A gate source: normal values of both signs with exact zeros (and a -0), rounded to dtype."""
    t = torch.randn(shape, generator=gen)
    t = torch.where(torch.rand(shape, generator=gen) < zero_frac, torch.zeros(()), t)
    t.view(-1)[0] = -0.0
    return t.to(dtype)


def _where(gate, val):
    return torch.where(gate > 0, val, torch.zeros((), dtype=val.dtype))


def _nonfinite_equal(out, ref):
    """The set of non-finite elements of `out` equals the reference's, and is not empty."""
    bo, br = ~torch.isfinite(out), ~torch.isfinite(ref)
    assert bool(br.any())
    assert torch.equal(bo, br), ('non-finite in out only: %d, in ref only: %d of %d'
                                 % (int((bo & ~br).sum()), int((br & ~bo).sum()), int(br.sum())))


def _assert_overflow_is_inf(out, ref):
    """Store overflow: wherever the finite fp32 reference exceeds fp16's range the stored value is inf with the
    reference's sign -- not 65504, not NaN; nothing is NaN anywhere."""
    assert bool(torch.isfinite(ref).all())
    big = ref.abs() > F16_MAX
    assert bool(big.any())
    expect = torch.where(ref > 0, torch.tensor(float('inf')), torch.tensor(float('-inf')))
    assert torch.equal(out[big], expect[big]), out[big][out[big] != expect[big]][:8]
    assert not bool(torch.isnan(out).any())
    return big


# ----------------------------------------------------------------------------------------------------
# 3. direct tests of the ops that had none
# ----------------------------------------------------------------------------------------------------
def _ref_unshuffle_gate(S, dS, s):
    return F.pixel_unshuffle(_where(S, dS), s)


# (B, H, W, s, c, du padding): 5x7 ragged; 8*8*4 = 256 tasks = exactly one pass of the 16-B kernel's 256 threads;
# 320 tasks = a second pass; c % 8 != 0 = the element kernel also in 16-bit; 65792 pixels > the 16-B kernel's
# 65536 blocks = its grid-stride loop
@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('case', [(2, 5, 7, 2, 32, 0), (1, 3, 4, 8, 32, 0), (1, 2, 3, 8, 40, 24), (2, 4, 5, 4, 3, 5),
                                  (1, 257, 256, 2, 8, 0)])
def test_unshuffle_gate(ops, dtype, case):
    """PixelShuffle + ReLU backward is a gather and a select: bitwise F.pixel_unshuffle(where(S > 0, dS, 0)) in
    torch's channel order; padding channels of du (ld > c s s, NaN) are neither read nor written."""
    B, H, W, s, c, pad = case
    gen = _gen(c * 11 + s + W)
    dS = torch.randn(B, c, H * s, W * s, generator=gen).to(dtype)
    S = _signed((B, c, H * s, W * s), gen, dtype)
    ref = _ref_unshuffle_gate(S, dS, s).permute(0, 2, 3, 1)
    K = c * s * s
    ld_in = (c + 7) // 8 * 8
    ds, gs = (torch.zeros(B, H * s, W * s, ld_in, dtype=dtype, device=DEV) for _ in range(2))
    ds[..., :c], gs[..., :c] = dS.permute(0, 2, 3, 1).to(DEV), S.permute(0, 2, 3, 1).to(DEV)
    du = _nan_buf(B, H, W, K + pad, dtype=dtype)
    ops.unshuffle_gate(ds, gs, du, s, c)
    _assert_bitwise(du[..., :K], ref)
    if pad:
        _assert_padding_untouched(du, K)


def _ref_merge_prep_backward(pre, dwp, c):
    """Autograd through merging.py:79-89's weight-predictor input on proj = relu(pre): pre [B,N,hw,c], dwp
    [B,N,hw,2c], in fp64."""
    p = pre.double().requires_grad_()
    proj = F.relu(p)
    torch.cat([proj[:, :1].expand_as(proj), proj - proj[:, :1]], 3).backward(dwp.double())
    return p.grad


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('case', [(2, 1, 35, 64), (2, 5, 42, 64), (1, 14, 9, 8)])
def test_merge_prep_backward(ops, dtype, case):
    """dproj against autograd.  Frames n >= 1 are a gated copy of d diff (bitwise); frame 0 sums 2N - 1 terms in
    fp32: 1e-6 of the sum of their magnitudes, plus the one rounding of a 16-bit store.  dwp's channels
    [2c, ld) hold NaN and must not be read; dproj's padding must not be written."""
    B, N, hw, c = case
    gen = _gen(N * 5 + c)
    pre = _signed((B, N, hw, c), gen, dtype)
    dwp = torch.randn(B, N, hw, 2 * c, generator=gen).to(dtype)
    ref = _ref_merge_prep_backward(pre.float(), dwp.float(), c)
    d_dwp = _nan_buf(B * N, hw, 2 * c + 64, dtype=dtype)
    d_dwp[..., :2 * c] = dwp.reshape(B * N, hw, 2 * c).to(DEV)
    proj = F.relu(pre.float()).to(dtype).reshape(B * N, hw, c).to(DEV).contiguous()
    dproj = _nan_buf(B * N, hw, c + 8, dtype=dtype)
    ops.merge_prep_backward(d_dwp, proj, dproj, N, c)
    _assert_padding_untouched(dproj, c)
    out = dproj[..., :c].cpu().reshape(B, N, hw, c)
    if N > 1:
        _assert_bitwise(out[:, 1:], _where(pre[:, 1:], dwp[:, 1:, :, c:]))
    terms = dwp[..., :c].double().abs().sum(1) + dwp[:, 1:, :, c:].double().abs().sum(1)
    err = (out[:, 0].double() - ref[:, 0]).abs()
    assert bool((err <= 1e-6 * terms + RND[dtype] * ref[:, 0].abs()).all()), float(err.max())
    assert bool((out[:, 0][pre[:, 0] <= 0] == 0).all())


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('case', [(3, 35, 64), (1, 1, 8), (2, 300, 512)])
def test_gate_copy(ops, dtype, case):
    """out = where(gate > 0, in, 0), bitwise, into the channel slice [8, 8 + c) of a wider buffer whose other
    channels (NaN) stay as they are; the gate is every third image of its tensor, the frame map (1, 3, 0, 1) the
    plan uses for the reference frame of each burst."""
    n, hw, c = case
    NF = 3
    gen = _gen(hw + c)
    x = torch.randn(n, hw, c, generator=gen).to(dtype)
    gate = _signed((n, NF, hw, c), gen, dtype)
    gate[:, 1:] = -gate[:, :1] + 0.5              # the other frames would give another result
    out = _nan_buf(n, hw, 8 + c + 16, dtype=dtype)
    ops.gate_copy(x.to(DEV), gate.reshape(n * NF, hw, c).to(DEV), out, c, out_c0=8, gate_map=(1, NF, 0, 1))
    _assert_bitwise(out[..., 8:8 + c], _where(gate[:, 0], x))
    _assert_padding_untouched(out, 0, 8)
    _assert_padding_untouched(out, 8 + c)


def _ref_enc_grad_gate(e, dref, dsrc32, dtype):
    """e [B,N,hw,c], dref [B,hw,c] (dtype), dsrc32 [B,N,hw,c] fp32."""
    ref = _where(e, dsrc32).to(dtype)
    ref[:, 0] = _where(e[:, 0], dref)
    return ref


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('case', [(2, 3, 35, 64), (1, 1, 9, 8)])
def test_enc_grad_gate(ops, dtype, case):
    """Frame 0 bitwise where(e > 0, dref, 0); frames n >= 1 bitwise where(e > 0, dsrc32, 0) rounded to the dtype
    (dsrc32's frame 0 is NaN: it is not read)."""
    B, N, hw, c = case
    gen = _gen(hw + c + N)
    e = _signed((B, N, hw, c), gen, dtype)
    dref = torch.randn(B, hw, c, generator=gen).to(dtype)
    dsrc = torch.randn(B, N, hw, c, generator=gen)
    dsrc[:, 0] = float('nan')
    de = _nan_buf(B * N, hw, c + 8, dtype=dtype)
    ops.enc_grad_gate(dref.to(DEV), dsrc.reshape(B * N, hw, c).to(DEV), e.reshape(B * N, hw, c).to(DEV), de, N, c)
    _assert_bitwise(de[..., :c].cpu().reshape(B, N, hw, c), _ref_enc_grad_gate(e, dref, dsrc, dtype))
    _assert_padding_untouched(de, c)


@pytest.mark.parametrize('dtype', DT)
@pytest.mark.parametrize('case', [(2, 3, 40, 56), (1, 1, 7, 37)])
def test_relu_grad(ops, dtype, case):
    """dpre = where(pred > 0, gout, 0) as NHWC in the dtype (one rounding), bitwise; channels C..7 untouched."""
    B, C, H, W = case
    gen = _gen(H + W)
    pred = _signed((B, C, H, W), gen, torch.float32, zero_frac=0.2)
    gout = torch.randn(B, C, H, W, generator=gen)
    dpre = _nan_buf(B, H, W, 8, dtype=dtype)
    ops.relu_grad(pred.to(DEV), gout.to(DEV), dpre)
    _assert_bitwise(dpre[..., :C], _where(pred, gout).permute(0, 2, 3, 1).to(dtype))
    _assert_padding_untouched(dpre, C)


# (cout, cin, kh, kw); only square kernels are passed by the trainer, the export takes kh and kw apart
@pytest.mark.parametrize('case', [(64, 4, 3, 3), (3, 32, 1, 1), (128, 96, 3, 3), (5, 7, 2, 5)])
def test_dgrad_weights(ops, case):
    cout, cin, kh, kw = case
    w = torch.randn(cout, cin, kh, kw, generator=_gen(cout + cin))
    _assert_bitwise(ops.dgrad_weights(w.to(DEV)), w.flip(2, 3).transpose(0, 1).contiguous())


# the C ABI takes lr, the betas and eps as fp32
_B32 = tuple(float(torch.tensor(b, dtype=torch.float32)) for b in (0.9, 0.999))


@pytest.mark.parametrize('grad_scale', [1.0, 0.5])
@pytest.mark.parametrize('gstd,betas', [(0.1, (0.9, 0.999)), (1.0, _B32)])
def test_adam_step(ops, gstd, betas, grad_scale):
    """Three successive dbsr_adam_step calls (step = 1, 2, 3; fresh gradients) against torch.optim.Adam(lr=1e-4)
    fed grad_scale * g: p, exp_avg and exp_avg_sq at the tolerance of test_guarded_adam_and_update_sequence; the 8
    elements after n of the over-allocated buffers are untouched.

    Two references.  torch's defaults, with that test's gradients (0.1 N(0, 1)).  And N(0, 1) gradients, where
    exp_avg_sq is far above atol and the relative term decides, against torch given the betas the kernel is given:
    the export takes them as fp32, so it runs Adam at beta2 = fp32(0.999) = 0.999000013, whose 1 - beta2 is
    1.3e-5 below 0.001 -- exp_avg_sq sits 1.3e-5 (relative) below torch's at the decimal beta2, bias correction
    cancels it to first order, and p agrees to an fp32 ulp."""
    import numpy as np
    n, extra = 4099, 8
    gen = _gen(7)
    p0 = torch.randn(n + extra, generator=gen)
    bufs = [p0.clone().to(DEV), None, torch.zeros(n + extra, device=DEV), torch.zeros(n + extra, device=DEV)]
    for i in (2, 3):
        bufs[i][n:] = float(i)                           # sentinels after n
    pr = p0[:n].clone().requires_grad_()
    opt = torch.optim.Adam([pr], lr=1e-4, betas=betas)
    for step in (1, 2, 3):
        g = torch.randn(n + extra, generator=gen) * gstd
        bufs[1] = g.to(DEV)
        ops.adam_step(bufs[0], bufs[1], bufs[2], bufs[3], step, lr=1e-4, grad_scale=grad_scale, n=n)
        pr.grad = (grad_scale * g[:n]).clone()
        opt.step()
        st = opt.state[pr]
        for got, want in ((bufs[0], pr.detach()), (bufs[2], st['exp_avg']), (bufs[3], st['exp_avg_sq'])):
            np.testing.assert_allclose(got[:n].cpu().numpy(), want.numpy(), rtol=1e-6, atol=1e-7)
    _assert_bitwise(bufs[0][n:], p0[n:])
    for i in (2, 3):
        _assert_bitwise(bufs[i][n:], torch.full((extra,), float(i)))


# ----------------------------------------------------------------------------------------------------
# 2. scaled-gradient magnitudes: subnormal fp16 operands and results
# ----------------------------------------------------------------------------------------------------
SUB = 2.0 ** -14                        # below: fp16 subnormal (spacing 2^-24)


def _scaled_grad(shape, gen):
    """An upstream gradient at the fp16 trainer's magnitude: randn 2^-15 rounded to fp16 -- at least half of its
    nonzero entries subnormal, fewer than 5 % rounded to zero (asserted here, on the CPU)."""
    dy = (torch.randn(shape, generator=gen) * 2.0 ** -15).half()
    nz = dy != 0
    assert int(((dy.float().abs() < SUB) & nz).sum()) * 2 >= int(nz.sum())
    assert float((~nz).float().mean()) < 0.05
    return dy.float()


def _rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))


def _assert_subnormal_result(out, ref, sums_to_normal=False):
    """A subnormal fp16 result against the fp64 reference: 1e-4 of the largest magnitude (fp32 summation order)
    plus one subnormal spacing 2^-24, which covers two half-spacing roundings.  That spacing is fp16's up to
    2^-13 and the half-spacing stays within it up to 2^-12, so the references are asserted to stay below 2^-12.
    sums_to_normal: an op whose sums of such gradients leave that range (merge-prep's frame 0 adds 2N - 1 of them)
    gets round-to-nearest's own half ulp, 2^-11 |ref|, where that exceeds 2^-24 -- above 2^-13 only."""
    err = (out.double() - ref).abs()
    print('max err %.3g, max|ref| %.3g (2^-24 = %.3g)' % (float(err.max()), float(ref.abs().max()), 2.0 ** -24))
    assert bool((ref.abs() < SUB).float().mean() > 0.5)           # the results are themselves subnormal
    spacing = torch.full_like(ref, 2.0 ** -24)
    if sums_to_normal:
        spacing = torch.maximum(spacing, 2.0 ** -11 * ref.abs())
    else:
        assert float(ref.abs().max()) < 2.0 ** -12
    assert bool((err <= 1e-4 * float(ref.abs().max()) + spacing).all()), float(err.max())


@pytest.mark.parametrize('case', [(2, 64, 20, 36, 64, 3), (3, 32, 20, 36, 32, 3), (2, 512, 8, 16, 64, 1)])
def test_wgrad_subnormal_dy(ops, case):
    """fp16 wgrad (mfma_f32_16x16x32_f16) with dY in fp16's subnormal range, activations at the usual magnitude:
    dW (both algos) and db against fp64 on the rounded values.  A kernel or an MFMA that flushes subnormal operands
    loses over half of dY here."""
    from dbsr_amd import _lib as L
    N, Cin, H, W, Cout, k = case
    gen = _gen(Cin + Cout + k)
    x = torch.randn(N, Cin, H, W, generator=gen).half().float()
    dy = _scaled_grad((N, Cout, H, W), gen)
    w = torch.zeros(Cout, Cin, k, k, dtype=torch.float64, requires_grad=True)
    F.conv2d(x.double(), w, padding=k // 2).backward(dy.double())
    asum = float(dy.double().abs().sum((0, 2, 3)).max())
    dw, db = ops.conv2d_wgrad(x.to(DEV), dy.to(DEV), k, compute_dtype=torch.float16, with_bias=True)
    L.lib().dbsr_set_wgrad_algo(0)
    try:
        dw0, db0 = ops.conv2d_wgrad(x.to(DEV), dy.to(DEV), k, compute_dtype=torch.float16, with_bias=True)
    finally:
        L.lib().dbsr_set_wgrad_algo(1)
    for a, b in ((dw, db), (dw0, db0)):
        print('dW rel %.3g' % _rel(a.cpu().double(), w.grad))
        assert _rel(a.cpu().double(), w.grad) <= 1e-4
        assert float((b.cpu().double() - dy.double().sum((0, 2, 3))).abs().max()) <= 1e-5 * asum


def _dgrad_ref64(dy, w, res, gate):
    x = torch.zeros(dy.shape[0], w.shape[1], *dy.shape[2:], dtype=torch.float64, requires_grad=True)
    F.conv2d(x, w.double(), padding=w.shape[2] // 2).backward(dy.double())
    g = x.grad if res is None else x.grad + res.double()
    return _where(gate, g)


@pytest.mark.parametrize('use_res', [False, True])
@pytest.mark.parametrize('case', [(1, 64, 12, 16, 4, 3, 1), FAST[0]])
def test_dgrad_subnormal(ops, case, use_res):
    """fp16 dgrad (gated, with and without a residual at the same scale) with dY in the subnormal range: the
    MFMA's A operand, and results that are subnormal fp16 themselves (the store's conversion)."""
    N, Cout, H, W, Cin, _, kern = case
    gen = _gen(Cin + Cout + W)
    dy = _scaled_grad((N, Cout, H, W), gen)
    w = (torch.randn(Cout, Cin, 3, 3, generator=gen) / (Cout * 9) ** 0.5).half().float()
    res = _scaled_grad((N, Cin, H, W), gen) if use_res else None
    gate = _signed((N, Cin, H, W), gen, torch.float16).float()
    ref = _dgrad_ref64(dy, w, res, gate)
    out = ops.conv2d_dgrad(dy.to(DEV), w.to(DEV), residual=res.to(DEV) if use_res else None, gate=gate.to(DEV),
                           compute_dtype=torch.float16).cpu()
    assert ops.conv2d_dgrad.last_kernel == kern, ops.conv2d_dgrad.last_kernel
    _assert_subnormal_result(out, ref)
    assert bool((out[gate <= 0] == 0).all())


def _fuse_inputs(B, N, C, H, W, gen, dtype):
    w = F.softmax(torch.randn(B, N, C, H, W, generator=gen), dim=1).to(dtype)
    f = torch.randn(B, N, C, H, W, generator=gen).to(dtype)
    fused = (w.double() * f.double()).sum(1).to(dtype)
    return w, f, fused


def _ref_fuse_backward(w, f, fused, dfu):
    """merging.py:116-124's backward in closed form, fp64: dF_n = w_n dfused, dl_n = w_n dfused (f_n - fused)
    (tests/test_gpu_train.py checks this form against autograd)."""
    df = w.double() * dfu.double()[:, None]
    return df * (f.double() - fused.double()[:, None]), df


def test_fuse_backward_subnormal(ops):
    B, N, C, H, W = 2, 8, 8, 5, 7
    gen = _gen(21)
    w, f, fused = _fuse_inputs(B, N, C, H, W, gen, torch.float16)
    dfu = _scaled_grad((B, C, H, W), gen).half()
    rdl, rdf = _ref_fuse_backward(w, f, fused, dfu)
    dl, df = ops.fuse_backward(w.to(DEV), f.to(DEV), fused.to(DEV), dfu.to(DEV))
    _assert_subnormal_result(df.cpu(), rdf)
    _assert_subnormal_result(dl.cpu(), rdl)


def test_merge_prep_backward_subnormal(ops):
    B, N, hw, c = 2, 5, 42, 64
    gen = _gen(22)
    pre = _signed((B, N, hw, c), gen, torch.float16)
    dwp = _scaled_grad((B, N, hw, 2 * c), gen).half()
    ref = _ref_merge_prep_backward(pre.float(), dwp.float(), c)
    dproj = torch.empty(B * N, hw, c, dtype=torch.float16, device=DEV)
    ops.merge_prep_backward(dwp.reshape(B * N, hw, 2 * c).to(DEV),
                            F.relu(pre.float()).half().reshape(B * N, hw, c).to(DEV), dproj, N, c)
    _assert_subnormal_result(dproj.cpu().reshape(B, N, hw, c), ref, sums_to_normal=True)


def _head_inputs(n, hw, hc, gen, dtype):
    h = _signed((n, hw, 32), gen, dtype)
    w = (torch.randn(hc, 32, generator=gen) * 0.2)
    return h, w


def _ref_head_dh(h, w, dp):
    """dh = where(h > 0, w^T dp, 0): h [n,hw,32], w [hc,32], dp [n,hw,hc]."""
    return _where(h, dp.to(w.dtype) @ w)


def _run_head_backward(ops, h, w, dp, dtype):
    n, hw, hc = dp.shape
    dps = torch.zeros(n, hw, 8, dtype=dtype, device=DEV)
    dps[..., :hc] = dp.to(DEV).to(dtype)
    dh = torch.empty(n, hw, 32, dtype=dtype, device=DEV)
    dh, dw, db = ops.head_backward(h.to(DEV).to(dtype), dps, w.to(DEV), hc, dh)
    return dh.cpu(), dw.cpu(), db.cpu()


def test_head_backward_subnormal(ops):
    n, hw, hc = 2, 33 * 47, 3
    gen = _gen(23)
    h, w = _head_inputs(n, hw, hc, gen, torch.float16)
    dp = _scaled_grad((n, hw, hc), gen)
    dh, _, _ = _run_head_backward(ops, h, w, dp, torch.float16)
    _assert_subnormal_result(dh, _ref_head_dh(h, w.double(), dp))


# ----------------------------------------------------------------------------------------------------
# 4. an overflow cannot be hidden
# ----------------------------------------------------------------------------------------------------
def _ones_dgrad_ref(N, Cout, H, W, Cin, k, sign):
    """dX of an all-ones k x k conv for dY = +-60000 per frame: 60000 Cout (in-frame taps), fp32."""
    taps = F.conv2d(torch.ones(1, 1, H, W), torch.ones(1, 1, k, k), padding=k // 2)
    return (taps * (60000.0 * Cout)).expand(N, Cin, H, W) * sign.view(N, 1, 1, 1)


@pytest.mark.parametrize('case', SLOW + FAST)
def test_dgrad_store_overflow(ops, case):
    """dY = +-60000 (by frame) through an all-ones conv: every dX with an open gate is a finite fp32 sum
    beyond 65504 and is stored as inf of that sign; closed gates are exactly 0."""
    N, Cout, H, W, Cin, k, kern = case
    gen = _gen(Cin + Cout)
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    dy = (60000.0 * sign).view(N, 1, 1, 1).expand(N, Cout, H, W).contiguous()
    gate = _signed((N, Cin, H, W), gen, torch.float16).float()
    ref = _where(gate, _ones_dgrad_ref(N, Cout, H, W, Cin, k, sign))
    out = ops.conv2d_dgrad(dy.to(DEV), torch.ones(Cout, Cin, k, k, device=DEV), gate=gate.to(DEV),
                           compute_dtype=torch.float16).float().cpu()
    assert ops.conv2d_dgrad.last_kernel == kern, ops.conv2d_dgrad.last_kernel
    big = _assert_overflow_is_inf(out, ref)
    assert torch.equal(big, gate > 0)
    assert bool((out[gate <= 0] == 0).all())


def _dgrad_ref32(dy, w, res, gate):
    x = torch.zeros(dy.shape[0], w.shape[1], *dy.shape[2:], requires_grad=True)
    F.conv2d(x, w, padding=w.shape[2] // 2).backward(dy)
    return _where(gate, x.grad if res is None else x.grad + res)


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('case', [c + (dt,) for c in SLOW for dt in D16] + [c + (torch.float16,) for c in FAST])
def test_dgrad_propagation(ops, case, bad):
    """One inf (or NaN) in dY, at an interior pixel of the last frame, with a residual: dX is non-finite exactly on
    the open gates of that pixel's k x k footprint (all Cin), as in torch; the footprint's closed gates -- the centre
    pixel's are closed for every second channel -- and everything else are finite, closed ones exactly 0."""
    N, Cout, H, W, Cin, k, kern, dtype = case
    gen = _gen(Cin * 3 + Cout)
    dy = torch.randn(N, Cout, H, W, generator=gen).to(dtype).float()
    w = (torch.randn(Cout, Cin, k, k, generator=gen) / (Cout * k * k) ** 0.5).to(dtype).float()
    res = torch.randn(N, Cin, H, W, generator=gen).to(dtype).float()
    gate = _signed((N, Cin, H, W), gen, dtype).float()
    y0, x0 = H // 2, W // 2 + 1
    gate[N - 1, 0::2, y0, x0], gate[N - 1, 1::2, y0, x0] = 1.0, -1.0
    dy[N - 1, Cout // 3, y0, x0] = bad
    ref = _dgrad_ref32(dy, w, res, gate)
    out = ops.conv2d_dgrad(dy.to(DEV), w.to(DEV), residual=res.to(DEV), gate=gate.to(DEV),
                           compute_dtype=dtype).float().cpu()
    assert ops.conv2d_dgrad.last_kernel == kern, ops.conv2d_dgrad.last_kernel
    foot = torch.zeros_like(gate, dtype=torch.bool)
    foot[N - 1, :, y0 - k // 2:y0 + k // 2 + 1, x0 - k // 2:x0 + k // 2 + 1] = True
    assert torch.equal(~torch.isfinite(ref), foot & (gate > 0))           # the reference's own footprint
    assert float(ref[torch.isfinite(ref)].abs().max()) < 6e4
    _nonfinite_equal(out, ref)
    assert bool((out[gate <= 0] == 0).all())


def test_head_backward_store_overflow(ops):
    n, hw, hc = 2, 99, 3
    gen = _gen(31)
    h, _ = _head_inputs(n, hw, hc, gen, torch.float16)
    w = torch.ones(hc, 32)
    dp = torch.full((n, hw, hc), 60000.0)
    dp[1] = -60000.0
    ref = _ref_head_dh(h, w, dp)                         # +-180000 on the open gates
    dh, _, _ = _run_head_backward(ops, h, w, dp, torch.float16)
    big = _assert_overflow_is_inf(dh.float(), ref)
    assert torch.equal(big, h > 0) and bool((dh[h <= 0] == 0).all())


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('dtype', D16)
def test_head_backward_propagation(ops, dtype, bad):
    """A non-finite dP element at (pixel, channel 1): dh non-finite on that pixel's open gates only (closed: 0),
    dW's row 1 and db[1] non-finite and no other -- as the fp32 reference."""
    n, hw, hc = 2, 33 * 47, 3
    gen = _gen(32)
    h, w = _head_inputs(n, hw, hc, gen, dtype)
    dp = torch.randn(n, hw, hc, generator=gen).to(dtype).float()
    h[1, 777, 0::2], h[1, 777, 1::2] = 1.0, -1.0
    dp[1, 777, 1] = bad
    dh, dw, db = _run_head_backward(ops, h, w, dp, dtype)
    _nonfinite_equal(dh.float(), _ref_head_dh(h, w, dp))
    assert bool((dh[h <= 0] == 0).all())
    hf = h.float().reshape(-1, 32)
    _nonfinite_equal(dw, dp.reshape(-1, hc).t() @ hf)
    _nonfinite_equal(db, dp.reshape(-1, hc).sum(0))


def test_fuse_backward_store_overflow(ops):
    """w = 1, dfused = +-60000, f - fused = 2: dF = +-60000 is stored exactly, dl = +-120000 as +-inf."""
    B, N, C, H, W = 2, 3, 8, 5, 7
    w = torch.ones(B, N, C, H, W, dtype=torch.float16)
    f = torch.full((B, N, C, H, W), 3.0, dtype=torch.float16)
    fused = torch.ones(B, C, H, W, dtype=torch.float16)
    dfu = torch.full((B, C, H, W), 60000.0, dtype=torch.float16)
    dfu[1] = -60000.0
    rdl, rdf = _ref_fuse_backward(w, f, fused, dfu)
    dl, df = ops.fuse_backward(w.to(DEV), f.to(DEV), fused.to(DEV), dfu.to(DEV))
    big = _assert_overflow_is_inf(dl.float().cpu(), rdl.float())
    assert bool(big.all())
    assert torch.equal(df.float().cpu(), rdf.float())


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('dtype', D16)
def test_fuse_backward_propagation(ops, dtype, bad):
    """A non-finite dfused element makes dF and dl non-finite at its (b, channel, pixel) in every frame -- the
    second chunk's frames included -- and nowhere else (reference: autograd through the fp32 softmax fusion)."""
    B, N, C, H, W = 2, 8, 8, 5, 7
    gen = _gen(33)
    lg = torch.randn(B, N, C, H, W, generator=gen).requires_grad_()
    f = torch.randn(B, N, C, H, W, generator=gen).to(dtype).float().requires_grad_()
    dfu = torch.randn(B, C, H, W, generator=gen).to(dtype).float()
    dfu[1, 5, 2, 3] = bad
    w = F.softmax(lg, dim=1)
    fused = (w * f).sum(1)
    fused.backward(dfu)
    dl, df = ops.fuse_backward(w.detach().to(dtype).to(DEV), f.detach().to(dtype).to(DEV),
                               fused.detach().to(dtype).to(DEV), dfu.to(dtype).to(DEV))
    spot = torch.zeros(B, N, C, H, W, dtype=torch.bool)
    spot[1, :, 5, 2, 3] = True
    assert torch.equal(~torch.isfinite(f.grad), spot) and torch.equal(~torch.isfinite(lg.grad), spot)
    _nonfinite_equal(df.float().cpu(), f.grad)
    _nonfinite_equal(dl.float().cpu(), lg.grad)


def _run_merge_prep(ops, pre, dwp, N, c, dtype):
    B, hw = pre.shape[0], pre.shape[2]
    dproj = torch.empty(B * N, hw, c, dtype=dtype, device=DEV)
    ops.merge_prep_backward(dwp.to(dtype).reshape(B * N, hw, 2 * c).to(DEV),
                            F.relu(pre.float()).to(dtype).reshape(B * N, hw, c).to(DEV), dproj, N, c)
    return dproj.float().cpu().reshape(B, N, hw, c)


def test_merge_prep_backward_store_overflow(ops):
    """Five frames of d base = +-60000 sum to +-300000 in frame 0: inf on its open gates; frames n >= 1 keep
    their finite d diff."""
    B, N, hw, c = 2, 5, 35, 8
    gen = _gen(34)
    pre = _signed((B, N, hw, c), gen, torch.float16)
    dwp = torch.zeros(B, N, hw, 2 * c)
    dwp[0, ..., :c], dwp[1, ..., :c] = 60000.0, -60000.0
    dwp[..., c:] = torch.randn(B, N, hw, c, generator=gen).half().float()
    ref = _ref_merge_prep_backward(pre.float(), dwp, c).float()
    out = _run_merge_prep(ops, pre, dwp, N, c, torch.float16)
    big = _assert_overflow_is_inf(out, ref)
    gate0 = torch.zeros_like(big)
    gate0[:, 0] = pre[:, 0] > 0
    assert torch.equal(big, gate0)
    assert torch.equal(out[:, 1:], ref[:, 1:])


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('dtype', D16)
def test_merge_prep_backward_propagation(ops, dtype, bad):
    """Non-finite d base (frame 2) and d diff (frame 3) elements, each once under an open and once under a closed
    projection gate: autograd's set of non-finite dproj elements (frame 0 through the sum, frame 3 itself)."""
    B, N, hw, c = 2, 5, 35, 8
    gen = _gen(35)
    pre = _signed((B, N, hw, c), gen, dtype)
    dwp = torch.randn(B, N, hw, 2 * c, generator=gen).to(dtype).float()
    # (b, pixel, channel): open at frame 0 and frame 3 / closed at both
    pre[0, 0, 4, 1], pre[0, 3, 4, 1], pre[1, 0, 9, 6], pre[1, 3, 9, 6] = 1.0, 1.0, -1.0, -1.0
    pre[0, 0, 20, 2], pre[1, 0, 21, 3] = 1.0, -1.0
    dwp[0, 3, 4, c + 1] = dwp[1, 3, 9, c + 6] = bad       # d diff, frame 3
    dwp[0, 2, 20, 2] = dwp[1, 2, 21, 3] = bad             # d base, frame 2
    ref = _ref_merge_prep_backward(pre.float(), dwp, c).float()
    assert int((~torch.isfinite(ref)).sum()) == 3
    out = _run_merge_prep(ops, pre, dwp, N, c, dtype)
    _nonfinite_equal(out, ref)
    assert bool((out[pre <= 0] == 0).all())


def _warp_ref(dy, fl):
    from oracle import dbsr_oracle as orc
    x = torch.zeros_like(dy).requires_grad_()
    orc.warp(x, fl).backward(dy)
    return x.grad


def test_warp_backward_gather_store_overflow(ops):
    """Flows that send each odd column onto its even neighbour: two contributions of 60000 with weight 1 meet in
    one pixel, a finite fp32 sum of 120000 that is stored as inf."""
    N, C, H, W = 2, 8, 6, 10
    fl = torch.zeros(N, 2, H, W)
    fl[:, 0, :, 1::2] = -1.0
    dy = torch.full((N, C, H, W), 60000.0)
    dy[1] = -60000.0
    ref = _warp_ref(dy, fl)
    out = ops.warp_backward_gather(dy.half().to(DEV), fl.to(DEV), None).float().cpu()
    big = _assert_overflow_is_inf(out, ref)
    assert int(big.sum()) == N * C * H * W // 2


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('dtype', D16)
def test_warp_backward_gather_propagation(ops, dtype, bad):
    """Two non-finite dout elements; the gate (the encoder's ReLU) is open on the bilinear footprint of the first
    and closed on that of the second: non-finite exactly on the first footprint (autograd through the oracle's
    grid_sample warp), exact zeros on the second."""
    N, C, H, W = 2, 8, 12, 20
    gen = _gen(36)
    fl = torch.randn(N, 2, H, W, generator=gen) * 0.7
    dy = torch.randn(N, C, H, W, generator=gen).to(dtype).float()
    dy[1, 3, 3, 7] = bad
    dy[1, 3, 9, 12] = bad
    ungated = _warp_ref(dy, fl)
    nf = ~torch.isfinite(ungated)
    top = torch.zeros_like(nf)
    top[:, :, :6] = True
    assert bool((nf & top).any()) and bool((nf & ~top).any()) and int(nf.sum()) <= 8
    gate = _signed((N, C, H, W), gen, dtype).float()
    gate[nf & top], gate[nf & ~top] = 1.0, -1.0
    ref = _where(gate, ungated)
    out = ops.warp_backward_gather(dy.to(dtype).to(DEV), fl.to(DEV), gate.to(dtype).to(DEV)).float().cpu()
    _nonfinite_equal(out, ref)
    assert bool((out[gate <= 0] == 0).all())


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('dtype', D16)
def test_unshuffle_gate_propagation(ops, dtype, bad):
    """(The op stores what it loads: no store overflow to test.)  Non-finite dS under an open gate arrives, under a
    closed gate it is an exact 0 -- both kernels (c = 32: 16-byte, c = 3: element)."""
    for B, H, W, s, c in ((1, 3, 4, 2, 32), (1, 3, 4, 2, 3)):
        gen = _gen(c)
        dS = torch.randn(B, c, H * s, W * s, generator=gen).to(dtype)
        S = _signed((B, c, H * s, W * s), gen, dtype)
        S[0, 1, 2, 3], S[0, 2, 4, 5] = 1.0, -1.0
        dS[0, 1, 2, 3] = dS[0, 2, 4, 5] = bad
        ref = _ref_unshuffle_gate(S, dS, s).permute(0, 2, 3, 1).float()
        ld_in = (c + 7) // 8 * 8
        ds, gs = (torch.zeros(B, H * s, W * s, ld_in, dtype=dtype, device=DEV) for _ in range(2))
        ds[..., :c], gs[..., :c] = dS.permute(0, 2, 3, 1).to(DEV), S.permute(0, 2, 3, 1).to(DEV)
        du = ops.unshuffle_gate(ds, gs, torch.empty(B, H, W, c * s * s, dtype=dtype, device=DEV), s, c).float().cpu()
        assert int((~torch.isfinite(ref)).sum()) == 1
        _nonfinite_equal(du, ref)
        assert bool((du[ref == 0] == 0).all())


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
@pytest.mark.parametrize('dtype', D16)
def test_gate_copy_propagation(ops, dtype, bad):
    """(A copy: no store overflow to test.)"""
    n, hw, c = 2, 35, 64
    gen = _gen(37)
    x = torch.randn(n, hw, c, generator=gen).to(dtype)
    gate = _signed((n, hw, c), gen, dtype)
    gate[1, 5, 9], gate[1, 6, 10] = 1.0, -1.0
    x[1, 5, 9] = x[1, 6, 10] = bad
    out = ops.gate_copy(x.to(DEV), gate.to(DEV), torch.empty(n, hw, c, dtype=dtype, device=DEV), c).float().cpu()
    ref = _where(gate, x).float()
    assert int((~torch.isfinite(ref)).sum()) == 1
    _nonfinite_equal(out, ref)
    assert bool((out[gate <= 0] == 0).all())


def test_enc_grad_gate_and_relu_grad_store_overflow(ops):
    """The two ops that round fp32 gradients to the compute dtype: a finite fp32 1e5 is stored as inf in fp16."""
    B, N, hw, c = 1, 2, 9, 8
    gen = _gen(38)
    e = _signed((B, N, hw, c), gen, torch.float16)
    dsrc = torch.full((B, N, hw, c), 1e5)
    dsrc[..., 1::2] = -1e5
    dref = torch.zeros(B, hw, c, dtype=torch.float16)
    de = torch.empty(B * N, hw, c, dtype=torch.float16, device=DEV)
    ops.enc_grad_gate(dref.to(DEV), dsrc.reshape(B * N, hw, c).to(DEV), e.reshape(B * N, hw, c).to(DEV), de, N, c)
    ref = _where(e.float(), dsrc)
    ref[:, 0] = 0
    big = _assert_overflow_is_inf(de.float().cpu().reshape(B, N, hw, c), ref)
    assert torch.equal(big[:, 1], e[:, 1] > 0)
    pred = _signed((1, 3, 7, 9), gen, torch.float32)
    gout = torch.full((1, 3, 7, 9), 1e5)
    gout[:, 1] = -1e5
    dpre = torch.zeros(1, 7, 9, 8, dtype=torch.float16, device=DEV)
    ops.relu_grad(pred.to(DEV), gout.to(DEV), dpre)
    big = _assert_overflow_is_inf(dpre[..., :3].float().cpu(), _where(pred, gout).permute(0, 2, 3, 1))
    assert torch.equal(big, (pred > 0).permute(0, 2, 3, 1))


@pytest.mark.parametrize('algo', [1, 0])
@pytest.mark.parametrize('case', [(2, 64, 20, 36, 64, 3), (3, 32, 20, 36, 32, 3), (2, 512, 8, 16, 64, 1)])
def test_wgrad_inf_reaches_dw_and_db(ops, case, algo):
    """The ops that reduce to fp32 (what dbsr_grad_unscale_check then sees): one inf in dY at an interior pixel
    makes dW[co] (every cin, every tap) and db[co] non-finite, and no other -- as the fp32 reference; both wgrad
    kernels."""
    from dbsr_amd import _lib as L
    N, Cin, H, W, Cout, k = case
    gen = _gen(Cin + Cout)
    x = torch.randn(N, Cin, H, W, generator=gen).half().float()
    dy = torch.randn(N, Cout, H, W, generator=gen).half().float()
    dy[N - 1, Cout // 2, H // 2, W // 2] = float('inf')
    w = torch.zeros(Cout, Cin, k, k, requires_grad=True)
    F.conv2d(x, w, padding=k // 2).backward(dy)
    row = torch.zeros(Cout, dtype=torch.bool)
    row[Cout // 2] = True
    assert torch.equal(~torch.isfinite(w.grad), row.view(-1, 1, 1, 1).expand_as(w.grad))
    L.lib().dbsr_set_wgrad_algo(algo)
    try:
        dw, db = ops.conv2d_wgrad(x.to(DEV), dy.to(DEV), k, compute_dtype=torch.float16, with_bias=True)
    finally:
        L.lib().dbsr_set_wgrad_algo(1)
    _nonfinite_equal(dw.cpu(), w.grad)
    _nonfinite_equal(db.cpu(), dy.sum((0, 2, 3)))


@pytest.mark.parametrize('dtype', D16)
@pytest.mark.parametrize('case', [(2, 3, 40, 56), (2, 64, 17, 23), (1, 72, 9, 9)])
def test_chan_sum_inf(ops, dtype, case):
    N, C, H, W = case
    t = torch.randn(N, C, H, W, generator=_gen(C)).to(dtype)
    t[N - 1, C // 2, H // 2, 1] = float('inf')
    _nonfinite_equal(ops.chan_sum(t.to(DEV)).cpu(), t.float().sum((0, 2, 3)))
