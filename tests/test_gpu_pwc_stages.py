"""Op-level tests of the fused PWC-Net alignment kernels (csrc/pwc_dense.hip, csrc/pwc_fused.hip): dbsr_pwc_dense,
dbsr_pwc_level_prep and dbsr_pwc_extract, each against plain torch on the CPU in float64 computed from the same
16-bit-rounded operands the kernel reads (tests/pwc_ref.py: the error unit u and the single-rounding bound
0.5 u + A, A = n_r 2^-24 S).

Teacher forcing: wherever a kernel leaves an intermediate in global memory, the stage that consumes it is recomputed
from the kernel's own stored values, so every stage meets the single-rounding bound with no amplification along the
chain.  Where intermediates stay in the LDS the float64 chain rounds at the same points, and the bound is measured:
1.5 x the per-conv / per-op path's error against the same reference, in the same unit, plus 0.5 u; the mean error is
at most 1.25 x that path's mean (a systematic error moves the mean long before the max).  Means are taken over at
least 1024 elements: the standard error of a mean of n per-element errors of spread ~0.3 u is 0.3 u / sqrt(n), and a
25 % change of a ~0.25 u mean is three standard errors of the difference of two such means only from n ~ 500 on, so
smaller groups are pooled with their neighbour.

Slice discipline: output buffers are prefilled with 3.0 (exact in every dtype); what the header says an op does not
write is bitwise 3.0 afterwards, pad channels it writes are exactly +0.  Buffers a kernel reads never hold NaN: pad
channels that meet zero-padded weights hold finite non-zero values instead (the weights must cancel them)."""
import types

import pytest
import torch
import torch.nn.functional as F

from tests.pwc_ref import (D16, SENTINEL, assert_bitwise, assert_pos_zero, assert_sentinel, assert_single_rounding,
                           backwarp64, bits, correlation64, err_units, lrelu, mask_ambiguous, nchw, rnd, unit)

DEV = 'cuda'
BASE_OFF = 448
DENSE_OUT = [128, 128, 96, 64, 32]
DENSE_OFF = [320, 192, 96, 32, 0]
EXT_CH = [3, 16, 32, 64, 96, 128, 196]
PAD_VALUE = 1.5         # finite, non-zero, exact: pad channels that zero-padded weights must cancel


def cpad(c):
    return (c + 7) // 8 * 8 if c <= 16 else (c + 31) // 32 * 32


def _seed(key):
    """A stable seed from a case key (no Python hash randomisation)."""
    s = 0
    for ch in '|'.join(str(k) for k in key):
        s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
    return s


def _env(dtype):
    from dbsr_amd import _lib as L
    from dbsr_amd import engine as E
    stream = L.stream_ptr(DEV)
    return L, E, stream, E._Weights(dtype, torch.device(DEV), stream)


def _conv_mod(w, b, stride=1):
    return types.SimpleNamespace(weight=w.to(DEV), bias=b.to(DEV), stride=(stride,), padding=(1,), dilation=(1,))


def _sentinel_nhwc(E, n, h, w, ld, dtype):
    t = E.NHWC(n, h, w, ld, dtype, DEV)
    t.t.fill_(SENTINEL)
    return t


def _pooled_means(groups_f, groups_u, min_n=1024):
    """Pool per-group error tensors (coarsest first) until each pool has >= min_n elements; returns
    [(n, mean_f, mean_u)]."""
    out, cf, cu = [], [], []
    for ef, eu in zip(groups_f, groups_u):
        cf.append(ef.reshape(-1))
        cu.append(eu.reshape(-1))
        if sum(t.numel() for t in cf) >= min_n:
            out.append((torch.cat(cf), torch.cat(cu)))
            cf, cu = [], []
    if cf:
        if out:
            out[-1] = (torch.cat([out[-1][0]] + cf), torch.cat([out[-1][1]] + cu))
        else:
            out.append((torch.cat(cf), torch.cat(cu)))
    return [(a.numel(), a.mean().item(), b.mean().item()) for a, b in out]


# ====================================================================================================
# 2. dbsr_pwc_dense
# ====================================================================================================
# (h, w, C of the level's features, previous level present, P values, specialised level or 0).  ld = 448 +
# cpad(81 [+ C + 4]).  Specialised (pwc_dense_level_kernel, dense_level_of: h == w and ld == the 64x64 pyramid's):
# pairs per block 8, 4, 1, 1, so P at, below and above it.  Generic (pwc_dense_kernel): the shapes of the 128x128
# and 64x128 pyramids that dbsr_pwc_dense_supported accepts; 8x8 x 640 fills the NT = 4 LDS tile exactly
# (10 * 10 * 648 elements).
DENSE_CASES = {
    'L6': (1, 1, 196, False, (1, 8, 11), 6),
    'L5': (2, 2, 128, True, (3, 4, 5), 5),
    'L4': (4, 4, 96, True, (1, 2), 4),
    'L3': (8, 8, 64, True, (1, 2), 3),
    'g2x2': (2, 2, 196, False, (3, 9), 0),
    'g4x4': (4, 4, 128, True, (2,), 0),
    'g8x8': (8, 8, 96, True, (2,), 0),
    'g2x4': (2, 4, 128, True, (3,), 0),
}
DENSE_PARAMS = [(name, P) for name, c in DENSE_CASES.items() for P in c[4]]


def _dense_geom(name):
    h, w, C, prev, _, lvl = DENSE_CASES[name]
    base_real = 81 + (C + 4 if prev else 0)
    return h, w, base_real, BASE_OFF + cpad(base_real), lvl


def _dense_convs(base_real):
    """(start, cin, cout, out_off) of the six convs: Decoder.forward's cat([conv(x), x], 1) in the engine's layout."""
    out, cin = [], base_real
    for i in range(6):
        start = 0 if i == 5 else (BASE_OFF if i == 0 else DENSE_OFF[i - 1])
        out.append((start, cin, DENSE_OUT[i] if i < 5 else 2, DENSE_OFF[i] if i < 5 else 0))
        if i < 5:
            cin += DENSE_OUT[i]
    return out


def _dense_nr(i, cin, cout, single, specialised):
    """Sequential fp32 roundings of one output of dense conv i, read off csrc/pwc_dense.hip: one per 32-wide MFMA
    k-step of the wave's K slice (specialised: KPW = ceil(NKS / KSPLIT) consecutive steps; generic: chunks of
    KCH = 16 steps dealt round-robin to the KSPLIT waves), KSPLIT - 1 adds of the K-split reduction (kid 0 adds the
    partial sums of kid 1.. in order), the bias add, and for the dense convs the LeakyReLU (0.1f is not 0.1: one for
    the constant, one for the product)."""
    gpt = cpad(cin) // 32
    ksteps = gpt if single else 9 * gpt
    mb = (cout + 15) // 16
    ksplit = 1 if mb >= 5 else 2 if mb >= 3 else 4 if mb == 2 else 8
    if specialised:
        chain = -(-ksteps // ksplit)
    else:
        nch = -(-ksteps // 16)
        chain = min(ksteps, -(-nch // ksplit) * 16)
    return chain + (ksplit - 1) + 1 + (2 if i < 5 else 0)


_dense_cache = {}


def _dense_inputs(name, P, dtype, impulse):
    """D0 [P, h, w, ld] fp32 holding dtype values: [0, 448) the sentinel, the base channels seeded random, the pad
    channels beyond base_real PAD_VALUE; weights rounded to dtype, fp32 biases.  impulse: the base channels are
    zero except at the corner pixels, and pair p also lacks corner p % 4, so that pairs sharing a 16-slot tile differ
    in where their data sits."""
    h, w, base_real, ld, _ = _dense_geom(name)
    g = torch.Generator().manual_seed(_seed(('dense', name, P, dtype, impulse)))
    D0 = torch.full((P, h, w, ld), SENTINEL)
    base = torch.randn(P, h, w, base_real, generator=g).to(dtype).float()
    if impulse:
        corners = sorted({(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)})
        m = torch.zeros(P, h, w, 1)
        for p in range(P):
            for k, (y, x) in enumerate(corners):
                if len(corners) == 1 or k != p % len(corners):
                    m[p, y, x] = 1.0
        base = base * m
    D0[..., BASE_OFF:BASE_OFF + base_real] = base
    D0[..., BASE_OFF + base_real:] = PAD_VALUE
    wkey = ('dense-w', name, dtype)
    if wkey not in _dense_cache:
        gw = torch.Generator().manual_seed(_seed(wkey))
        ws = [(torch.randn(co, ci, 3, 3, generator=gw) * (2.0 / (9 * ci)) ** 0.5).to(dtype).float()
              for _, ci, co, _ in _dense_convs(base_real)]
        bs = [torch.randn(co, generator=gw) * 0.1 for _, _, co, _ in _dense_convs(base_real)]
        _dense_cache[wkey] = (ws, bs)
    return D0, _dense_cache[wkey]


def _dense_run(name, D0, wb, dtype, fused):
    """dbsr_pwc_dense, or the plan.conv chain PWCPlanner.build emits with FUSED_DENSE off, on a copy of D0.
    Returns (D [P, h, w, ld] in dtype, flow [P, h, w, 8] fp32) on the CPU; the flow buffer is prefilled with the
    sentinel."""
    L, E, stream, W = _env(dtype)
    h, w, base_real, ld, _ = _dense_geom(name)
    P = D0.shape[0]
    ws, bs = wb
    pkey = ('dense-packed', name, dtype)
    if pkey not in _dense_cache:
        _dense_cache[pkey] = [W.conv(_conv_mod(wt, b)) for wt, b in zip(ws, bs)]
    pcs = _dense_cache[pkey]
    D = E.NHWC(P, h, w, ld, dtype, DEV)
    D.t.copy_(D0.to(DEV))
    fl = _sentinel_nhwc(E, P, h, w, 8, torch.float32)
    if fused:
        convs = (L.PwcDenseConv * 6)()
        for i, (pc, (start, cin, cout, off)) in enumerate(zip(pcs, _dense_convs(base_real))):
            cg = cpad(pc.cin) // 8
            convs[i] = L.PwcDenseConv(pc.w.data_ptr(), pc.bias.data_ptr(), 9 * cg * 8, cg, start, pc.cout, off)
        L.check(L.lib().dbsr_pwc_dense(P, h, w, D.d(0), BASE_OFF, convs, fl.d(0), stream), 'dbsr_pwc_dense')
    else:
        plan = E.Plan()
        for i, (start, cin, cout, off) in enumerate(_dense_convs(base_real)):
            if i < 5:
                plan.conv('dense%d' % i, pcs[i], P, D, start, (h, w), D, off, L.ACT_LRELU, cin=cin)
            else:
                plan.conv('flow', pcs[5], P, D, 0, (h, w), None, 0, L.ACT_NONE, cin=cin, y_desc=fl.d(0))
        plan.finalize_workspace(DEV)
        plan.run(stream)
    torch.cuda.synchronize()
    return D.t.cpu(), fl.t.cpu()


def _dense_fused(name, P, dtype, impulse):
    key = ('dense-out', name, P, dtype, impulse)
    if key not in _dense_cache:
        D0, wb = _dense_inputs(name, P, dtype, impulse)
        _dense_cache[key] = (D0, wb) + _dense_run(name, D0, wb, dtype, True)
    return _dense_cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize('impulse', [False, True], ids=['random', 'corners'])
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('name,P', DENSE_PARAMS)
def test_dense_teacher_forced(name, P, dtype, impulse):
    """Every one of the six convs against float64 conv2d of the kernel's own stored input slice
    D[start_i, start_i + cin_i): the five dense outputs within 0.5 u + A, the fp32 flow within A (n_r: _dense_nr).
    The base and pad channels [448, ld) come back bitwise, channels 2..7 of the flow buffer are untouched.  The
    corner-impulse inputs exercise the one-pixel LDS border (a tap that wraps into a neighbouring row or pair sees
    data where the reference sees zero padding) and, at 1x1, the centre-tap-only path."""
    L = _env(dtype)[0]
    h, w, base_real, ld, lvl = _dense_geom(name)
    assert L.lib().dbsr_pwc_dense_supported(h, w, ld) == 1
    D0, (ws, bs), D, fl = _dense_fused(name, P, dtype, impulse)
    assert_bitwise(D[..., BASE_OFF:], D0[..., BASE_OFF:].to(dtype), 'base and pad channels')
    assert_sentinel(fl[..., 2:], 'flow channels 2..7')
    for i, (start, cin, cout, off) in enumerate(_dense_convs(base_real)):
        x = nchw(D[..., start:start + cin])
        y = F.conv2d(x, ws[i].double(), bs[i].double(), padding=1)
        S = F.conv2d(x.abs(), ws[i].double().abs(), bs[i].double().abs(), padding=1)
        n_r = _dense_nr(i, cin, cout, h * w == 1, lvl != 0)
        what = 'dense %s P=%d %s conv %d' % (name, P, dtype, i)
        if i < 5:
            assert_single_rounding(nchw(D[..., off:off + cout]), lrelu(y), S, n_r, dtype, what)
        else:
            assert_single_rounding(nchw(fl[..., :2]), y, S, n_r, torch.float32, what)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('name', list(DENSE_CASES))
def test_dense_pairs_isolated(name, dtype):
    """Pairs that share a block (and, at 1x1 .. 2x4, one 16-slot MFMA column tile) must not see each other's pixels:
    with the corner-impulse inputs, where neighbouring pairs differ in which corners hold data, every pair of the
    largest-P run equals its own single-pair run bitwise (dense outputs and flow)."""
    P = DENSE_CASES[name][4][-1]
    D0, wb, D, fl = _dense_fused(name, P, dtype, True)
    for p in range(P):
        D1, fl1 = _dense_run(name, D0[p:p + 1], wb, dtype, True)
        assert_bitwise(D[p:p + 1], D1, 'pair %d of %d: D' % (p, P))
        assert_bitwise(fl[p:p + 1], fl1, 'pair %d of %d: flow' % (p, P))


def _dense_forced_units(name, D, fl, wb, dtype):
    """Teacher-forced errors of a path's stored D / flow, conv by conv, in units: u for the five dense outputs, the
    fused kernel's allowance A (pwc_ref: what fp32 outputs are measured in) for the flow."""
    h, w, base_real, _, lvl = _dense_geom(name)
    ws, bs = wb
    dense, flow = [], None
    for i, (start, cin, cout, off) in enumerate(_dense_convs(base_real)):
        x = nchw(D[..., start:start + cin])
        y = F.conv2d(x, ws[i].double(), bs[i].double(), padding=1)
        if i < 5:
            dense.append(err_units(nchw(D[..., off:off + cout]), lrelu(y), dtype).reshape(-1))
        else:
            S = F.conv2d(x.abs(), ws[i].double().abs(), bs[i].double().abs(), padding=1)
            A = _dense_nr(i, cin, cout, h * w == 1, lvl != 0) * 2.0 ** -24 * S
            flow = ((nchw(fl[..., :2]) - y).abs() / A).reshape(-1)
    return torch.cat(dense), flow


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('name', list(DENSE_CASES))
def test_dense_vs_per_conv(name, dtype):
    """The fused kernel against the plan.conv chain of FUSED_DENSE off on the same inputs, each path teacher-forced
    conv by conv from its own stored D (every intermediate of either path is in global memory), in units of u (the
    fp32 flow in units of the allowance A): fused max <= 1.5 x per-conv max + 0.5, fused mean <= 1.25 x per-conv
    mean, over the five dense outputs of the case's largest P (>= 1024 elements).

    Not compared: the two free-running chains against one float64 chain that rounds each dense output.  There both
    paths agree with the reference except for a handful of rounding flips (an fp32 sum within ~1e-7 of a 16-bit
    rounding boundary lands on either side depending on the summation order), each amplified by the convs behind it;
    which path flips is a coin toss, and max and mean compare 0-3 such events (measured on MI355X, 4x4 x 672 bf16:
    fused 11 u, per-conv 0.06 u, with every conv of both paths inside the single-rounding bound).

    Measured on MI355X, fused / per-conv (dense max, dense mean; flow max in units of A), fp16 then bf16:
    L6 0.502 / 0.501, 0.2429 / 0.2430, 0.028 / 0.025; 0.500 / 0.500, 0.2461 / 0.2461, 0.033 / 0.033.
    L5 0.501 / 0.501, 0.2430 / 0.2429, 0.008 / 0.014; 0.500 / 0.500, 0.2424 / 0.2424, 0.007 / 0.016.
    L4 0.504 / 0.516, 0.2448 / 0.2448, 0.007 / 0.017; 0.500 / 0.500, 0.2447 / 0.2447, 0.008 / 0.020.
    L3 0.537 / 0.537, 0.2452 / 0.2452, 0.008 / 0.043; 0.500 / 0.500, 0.2452 / 0.2452, 0.010 / 0.034.
    2x2 0.501 / 0.508, 0.2413 / 0.2413, 0.006 / 0.025; 0.500 / 0.500, 0.2448 / 0.2448, 0.005 / 0.014.
    4x4 0.507 / 0.500, 0.2437 / 0.2441, 0.005 / 0.010; 0.500 / 0.500, 0.2435 / 0.2433, 0.005 / 0.019.
    8x8 0.544 / 0.534, 0.2454 / 0.2454, 0.006 / 0.021; 0.506 / 0.500, 0.2452 / 0.2451, 0.005 / 0.034.
    2x4 0.504 / 0.502, 0.2441 / 0.2441, 0.005 / 0.014; 0.500 / 0.500, 0.2421 / 0.2421, 0.004 / 0.021."""
    P = DENSE_CASES[name][4][-1]
    D0, wb, D, fl = _dense_fused(name, P, dtype, False)
    Du, flu = _dense_run(name, D0, wb, dtype, False)
    ef, ff = _dense_forced_units(name, D, fl, wb, dtype)
    eu, fu = _dense_forced_units(name, Du, flu, wb, dtype)
    print('dense-vs-per-conv %s %s P=%d: dense max %.3f / %.3f, mean %.4f / %.4f (n %d), flow max (units of A) '
          '%.3f / %.3f' % (name, dtype, P, ef.max(), eu.max(), ef.mean(), eu.mean(), ef.numel(), ff.max(), fu.max()))
    assert ef.numel() >= 1024
    assert ef.max() <= 1.5 * eu.max() + 0.5
    assert ff.max() <= 1.5 * fu.max() + 0.5
    assert ef.mean() <= 1.25 * eu.mean()


def _fake(L, ptr, dtype, hw, ld, c0=0):
    return L.Tensor(ptr, dtype, hw * ld, ld, c0, L.FrameMap(1, 1, 0, 1))


def _fake_dense_convs(L, base_real, edit=None):
    rows = []
    for i, (start, cin, cout, off) in enumerate(_dense_convs(base_real)):
        cg = cpad(cin) // 8
        rows.append([1 << 23, 1 << 24, 9 * cg * 8, cg, start, cout, off])
    if edit:
        edit(rows)
    return (L.PwcDenseConv * 6)(*[L.PwcDenseConv(*r) for r in rows])


def test_dense_rejects_bad_arguments():
    """Host-side checks only (fake pointers; each returns before any launch): the sizes with no LDS tile -- 4x8 and
    8x16, the level-4 / level-3 shapes of a 64x128 pyramid, and 1x2 x 544, its level 6: 8 pairs of 3x4 bordered
    pixels x 552 channels are 52,992 elements, beyond the 44,352 of the
    NT = 1 tile, so the planner keeps the per-conv path there -- a wrong dtype, a flow that is not fp32, a D layout
    that is not 8-aligned, a conv whose packed K is not 9 taps of cin padded to 32, an input slice beyond ld, an
    output slice that overlaps its input."""
    from dbsr_amd import _lib as L
    lib = L.lib()
    for name in DENSE_CASES:
        h, w, _, ld, _ = _dense_geom(name)
        assert lib.dbsr_pwc_dense_supported(h, w, ld) == 1, name
    for h, w, ld in [(4, 8, 640), (8, 16, 608), (4, 8, 672), (8, 16, 640), (1, 2, 544)]:
        assert lib.dbsr_pwc_dense_supported(h, w, ld) == 0
        base_real = 81 if ld == 544 else ld - BASE_OFF - 11         # any conv list: the size is refused first
        D, fl = _fake(L, 1 << 20, L.DBSR_F16, h * w, ld), _fake(L, 1 << 21, L.DBSR_F32, h * w, 8)
        assert lib.dbsr_pwc_dense(2, h, w, D, BASE_OFF, _fake_dense_convs(L, base_real), fl, None) == -1
        assert b'pwc_dense' in lib.dbsr_last_error()
    D, fl = _fake(L, 1 << 20, L.DBSR_F16, 1, 544), _fake(L, 1 << 21, L.DBSR_F32, 1, 8)
    ok = _fake_dense_convs(L, 81)
    D32 = _fake(L, 1 << 20, L.DBSR_F32, 1, 544)
    assert lib.dbsr_pwc_dense(2, 1, 1, D32, BASE_OFF, ok, fl, None) == -1
    assert b'bf16 or fp16' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_dense(2, 1, 1, D, BASE_OFF, ok, _fake(L, 1 << 21, L.DBSR_F16, 1, 8), None) == -1
    assert b'flow must be fp32' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_dense(2, 1, 1, D, BASE_OFF, ok, _fake(L, 1 << 21, L.DBSR_F32, 1, 8, c0=7), None) == -1
    assert b'flow must be fp32' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_dense(2, 1, 1, L.NULL_TENSOR, BASE_OFF, ok, fl, None) == -1
    assert b'null' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_dense(2, 1, 1, D, BASE_OFF, None, fl, None) == -1
    assert b'null' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_dense(2, 1, 1, _fake(L, 1 << 20, L.DBSR_F16, 1, 544, c0=8), BASE_OFF, ok, fl, None) == -1
    assert b'D layout' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_dense(2, 1, 1, D, BASE_OFF + 4, ok, fl, None) == -1
    assert b'D layout' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_dense(2, 9, 9, D, BASE_OFF, ok, fl, None) == -1
    assert b'1..64 pixels' in lib.dbsr_last_error()

    def bad_kp(rows):
        rows[1][2] -= 8

    def bad_slice(rows):
        rows[0][4] = 456

    def bad_out(rows):
        rows[2][6] = rows[2][4]
    for edit, msg in [(bad_kp, b'cin padded to 32'), (bad_slice, b'input slice exceeds ld'),
                      (bad_out, b'below its input slice')]:
        assert lib.dbsr_pwc_dense(2, 1, 1, D, BASE_OFF, _fake_dense_convs(L, 81, edit), fl, None) == -1
        assert msg in lib.dbsr_last_error(), lib.dbsr_last_error()


# ====================================================================================================
# 1. dbsr_pwc_level_prep
# ====================================================================================================
# level size -> (C, previous level's C or None, fltBackwarp (engine.BACKWARP_SCALE))
PREP_LEVELS = {1: (196, None, 1.0), 2: (128, 196, 0.625), 4: (96, 128, 1.25), 8: (64, 96, 2.5), 16: (32, 64, 5.0)}
# flow kinds: 'rand' flows of ~0.3 h pixels; 'far' (c) flows of ~+-1.5 h pixels, most samples outside the image;
# 'ident' (a) zero ConvT weights and bias: the identity warp; 'shift' (b) zero weights, bias (2, -3): an exact
# integer shift; 'impulse' (d): the shift on features that are zero except at the corner pixels and columns
# W/2 - 1 and W/2 (7 and 8 at h = 16: x < 8 and x >= 8 come from different 16-wide MFMA windows)
PREP_EXACT = ('ident', 'shift', 'impulse')
PREP_KINDS = ('rand', 'far') + PREP_EXACT
# chosen so that no case's float64 reference has a weight mass within 1e-4 of the mask threshold
# (test_prep_mask_exclusions; seed 0 put one of the 36 pixels of the 2x2, P = 9, bf16 case at 0.9991)
PREP_SEED = 1


def _prep_prev(h):
    """(prev_base, prev_cin, prev_ld) of the level below an h x h level."""
    _, pC, _ = PREP_LEVELS[h]
    pbase = 81 if pC == 196 else 81 + pC + 4
    return pbase, BASE_OFF + pbase, BASE_OFF + cpad(pbase)


_prep_cache = {}


def _prep_inputs(h, P, dtype, kind, frames=None):
    """Seeded operands of one level_prep call as CPU fp32 tensors holding storage-dtype values.
    first / second [P, h, h, cpad(C)] (pad channels zero: the extractor writes them so, and the correlation sums
    over the padded width); prev D [P, h/2, h/2, prev_ld] with the channels from prev_cin to its end PAD_VALUE;
    prev flow fp32 [P, h/2, h/2, 8] with channels 2..7 PAD_VALUE; the ConvT weights and biases."""
    C, pC, scale = PREP_LEVELS[h]
    g = torch.Generator().manual_seed(_seed(('prep', PREP_SEED, h, P, dtype, kind)))
    case = {'h': h, 'C': C, 'P': P, 'dtype': dtype, 'kind': kind, 'prev': pC is not None, 'scale': scale}
    CP = cpad(C)
    for k in ('first', 'second'):
        t = torch.zeros(P, h, h, CP)
        t[..., :C] = torch.randn(P, h, h, C, generator=g).to(dtype).float()
        if kind == 'impulse':
            m = torch.zeros(1, h, h, 1)
            for y in sorted({0, h // 2, h - 1}):
                for x in sorted({0, h // 2 - 1, h // 2, h - 1}):
                    if x >= 0:
                        m[0, y, x] = 1.0
            t = t * m
        case[k] = t
    if pC is None:
        return case
    pbase, pcin, pld = _prep_prev(h)
    ph = h // 2
    pD = torch.full((P, ph, ph, pld), PAD_VALUE)
    pD[..., :pcin] = torch.randn(P, ph, ph, pcin, generator=g).to(dtype).float()
    pfl = torch.full((P, ph, ph, 8), PAD_VALUE)
    amp = {'rand': 0.3, 'far': 1.5}.get(kind, 0.3) * h / scale
    pfl[..., :2] = torch.randn(P, ph, ph, 2, generator=g) * amp
    wflow = torch.randn(2, 2, 4, 4, generator=g) * 0.35
    bflow = torch.randn(2, generator=g) * 0.1
    wfeat = torch.randn(pcin, 2, 4, 4, generator=g) * (1.0 / pcin) ** 0.5
    bfeat = torch.randn(2, generator=g) * 0.1
    if kind in PREP_EXACT:
        wflow = torch.zeros_like(wflow)
        bflow = torch.zeros(2) if kind == 'ident' else torch.tensor([2.0, -3.0])
        if kind != 'ident':
            # backwarp normalises the flow by (W - 1) / 2 and grid_sample maps back by W / 2: a flow f moves the
            # sample by f * scale * W / (W - 1) pixels, so the shift is the integer (2, -3) for scale = (W - 1) / W,
            # and then every step of the fp32 position is exact (W is a power of two)
            case['scale'] = (h - 1.0) / h
    case.update(pD=pD, pflow=pfl, wflow=wflow, bflow=bflow, wfeat=wfeat, bfeat=bfeat, pcin=pcin, pld=pld)
    return case


def _convt64(x, w, b):
    return F.conv_transpose2d(x, w, b, stride=2, padding=1)


def _prep_reference(case):
    """float64 references of every output group, from the operands alone (CPU only)."""
    dtype, C, h = case['dtype'], case['C'], case['h']
    first, second = nchw(case['first'][..., :C]), nchw(case['second'][..., :C])
    ref = {}
    if case['prev']:
        x = nchw(case['pflow'][..., :2])
        wf, bf = case['wflow'].double(), case['bflow'].double()
        ref['upflow'], ref['S_upflow'] = _convt64(x, wf, bf), _convt64(x.abs(), wf.abs(), bf.abs())
        x = nchw(case['pD'][..., :case['pcin']])
        wt16, wt32, bt = rnd(case['wfeat'], dtype), case['wfeat'].double(), case['bfeat'].double()
        ref['upfeat'], ref['S_upfeat'] = _convt64(x, wt16, bt), _convt64(x.abs(), wt16.abs(), bt.abs())
        ref['upfeat32'], ref['upfeat_wdiff'] = _convt64(x, wt32, bt), _convt64(x, wt16 - wt32, None).abs()
        ref['S_upfeat32'] = _convt64(x.abs(), wt32.abs(), bt.abs())
        warped, mass = backwarp64(second, ref['upflow'] * case['scale'])[:2]
        amb = mask_ambiguous(mass)
        ref['amb_share'] = amb.double().mean().item()
        # a cost-volume output reads the warped pixels of its 9x9 window
        ref['vol_ok'] = F.max_pool2d(amb.double(), 9, stride=1, padding=4) == 0
        second = rnd(warped, dtype)
        ref['warped'] = second
    else:
        ref['amb_share'] = 0.0
        ref['vol_ok'] = torch.ones(case['P'], 1, h, h, dtype=torch.bool)
    vol, S = correlation64(first, second)
    ref['vol'], ref['S_vol'] = lrelu(vol), S / C
    return ref


def _prep_run(case, fused, maps=None):
    """dbsr_pwc_level_prep, or the five launches PWCPlanner.build emits with FUSED_PREP off (two ConvTs, backwarp,
    assemble, correlation), into a D [P, h, h, ld] prefilled with the sentinel.  maps = (first_map, second_map,
    frames): the features are `frames` images and pair p reads first_map(p) / second_map(p).  Returns D on the CPU
    (per-op: also the fp32 upflow and upfeat)."""
    dtype, C, h, P = case['dtype'], case['C'], case['h'], case['P']
    L, E, stream, W = _env(dtype)
    lib = L.lib()
    base_real = 81 + (C + 4 if case['prev'] else 0)
    ld = BASE_OFF + cpad(base_real)
    D = _sentinel_nhwc(E, P, h, h, ld, dtype)
    nfr = case['first'].shape[0]
    fa, fb = E.NHWC(nfr, h, h, cpad(C), dtype, DEV), E.NHWC(case['second'].shape[0], h, h, cpad(C), dtype, DEV)
    fa.t.copy_(case['first'].to(DEV))
    fb.t.copy_(case['second'].to(DEV))
    fmap, smap = maps if maps else (L.IDENTITY, L.IDENTITY)
    extra = {}
    if not case['prev']:
        if fused:
            L.check(lib.dbsr_pwc_level_prep(P, h, h, C, 1.0, fa.d(0, fmap), fb.d(0, smap), D.d(BASE_OFF),
                                            L.NULL_TENSOR, 0, L.NULL_TENSOR, None, None, None, None, stream), 'prep')
        else:
            L.check(lib.dbsr_correlation(P, h, h, C, fa.d(0, fmap), fb.d(0, smap), D.d(BASE_OFF), 1, stream), 'corr')
    else:
        ph = h // 2
        pD = E.NHWC(P, ph, ph, case['pld'], dtype, DEV)
        pD.t.copy_(case['pD'].to(DEV))
        pfl = E.NHWC(P, ph, ph, 8, torch.float32, DEV)
        pfl.t.copy_(case['pflow'].to(DEV))
        wf, bf = E.pack_convt(types.SimpleNamespace(weight=case['wflow'], bias=case['bflow']), DEV)
        wt, bt = E.pack_convt(types.SimpleNamespace(weight=case['wfeat'], bias=case['bfeat']), DEV)
        if fused:
            cin8 = wt.shape[-1]
            wt16 = F.pad(wt.reshape(32, cin8), (0, (cin8 + 31) // 32 * 32 - cin8)).to(dtype).contiguous()
            L.check(lib.dbsr_pwc_level_prep(P, h, h, C, case['scale'], fa.d(0, fmap), fb.d(0, smap), D.d(BASE_OFF),
                                            pD.d(0), case['pcin'], pfl.d(0), wf.data_ptr(), bf.data_ptr(),
                                            wt16.data_ptr(), bt.data_ptr(), stream), 'prep')
        else:
            fu = _sentinel_nhwc(E, P, h, h, 8, torch.float32)
            fe = E.NHWC(P, h, h, 2, torch.float32, DEV)
            ws = E.NHWC(P, h, h, cpad(C), dtype, DEV)
            L.check(lib.dbsr_conv_transpose_k4s2(P, ph, ph, 2, 2, pfl.d(0), wf.data_ptr(), bf.data_ptr(), fu.d(0),
                                                 stream), 'upflow')
            L.check(lib.dbsr_conv_transpose_k4s2(P, ph, ph, case['pcin'], 2, pD.d(0), wt.data_ptr(), bt.data_ptr(),
                                                 fe.d(0), stream), 'upfeat')
            L.check(lib.dbsr_backwarp(P, h, h, C, fb.d(0, smap), fu.d(0), case['scale'], ws.d(0), stream), 'backwarp')
            L.check(lib.dbsr_pwc_assemble(P, h, h, C, fa.d(0, fmap), fu.d(0), fe.d(0), D.d(BASE_OFF), stream), 'asm')
            L.check(lib.dbsr_correlation(P, h, h, C, fa.d(0, fmap), ws.d(0), D.d(BASE_OFF), 1, stream), 'corr')
            torch.cuda.synchronize()
            extra = {'upflow32': fu.t.cpu(), 'upfeat32': fe.t.cpu()}
    torch.cuda.synchronize()
    return D.t.cpu(), extra


def _prep_vol_nr(h, C):
    """Cost-volume roundings (csrc/pwc_fused.hip): h >= 8 one per 32-channel MFMA k-step, else one fmaf per padded
    channel; then the division by C and the LeakyReLU (constant and product)."""
    return (cpad(C) // 32 if h >= 8 else cpad(C)) + 1 + 2


PREP_PARAMS = [(h, P, kind) for h in PREP_LEVELS for P in (1, 3, 9)
               for kind in (PREP_KINDS if h > 1 else ('rand', 'impulse'))
               if kind == 'rand' or P == 3]


def test_prep_mask_exclusions():
    """CPU only: in every level_prep case the share of pixels whose float64 weight mass lies within 1e-4 of the
    mask threshold stays under the 1 % cap (measured: 0 in every case)."""
    for h, P, kind in PREP_PARAMS:
        for dtype in D16:
            share = _prep_reference(_prep_inputs(h, P, dtype, kind))['amb_share']
            assert share <= 0.01, (h, P, kind, dtype, share)


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('h,P,kind', PREP_PARAMS)
def test_level_prep_groups(h, P, kind, dtype):
    """Each output group of D on its own.  upflow (fp32 weights; n_r = 32 fmaf of the <= 4 taps x 8 channels + the
    bias) and upfeat (weights rounded to the storage dtype, since the kernel runs it on MFMA from upfeat16; n_r =
    prev_cin32 / 32 MFMA k-steps + 4 adds of the (pixel, tap) terms + the bias) within 0.5 u + A of float64
    conv_transpose2d of the stored previous flow / previous D; prev_cin = 448 + base is no multiple of 32 at any
    level and the channels behind it hold 1.5.  The copy of `first` is bitwise.  The cost volume: for the exact
    flows (identity, integer shift) and the level with no previous one, 0.5 u + A against float64 correlation / C
    + LeakyReLU of the shifted image (n_r: _prep_vol_nr); for the random flows, against backwarp by the float64
    upflow, rounded to the storage dtype, with 1.5 x the per-op path's error + 0.5 u and 1.25 x its mean (pixels
    whose window holds a warped pixel with a weight mass within 1e-4 of 0.999 left out, at most 1 %).  The 81
    channels in front of D's base, and whatever lies behind the written groups, stay the sentinel.

    Measured on MI355X, cost volume with random flows, fused / per-op (bitwise alike in every case), max and mean
    in units of u over fp16 / bf16 and P: h = 2 max 0.33-0.49, mean 0.001-0.008; h = 4 max 0.50, mean 0.003-0.024;
    h = 8 max 0.50-6.93, mean 0.004-0.070; h = 16 max 2.19-55.4, mean 0.008-0.118 (above 0.5 u: a warped pixel whose
    fp32 value rounds to the other 16-bit neighbour than the float64 one, seen by up to 81 small outputs); no pixel
    left out by the mask rule."""
    case = _prep_inputs(h, P, dtype, kind)
    ref = _prep_reference(case)
    C = case['C']
    D, _ = _prep_run(case, True)
    c0 = BASE_OFF
    assert_sentinel(D[..., :c0], 'dense channels')
    assert_sentinel(D[..., c0 + 81 + (C + 4 if case['prev'] else 0):], 'pad behind the base channels')
    what = 'prep h=%d P=%d %s %s' % (h, P, kind, dtype)
    if case['prev']:
        assert_bitwise(D[..., c0 + 81:c0 + 81 + C], case['first'][..., :C].to(dtype), 'copy of first')
        assert_single_rounding(nchw(D[..., c0 + 81 + C:c0 + 83 + C]), ref['upflow'], ref['S_upflow'], 33, dtype,
                               what + ' upflow')
        assert_single_rounding(nchw(D[..., c0 + 83 + C:c0 + 85 + C]), ref['upfeat'], ref['S_upfeat'],
                               (case['pcin'] + 31) // 32 + 5, dtype, what + ' upfeat')
    assert ref['amb_share'] <= 0.01
    vol = nchw(D[..., c0:c0 + 81])
    ok = ref['vol_ok'].expand_as(vol)
    if kind in PREP_EXACT or not case['prev']:
        assert_single_rounding(vol, ref['vol'], ref['S_vol'], _prep_vol_nr(h, C), dtype, what + ' cost volume', ok)
    else:
        Du, _ = _prep_run(case, False)
        ef, eu = err_units(vol, ref['vol'], dtype)[ok], err_units(nchw(Du[..., c0:c0 + 81]), ref['vol'], dtype)[ok]
        print('%s cost volume: fused / per-op max %.3f / %.3f, mean %.4f / %.4f (n %d), left out %.3f %%'
              % (what, ef.max(), eu.max(), ef.mean(), eu.mean(), ef.numel(), 100 * ref['amb_share']))
        assert ef.max() <= 1.5 * eu.max() + 0.5
        if ef.numel() >= 1024:
            assert ef.mean() <= 1.25 * eu.mean()


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('h', [2, 4, 8, 16])
def test_level_prep_vs_per_op(h, dtype):
    """The fused launch against the five launches of FUSED_PREP off, group by group: the copy of `first` bitwise;
    upflow the 16-bit rounding of a value within one fp32 rounding step (2^-23 S) of the per-op ConvT's fp32 sum
    (the same fmaf chain); upfeat within the float64 difference of the two weight sets (rounded to the storage dtype
    for the MFMA, fp32 for the per-op kernel) on these inputs + both fp32 allowances + 0.5 u."""
    case = _prep_inputs(h, 3, dtype, 'rand')
    ref = _prep_reference(case)
    C, c0 = case['C'], BASE_OFF
    D, _ = _prep_run(case, True)
    Du, ex = _prep_run(case, False)
    assert_bitwise(D[..., c0 + 81:c0 + 81 + C], Du[..., c0 + 81:c0 + 81 + C], 'copy of first')
    uf32 = nchw(ex['upflow32'][..., :2])
    step = 2.0 ** -23 * ref['S_upflow']
    lo, hi = rnd(uf32 - step, dtype), rnd(uf32 + step, dtype)
    uf = nchw(D[..., c0 + 81 + C:c0 + 83 + C])
    assert bool(((uf >= lo) & (uf <= hi)).all()), 'upflow: %d beyond one fp32 step' % int(((uf < lo) | (uf > hi)).sum())
    assert_bitwise(Du[..., c0 + 81 + C:c0 + 83 + C], ex['upflow32'][..., :2].to(dtype), 'per-op assemble: upflow')
    ft = nchw(D[..., c0 + 83 + C:c0 + 85 + C])
    ft32 = nchw(ex['upfeat32'])
    nks = (case['pcin'] + 31) // 32
    A = 2.0 ** -24 * ((nks + 5) * ref['S_upfeat'] + (case['pcin'] + 8) * ref['S_upfeat32'])
    bound = ref['upfeat_wdiff'] + A + 0.5 * unit(ref['upfeat'], dtype, A)
    err = (ft - ft32).abs()
    print('prep-vs-per-op h=%d %s: upfeat max |diff| %.3g, worst ratio to the bound %.3f'
          % (h, dtype, err.max(), (err / bound).max()))
    assert bool((err <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('h', [1, 4, 16])
def test_level_prep_pair_maps(h, dtype):
    """The engine's pair-to-frame maps (B = 2 bursts of N = 3 frames, P = 4 pairs: first = frame b*N, second = frame
    b*N + n + 1) against identity-map runs on the gathered frames, bitwise."""
    B, N = 2, 3
    P = B * (N - 1)
    case = _prep_inputs(h, P, dtype, 'rand')
    frames = _prep_inputs(h, B * N, dtype, 'rand')
    mapped = dict(case, first=frames['first'], second=frames['first'])
    Dm, _ = _prep_run(mapped, True, maps=((N - 1, N, 0, 0), (N - 1, N, 1, 1)))
    fi = [(p // (N - 1)) * N for p in range(P)]
    si = [(p // (N - 1)) * N + p % (N - 1) + 1 for p in range(P)]
    gathered = dict(case, first=frames['first'][fi], second=frames['first'][si])
    Dg, _ = _prep_run(gathered, True)
    assert_bitwise(Dm, Dg, 'mapped against gathered')
    assert not torch.equal(bits(Dg[0]), bits(Dg[1]))


def test_level_prep_rejects_bad_arguments():
    """Host-side checks only (fake pointers; each returns before any launch)."""
    from dbsr_amd import _lib as L
    lib = L.lib()
    for h, (C, pC, _) in PREP_LEVELS.items():
        assert lib.dbsr_pwc_level_prep_supported(h, h, C) == 1
    for h, w, C in [(16, 16, 64), (32, 32, 32), (2, 4, 128), (4, 4, 128), (1, 2, 196)]:
        assert lib.dbsr_pwc_level_prep_supported(h, w, C) == 0
    F16, F32, BF = L.DBSR_F16, L.DBSR_F32, L.DBSR_BF16
    p = 1 << 20

    def call(h=4, w=4, C=96, dt=F16, first=None, second=None, D=None, pD='std', pcin=661, pfl='std', wts=True, P=2):
        first = first or _fake(L, p, dt, h * w, cpad(C))
        second = second or _fake(L, 2 * p, dt, h * w, cpad(C))
        D = D or _fake(L, 3 * p, dt, h * w, 640, BASE_OFF)
        pD = _fake(L, 4 * p, dt, h * w // 4, 672) if pD == 'std' else pD
        pfl = _fake(L, 5 * p, F32, h * w // 4, 8) if pfl == 'std' else pfl
        ws = (6 * p, 7 * p, 8 * p, 9 * p) if wts else (None, None, None, None)
        return lib.dbsr_pwc_level_prep(P, h, w, C, 1.0, first, second, D, pD, pcin, pfl, *ws, None)

    assert call(P=0) == -1 and b'bad sizes' in lib.dbsr_last_error()
    assert call(h=4, w=8) == -1 and b'no kernel' in lib.dbsr_last_error()
    assert call(C=64) == -1 and b'no kernel' in lib.dbsr_last_error()
    assert call(first=L.NULL_TENSOR) == -1 and b'null tensor' in lib.dbsr_last_error()
    assert call(dt=F32) == -1 and b'16-bit tensors' in lib.dbsr_last_error()
    assert call(second=_fake(L, 2 * p, BF, 16, 96)) == -1 and b'16-bit tensors' in lib.dbsr_last_error()
    assert call(first=_fake(L, p, F16, 16, 64)) == -1 and b'aligned slices' in lib.dbsr_last_error()
    assert call(first=_fake(L, p, F16, 16, 104, 8)) == -1 and b'aligned slices' in lib.dbsr_last_error()
    assert call(D=_fake(L, 3 * p, F16, 16, 624, BASE_OFF)) == -1 and b'exceeds ld' in lib.dbsr_last_error()
    assert call(pD=_fake(L, 4 * p, BF, 4, 672)) == -1 and b'bad previous D' in lib.dbsr_last_error()
    assert call(pfl=_fake(L, 5 * p, F32, 4, 2)) == -1 and b'previous flow' in lib.dbsr_last_error()
    assert call(pfl=_fake(L, 5 * p, F16, 4, 8)) == -1 and b'previous flow' in lib.dbsr_last_error()
    assert call(wts=False) == -1 and b'null ConvT' in lib.dbsr_last_error()
    assert call(pcin=700) == -1 and b'fewer than' in lib.dbsr_last_error()
    # a level that needs a previous one without it, and the coarsest level with one
    assert call(pD=L.NULL_TENSOR, D=_fake(L, 3 * p, F16, 16, 640, BASE_OFF)) == -1
    assert b'needs a previous level' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_level_prep(2, 1, 1, 196, 1.0, _fake(L, p, F16, 1, 224), _fake(L, 2 * p, F16, 1, 224),
                                   _fake(L, 3 * p, F16, 1, 768, BASE_OFF), _fake(L, 4 * p, F16, 1, 672), 661,
                                   _fake(L, 5 * p, F32, 1, 8), 6 * p, 7 * p, 8 * p, 9 * p, None) == -1
    assert b'level size must be twice' in lib.dbsr_last_error()


# ====================================================================================================
# 3. dbsr_pwc_extract
# ====================================================================================================
_ext_cache = {}


def _ext_weights(dtype):
    key = ('w', dtype)
    if key not in _ext_cache:
        g = torch.Generator().manual_seed(_seed(('ext-w', dtype)))
        ws, bs, st = [], [], []
        for l in range(6):
            for j in range(3):
                ci, co = (EXT_CH[l] if j == 0 else EXT_CH[l + 1]), EXT_CH[l + 1]
                ws.append((torch.randn(co, ci, 3, 3, generator=g) * (2.0 / (9 * ci)) ** 0.5).to(dtype).float())
                bs.append(torch.randn(co, generator=g) * 0.1)
                st.append(2 if j == 0 else 1)
        _ext_cache[key] = (ws, bs, st)
    return _ext_cache[key]


def _ext_frames(F_, dtype, kind):
    """[F, 64, 64, 8] fp32 holding dtype values: 3 real channels in [0, 1], pad channels zero.  'impulse': zero but
    for the four corner pixels and the four centre pixels; 'ones': constant 1.0, where every border tap matters."""
    g = torch.Generator().manual_seed(_seed(('ext-x', F_, dtype, kind)))
    x = torch.zeros(F_, 64, 64, 8)
    x[..., :3] = torch.rand(F_, 64, 64, 3, generator=g).to(dtype).float()
    if kind == 'impulse':
        m = torch.zeros(1, 64, 64, 1)
        for y in (0, 31, 32, 63):
            for xx in (0, 31, 32, 63):
                if (y in (0, 63)) == (xx in (0, 63)):
                    m[0, y, xx] = 1.0
        x = x * m
    elif kind == 'ones':
        x[..., :3] = 1.0
    return x


def _ext_run(x, dtype, fused, rgb_map=None):
    """dbsr_pwc_extract, or the 18 plan.conv launches of FUSED_EXTRACT off; the level outputs (sentinel prefill) on
    the CPU.  rgb_map = (map, frames): x holds more frames than are extracted; frame f reads image map(f)."""
    L, E, stream, W = _env(dtype)
    ws, bs, st = _ext_weights(dtype)
    if ('packed', dtype) not in _ext_cache:
        _ext_cache[('packed', dtype)] = [W.conv(_conv_mod(w, b, s)) for w, b, s in zip(ws, bs, st)]
    pcs = _ext_cache[('packed', dtype)]
    rgb = E.NHWC(x.shape[0], 64, 64, 8, dtype, DEV)
    rgb.t.copy_(x.to(DEV))
    fmap, nF = rgb_map if rgb_map else (L.IDENTITY, x.shape[0])
    levels = [_sentinel_nhwc(E, nF, 32 >> k, 32 >> k, cpad(EXT_CH[k + 1]), dtype) for k in range(6)]
    if fused:
        convs = (L.PwcExtConv * 18)(*[L.PwcExtConv(pc.w.data_ptr(), pc.bias.data_ptr(), pc.cin, pc.cout, pc.stride)
                                      for pc in pcs])
        lv = (L.Tensor * 6)(*[t.d(0) for t in levels])
        L.check(L.lib().dbsr_pwc_extract(nF, 64, 64, rgb.d(0, fmap), convs, lv, stream), 'dbsr_pwc_extract')
    else:
        plan = E.Plan()
        cur, hw = rgb, (64, 64)
        for k in range(6):
            oh = 32 >> k
            ta, tb = (E.NHWC(nF, oh, oh, cpad(EXT_CH[k + 1]), dtype, DEV) for _ in range(2))
            plan.conv('ext%d.0' % k, pcs[3 * k], nF, cur, 0, hw, ta, 0, L.ACT_LRELU,
                      xmap=fmap if k == 0 else L.IDENTITY)
            plan.conv('ext%d.2' % k, pcs[3 * k + 1], nF, ta, 0, (oh, oh), tb, 0, L.ACT_LRELU)
            plan.conv('ext%d.4' % k, pcs[3 * k + 2], nF, tb, 0, (oh, oh), levels[k], 0, L.ACT_LRELU)
            plan.keep.extend([ta, tb])
            cur, hw = levels[k], (oh, oh)
        plan.finalize_workspace(DEV)
        plan.run(stream)
    torch.cuda.synchronize()
    return [t.t.cpu() for t in levels]


def _ext_forced_errors(x, outs, dtype):
    """Per level: error (units of u) of the stored level output against the float64 three-conv chain from the
    stored previous level (level 1: the input frame), the two hidden activations rounded to the storage dtype."""
    ws, bs, st = _ext_weights(dtype)
    errs = []
    cur = nchw(x[..., :3])
    for k in range(6):
        a = cur
        for j in range(3):
            i = 3 * k + j
            a = lrelu(F.conv2d(a, ws[i].double(), bs[i].double(), stride=st[i], padding=1))
            if j < 2:
                a = rnd(a, dtype)
        C = EXT_CH[k + 1]
        errs.append(err_units(nchw(outs[k][..., :C]), a, dtype))
        cur = nchw(outs[k][..., :C])
    return errs


EXT_PARAMS = [(1, 'rand'), (3, 'rand'), (3, 'impulse'), (3, 'ones')]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
@pytest.mark.parametrize('F_,kind', EXT_PARAMS)
def test_extract_teacher_forced(F_, kind, dtype):
    """Every pyramid level against the float64 chain of its three convs computed from the kernel's own stored
    previous level, the two hidden activations (LDS-resident) rounded to the storage dtype; the 18-launch per-conv
    path (FUSED_EXTRACT off), forced the same way from its own outputs, sets the bound: per case (the maximum over
    the six levels), fused max <= 1.5 x per-conv max + 0.5 u; fused mean <= 1.25 x per-conv mean over pools of
    >= 1024 elements (levels pooled from the coarsest up).  Errors above 0.5 u are rounding flips of a hidden
    activation (the fp32 sum and the float64 value round to different 16-bit neighbours), which move a small output
    by several of its floored units: both paths show them, bitwise alike at levels 1-3 (up to 18 u), and at levels
    4-6, where the summation orders differ, in different places -- so the maximum is taken per case
    and the per-level figures are printed only.  The impulse frame (four corner and four centre pixels) and the
    constant frame exercise the taps
    that levels 5 and 6 skip as never in frame, and every border tap.  All six outputs are written in full: level
    6's pad channels 196..223 are exactly +0 over the sentinel.

    Measured on MI355X, fused / per-conv max over the six levels (units of u): F=1 random fp16 8.843 / 8.843, bf16
    1.541 / 1.541; F=3 random fp16 18.121 / 18.121, bf16 13.123 / 13.123; impulse fp16 9.849 / 9.849, bf16 13.560 /
    13.560; constant fp16 0.754 / 0.556, bf16 0.500 / 0.500.  Per-level means 0.219-0.272, equal in both paths to
    1e-3 except level 4 fp16 F=3 (random 0.2708 / 0.2500, impulse 0.2684 / 0.2447) and level 5 fp16 F=3 random
    (0.2517 / 0.3701); per-level maxima there 10.4 / 1.99 (level 4) and 0.50 / 10.5 (level 5)."""
    x = _ext_frames(F_, dtype, kind)
    outs = _ext_run(x, dtype, True)
    outs_u = _ext_run(x, dtype, False)
    assert_pos_zero(outs[5][..., 196:], 'level 6 pad channels')
    for k in range(5):
        assert outs[k].shape[-1] == EXT_CH[k + 1]
    ef, eu = _ext_forced_errors(x, outs, dtype), _ext_forced_errors(x, outs_u, dtype)
    for k in range(6):
        print('extract F=%d %s %s level %d: fused / per-conv max %.3f / %.3f, mean %.4f / %.4f'
              % (F_, kind, dtype, k + 1, ef[k].max(), eu[k].max(), ef[k].mean(), eu[k].mean()))
    e_f, e_u = max(e.max().item() for e in ef), max(e.max().item() for e in eu)
    print('extract F=%d %s %s: fused / per-conv max over the six levels %.3f / %.3f' % (F_, kind, dtype, e_f, e_u))
    assert e_f <= 1.5 * e_u + 0.5
    for n, mf, mu in _pooled_means(ef[::-1], eu[::-1]):
        print('  pooled mean over %d elements: %.4f / %.4f' % (n, mf, mu))
        assert mf <= 1.25 * mu


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', D16, ids=['fp16', 'bf16'])
def test_extract_frame_map(dtype):
    """A non-identity rgb map, as the engine passes for a burst group (frames 1, 2, 4, 5 of six), against the
    identity-map run on the gathered frames, bitwise."""
    x = _ext_frames(6, dtype, 'rand')
    mapped = _ext_run(x, dtype, True, rgb_map=((2, 3, 1, 1), 4))
    gathered = _ext_run(x[[1, 2, 4, 5]], dtype, True)
    for k in range(6):
        assert_bitwise(mapped[k], gathered[k], 'level %d' % (k + 1))
    assert not torch.equal(bits(gathered[0][0]), bits(gathered[0][1]))


def test_extract_rejects_bad_arguments():
    """Host-side checks only (fake pointers; each returns before any launch)."""
    from dbsr_amd import _lib as L
    lib = L.lib()
    assert lib.dbsr_pwc_extract_supported(64, 64) == 1
    assert lib.dbsr_pwc_extract_supported(128, 128) == 0 and lib.dbsr_pwc_extract_supported(64, 128) == 0

    def args(dt=L.DBSR_F16, conv_edit=None, lv_edit=None):
        rows = [[1 << 23, 1 << 24, EXT_CH[i // 3] if i % 3 == 0 else EXT_CH[i // 3 + 1], EXT_CH[i // 3 + 1],
                 2 if i % 3 == 0 else 1] for i in range(18)]
        if conv_edit:
            conv_edit(rows)
        lvs = [[(k + 2) << 20, dt, (32 >> k) ** 2, cpad(EXT_CH[k + 1]), 0] for k in range(6)]
        if lv_edit:
            lv_edit(lvs)
        return ((L.PwcExtConv * 18)(*[L.PwcExtConv(*r) for r in rows]),
                (L.Tensor * 6)(*[_fake(L, *r) for r in lvs]))

    rgb = _fake(L, 1 << 20, L.DBSR_F16, 64 * 64, 8)
    cv, lv = args()
    assert lib.dbsr_pwc_extract(2, 128, 128, rgb, cv, lv, None) == -1 and b'64x64' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_extract(2, 64, 64, rgb, None, lv, None) == -1 and b'null' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_extract(2, 64, 64, L.NULL_TENSOR, cv, lv, None) == -1 and b'null' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_extract(2, 64, 64, _fake(L, 1 << 20, L.DBSR_F32, 4096, 8), cv, lv, None) == -1
    assert b'16-bit' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_extract(2, 64, 64, _fake(L, 1 << 20, L.DBSR_F16, 4096, 16), cv, lv, None) == -1
    assert b'8-channel packed frame' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_extract(0, 64, 64, rgb, cv, lv, None) == -1 and b'no frames' in lib.dbsr_last_error()

    def lv_dtype(lvs):
        lvs[2][1] = L.DBSR_BF16

    def lv_ld(lvs):
        lvs[5][3] = 200

    def cv_stride(rows):
        rows[3][4] = 1

    def cv_cin(rows):
        rows[4][2] = 16

    def cv_bias(rows):
        rows[17][1] = None
    for kw, msg in [({'lv_edit': lv_dtype}, b'level 3 output'), ({'lv_edit': lv_ld}, b'level 6 output'),
                    ({'conv_edit': cv_stride}, b'conv 3 must be'), ({'conv_edit': cv_cin}, b'conv 4 must be'),
                    ({'conv_edit': cv_bias}, b'conv 17 must be')]:
        cv, lv = args(**kw)
        assert lib.dbsr_pwc_extract(2, 64, 64, rgb, cv, lv, None) == -1
        assert msg in lib.dbsr_last_error(), lib.dbsr_last_error()
