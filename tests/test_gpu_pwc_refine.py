"""The fused refiner tail (dbsr_pwc_refine: PWC-Net refiner convs 1-6 + the residual flow on the 16x16 level in
one launch, csrc/pwc_refine.hip) against the per-conv path on the same inputs and a torch fp32 reference, plus
the host-side argument checks (no GPU)."""
import types

import pytest
import torch
import torch.nn.functional as F

DEV = 'cuda'
# refiner convs 1-6 (pwcnet.py:191-203): cin, cout, dilation
TAIL = [(128, 128, 2), (128, 128, 4), (128, 96, 8), (96, 64, 16), (64, 32, 1), (32, 2, 1)]
# Check 2's absolute bounds: 3 x the per-conv path's max-abs error against the reference on these inputs
# (measured: see test_refine_vs_unfused's docstring), per (dtype, P, input kind)
UNFUSED_ERR = {(torch.float16, 1, False): 2.718e-4, (torch.float16, 3, False): 3.231e-4,
               (torch.bfloat16, 1, False): 9.991e-4, (torch.bfloat16, 3, False): 1.771e-3,
               (torch.float16, 3, True): 1.059e-4, (torch.bfloat16, 3, True): 2.672e-4}


def _case(dtype, P, corners=False):
    """Seeded inputs, each rounded to the storage dtype (fp32 tensors holding 16-bit values)."""
    gen = torch.Generator().manual_seed(100 * P + (7 if corners else 0) + (1 if dtype == torch.bfloat16 else 0))
    rnd = lambda t: t.to(dtype).float()                                          # noqa: E731
    x = rnd(torch.randn(P, 128, 16, 16, generator=gen))
    if corners:
        # zero everywhere but one pixel in each image corner: only the taps that stay inside the image may see data
        m = torch.zeros(1, 1, 16, 16)
        m[..., 0, 0] = m[..., 0, 15] = m[..., 15, 0] = m[..., 15, 15] = 1.0
        x = x * m
    ws = [rnd(torch.randn(co, ci, 3, 3, generator=gen) * (2.0 / (ci * 9)) ** 0.5) for ci, co, _ in TAIL]
    bs = [torch.randn(co, generator=gen) * 0.1 for _, co, _ in TAIL]
    res = torch.randn(P, 2, 16, 16, generator=gen) * 2.0
    return x, ws, bs, res


def _reference(x, ws, bs, res, dtype):
    """torch fp32 conv chain with the refiner's dilations, activations rounded to the storage dtype between convs."""
    for i, (w, b, (_, _, d)) in enumerate(zip(ws, bs, TAIL)):
        y = F.conv2d(x, w, b, padding=d, dilation=d)
        x = F.leaky_relu(y, 0.1).to(dtype).float() if i < 5 else y + res
    return x


def _run(x, ws, bs, res, dtype, fused):
    """Both paths through the C ABI as PWCPlanner.build emits them (refiner 4 as its centre tap); returns the flow
    [P, 2, 16, 16] fp32 on the CPU."""
    from dbsr_amd import _lib as L
    from dbsr_amd.engine import NHWC, Plan, _Weights
    P = x.shape[0]
    stream = L.stream_ptr(DEV)
    W = _Weights(dtype, torch.device(DEV), stream)
    mods = [types.SimpleNamespace(weight=w.to(DEV), bias=b.to(DEV), stride=(1,), padding=(d,), dilation=(d,))
            for w, b, (_, _, d) in zip(ws, bs, TAIL)]
    mods[3] = types.SimpleNamespace(weight=ws[3][:, :, 1:2, 1:2].contiguous().to(DEV), bias=bs[3].to(DEV), stride=(1,),
                                    padding=(0,), dilation=(1,))
    pcs = [W.conv(m) for m in mods]
    xin = NHWC(P, 16, 16, 128, dtype, DEV)
    xin.t.copy_(x.permute(0, 2, 3, 1).to(DEV))
    fl2 = NHWC(P, 16, 16, 8, torch.float32, DEV)
    fl2.t[..., :2] = res.permute(0, 2, 3, 1).to(DEV)
    out = NHWC(P, 16, 16, 2, torch.float32, DEV)
    plan = Plan()
    if fused:
        convs = (L.PwcRefineConv * 6)(*[L.PwcRefineConv(pc.w.data_ptr(), pc.bias.data_ptr(), pc.cin, pc.cout, pc.kh,
                                                        pc.dil) for pc in pcs])
        plan.keep.append(convs)
        plan.add('refine', L.lib().dbsr_pwc_refine, P, 16, 16, xin.d(0), convs, fl2.d(0), out.d(0))
    else:
        bufs = [NHWC(P, 16, 16, co, dtype, DEV) for _, co, _ in TAIL[:5]]
        cur = xin
        for i in range(5):
            plan.conv('refiner%d' % (i + 1), pcs[i], P, cur, 0, (16, 16), bufs[i], 0, L.ACT_LRELU)
            cur = bufs[i]
        plan.conv('refiner6', pcs[5], P, cur, 0, (16, 16), None, 0, L.ACT_NONE, y_desc=out.d(0), res=fl2)
        plan.keep.extend(bufs)
    plan.finalize_workspace(DEV)
    plan.run(stream)
    torch.cuda.synchronize()
    return out.t.permute(0, 3, 1, 2).contiguous().cpu()


_cache = {}


def _errors(dtype, P, corners):
    """(e_f, e_u, quantum): each path's max-abs error against the reference, computed once per case."""
    key = (dtype, P, corners)
    if key not in _cache:
        x, ws, bs, res = _case(dtype, P, corners)
        ref = _reference(x, ws, bs, res, dtype)
        e_f = (_run(x, ws, bs, res, dtype, True) - ref).abs().max().item()
        e_u = (_run(x, ws, bs, res, dtype, False) - ref).abs().max().item()
        _cache[key] = (e_f, e_u, torch.finfo(dtype).eps * ref.abs().max().item())
    return _cache[key]


@pytest.mark.gpu
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_refine_vs_unfused(dtype, P):
    """Check 1: e_f <= 1.5 e_u + one quantum of the storage dtype at the flow's magnitude (e_f / e_u: the fused /
    per-conv path's max-abs error against the fp32 reference chain; the suite's convention for fused PWC kernels).
    Check 2: e_f <= 3 x the per-conv path's error on these inputs (UNFUSED_ERR).

    Measured on MI355X (fused / per-conv max-abs error, |flow| max ~6): fp16 P=1 3.586e-4 / 2.718e-4, fp16 P=3
    2.700e-4 / 3.231e-4, bf16 P=1 9.978e-4 / 9.991e-4, bf16 P=3 1.477e-3 / 1.771e-3; corner inputs (P=3): fp16
    1.059e-4 / 1.059e-4, bf16 2.892e-4 / 2.672e-4."""
    e_f, e_u, q = _errors(dtype, P, False)
    print('refine %s P=%d: fused err %.4g, per-conv err %.4g, quantum %.4g' % (dtype, P, e_f, e_u, q))
    assert e_f <= 1.5 * e_u + q
    assert e_f <= 3.0 * UNFUSED_ERR[(dtype, P, False)]


@pytest.mark.gpu
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_refine_dead_taps(dtype):
    """Input zero except one pixel in each image corner: a wrongly skipped tap row or an unmasked out-of-image
    column changes the flow far beyond rounding; the bound is check 2's."""
    e_f, e_u, q = _errors(dtype, 3, True)
    print('refine corners %s: fused err %.4g, per-conv err %.4g, quantum %.4g' % (dtype, e_f, e_u, q))
    assert e_f <= 3.0 * UNFUSED_ERR[(dtype, 3, True)]


def _fake_args(L, dtype, convs=None):
    fm = L.FrameMap(1, 1, 0, 1)
    x = L.Tensor(1 << 20, dtype, 16 * 16 * 128, 128, 0, fm)
    fl = L.Tensor(1 << 21, L.DBSR_F32, 16 * 16 * 8, 8, 0, fm)
    out = L.Tensor(1 << 22, L.DBSR_F32, 16 * 16 * 2, 2, 0, fm)
    shapes = convs or [(128, 128, 3, 2), (128, 128, 3, 4), (128, 96, 3, 8), (96, 64, 1, 1), (64, 32, 3, 1), (32, 2, 3, 1)]
    cv = (L.PwcRefineConv * 6)(*[L.PwcRefineConv(1 << 23, 1 << 24, ci, co, k, d) for ci, co, k, d in shapes])
    return x, cv, fl, out


def test_refine_rejects_bad_arguments():
    """Host-side checks only (fake pointers, nothing is launched): another size, another dtype or another conv list
    is DBSR_E_ARG with a message."""
    from dbsr_amd import _lib as L
    lib = L.lib()
    assert lib.dbsr_pwc_refine_supported(16, 16, L.DBSR_F16) == 1
    assert lib.dbsr_pwc_refine_supported(16, 16, L.DBSR_BF16) == 1
    assert lib.dbsr_pwc_refine_supported(16, 16, L.DBSR_F32) == 0
    assert lib.dbsr_pwc_refine_supported(16, 32, L.DBSR_F16) == 0
    assert lib.dbsr_pwc_refine_supported(8, 8, L.DBSR_F16) == 0
    x, cv, fl, out = _fake_args(L, L.DBSR_F16)
    assert lib.dbsr_pwc_refine(2, 8, 8, x, cv, fl, out, None) == -1                 # wrong size
    assert b'16x16' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_refine(2, 16, 24, x, cv, fl, out, None) == -1
    assert b'16x16' in lib.dbsr_last_error()
    x32, cv, fl, out = _fake_args(L, L.DBSR_F32)
    assert lib.dbsr_pwc_refine(2, 16, 16, x32, cv, fl, out, None) == -1             # wrong dtype
    assert b'bf16 or fp16' in lib.dbsr_last_error()
    x, cv, fl, out = _fake_args(L, L.DBSR_F16)
    bad_out = L.Tensor(1 << 22, L.DBSR_F16, 16 * 16 * 2, 2, 0, L.FrameMap(1, 1, 0, 1))
    assert lib.dbsr_pwc_refine(2, 16, 16, x, cv, fl, bad_out, None) == -1           # the flow is fp32
    assert b'flow_out' in lib.dbsr_last_error()
    assert lib.dbsr_pwc_refine(2, 16, 16, L.NULL_TENSOR, cv, fl, out, None) == -1
    assert b'null' in lib.dbsr_last_error()
    # refiner 4 as the full dilated 3x3 conv (not its centre tap), and a wrong dilation
    for shapes in ([(128, 128, 3, 2), (128, 128, 3, 4), (128, 96, 3, 8), (96, 64, 3, 16), (64, 32, 3, 1), (32, 2, 3, 1)],
                   [(128, 128, 3, 2), (128, 128, 3, 2), (128, 96, 3, 8), (96, 64, 1, 1), (64, 32, 3, 1), (32, 2, 3, 1)]):
        x, cv, fl, out = _fake_args(L, L.DBSR_BF16, shapes)
        assert lib.dbsr_pwc_refine(2, 16, 16, x, cv, fl, out, None) == -1
        assert b'pwc_refine: conv' in lib.dbsr_last_error()
