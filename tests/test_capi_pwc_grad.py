"""CPU-only checks of the PWC-Net training C ABI (csrc/pwc_grad.hip; exports added under ABI 23): the exports exist,
every bad argument is refused with DBSR_E_ARG and a message before any launch (the device addresses are fake), and
the Python surface has the new attribute, constructor behaviour and keyword."""
import ctypes

import pytest

NEW = ['dbsr_conv_wgrad_sd_workspace_bytes', 'dbsr_conv_wgrad_sd', 'dbsr_dgrad_sd_packed_elems', 'dbsr_dgrad_sd_pack',
       'dbsr_conv_dgrad_sd', 'dbsr_act_backward', 'dbsr_flow_finalize_backward']
P = 1 << 20                                          # a fake device address: nothing is launched


@pytest.fixture(scope='module')
def L():
    from dbsr_amd import _lib
    _lib.lib()
    return _lib


def test_exports_and_abi(L):
    raw = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert hasattr(raw, name), name
        assert name in L.EXPORTED
    assert L.ABI_VERSION == 23 and L.lib().dbsr_abi_version() == 23            # exports only: the ABI stays


def _t(L, ptr=P, dtype=None, ld=16, c0=0, fpg=1, hw=12):
    return L.Tensor(ptr, L.DBSR_BF16 if dtype is None else dtype, hw * ld, ld, c0, L.FrameMap(fpg, 1, 0, 1))


def _refused(lib, rc, *needles):
    msg = lib.dbsr_last_error()
    assert rc == -1, (rc, msg)
    assert any(n in msg for n in needles), msg


# the conv family's argument errors, shared by wgrad_sd and dgrad_sd: (keyword overrides, message fragment)
CONV_BAD = [
    (dict(n=0), b'must be > 0'), (dict(in_h=0), b'must be > 0'), (dict(in_w=-1), b'must be > 0'),
    (dict(cin=0), b'must be > 0'), (dict(cout=-3), b'must be > 0'), (dict(out_h=0), b'must be > 0'),
    (dict(k=2), b'not in {1, 3, 4}'), (dict(k=5), b'not in {1, 3, 4}'), (dict(k=0), b'not in {1, 3, 4}'),
    (dict(s=3), b'not in {1, 2}'), (dict(s=0), b'not in {1, 2}'),
    (dict(d=0), b'dilation must be'), (dict(pad=-1), b'dilation must be'),
    # 5 x 7 through k3 s2 p1 is 3 x 4
    (dict(out_h=2), b"is not the conv's output"), (dict(out_w=3), b"is not the conv's output"),
    (dict(in_h=6, out_h=4), b"is not the conv's output"), (dict(s=1), b"is not the conv's output"),
    (dict(in_h=1, in_w=1, d=4, pad=0, out_h=1, out_w=1), b"is not the conv's output"),
]


def test_wgrad_sd_rejects_bad_arguments(L):
    lib = L.lib()

    def run(n=2, in_h=5, in_w=7, x=None, cin=16, out_h=3, out_w=4, dy=None, cout=16, k=3, s=2, d=1, pad=1, dw=P, db=P,
            acc=0, ws=P, wsb=None):
        need = lib.dbsr_conv_wgrad_sd_workspace_bytes(n, out_h, out_w, cin, cout, k)
        return lib.dbsr_conv_wgrad_sd(n, in_h, in_w, x or _t(L), cin, out_h, out_w, dy or _t(L), cout, k, s, d, pad, dw,
                                      db, acc, ws, need if wsb is None else wsb, None)

    for kw in (dict(dw=None), dict(ws=None)):
        _refused(lib, run(**kw), b'null')
    for kw in (dict(x=_t(L, ptr=None)), dict(dy=_t(L, ptr=None)), dict(x=_t(L, fpg=0))):
        _refused(lib, run(**kw), b'is null')
    for kw in (dict(x=_t(L, dtype=L.DBSR_F16)), dict(dy=_t(L, dtype=L.DBSR_F32)), dict(x=_t(L, dtype=7), dy=_t(L, dtype=7))):
        _refused(lib, run(**kw), b'dtype')
    for kw, msg in CONV_BAD:
        _refused(lib, run(**kw), msg)
    # ld or c0 off 16 bytes (8 elements in 16 bit, 4 in fp32)
    for kw in (dict(x=_t(L, ld=20)), dict(dy=_t(L, ld=20)), dict(x=_t(L, ld=24, c0=4)), dict(dy=_t(L, ld=24, c0=2)),
               dict(x=_t(L, dtype=L.DBSR_F32, ld=18), dy=_t(L, dtype=L.DBSR_F32))):
        _refused(lib, run(**kw), b'multiples of 16 bytes')
    # the slice leaves the pixel
    _refused(lib, run(x=_t(L, ld=16, c0=8)), b'leave the pixel')
    _refused(lib, run(cout=17), b'leave the pixel')
    _refused(lib, run(cin=24), b'leave the pixel')
    # a short or misaligned workspace
    need = lib.dbsr_conv_wgrad_sd_workspace_bytes(2, 3, 4, 16, 16, 3)
    assert need > 0
    _refused(lib, run(wsb=need - 1), b'needed')
    _refused(lib, run(wsb=0), b'needed')
    _refused(lib, run(ws=P + 4), b'16-byte aligned')
    assert lib.dbsr_conv_wgrad_sd_workspace_bytes(2, 3, 4, 16, 16, 2) == 0
    assert lib.dbsr_conv_wgrad_sd_workspace_bytes(0, 3, 4, 16, 16, 3) == 0


def test_dgrad_sd_rejects_bad_arguments(L):
    lib = L.lib()

    def run(n=2, in_h=5, in_w=7, dx=None, cin=16, out_h=3, out_w=4, dy=None, cout=16, k=3, s=2, d=1, pad=1, wp=P):
        return lib.dbsr_conv_dgrad_sd(n, in_h, in_w, dx or _t(L), cin, out_h, out_w, dy or _t(L), cout, k, s, d, pad, wp,
                                      None)

    _refused(lib, run(wp=None), b'null w_packed')
    _refused(lib, run(wp=P + 8), b'16-byte aligned')
    for kw in (dict(dx=_t(L, ptr=None)), dict(dy=_t(L, ptr=None)), dict(dy=_t(L, fpg=0))):
        _refused(lib, run(**kw), b'is null')
    for kw in (dict(dx=_t(L, dtype=L.DBSR_F16)), dict(dy=_t(L, dtype=L.DBSR_F32)), dict(dx=_t(L, dtype=9), dy=_t(L, dtype=9))):
        _refused(lib, run(**kw), b'dtype')
    for kw, msg in CONV_BAD:
        _refused(lib, run(**kw), msg)
    for kw in (dict(dx=_t(L, ld=20)), dict(dy=_t(L, ld=12)), dict(dx=_t(L, ld=24, c0=4))):
        _refused(lib, run(**kw), b'multiples of 16 bytes')
    _refused(lib, run(dx=_t(L, ld=16, c0=8)), b'leave the pixel')
    _refused(lib, run(cout=20), b'leave the pixel')
    # the pack entry point
    assert lib.dbsr_dgrad_sd_packed_elems(16, 3, 3) == 9 * 16 * 32
    assert lib.dbsr_dgrad_sd_packed_elems(16, 3, 2) == 0
    _refused(lib, lib.dbsr_dgrad_sd_pack(None, 16, 3, 3, L.DBSR_BF16, P, None), b'null')
    _refused(lib, lib.dbsr_dgrad_sd_pack(P, 16, 3, 3, L.DBSR_BF16, None, None), b'null')
    _refused(lib, lib.dbsr_dgrad_sd_pack(P, 0, 3, 3, L.DBSR_BF16, P, None), b'must be > 0')
    _refused(lib, lib.dbsr_dgrad_sd_pack(P, 16, 3, 2, L.DBSR_BF16, P, None), b'not in {1, 3, 4}')
    _refused(lib, lib.dbsr_dgrad_sd_pack(P, 16, 3, 3, 5, P, None), b'dtype')


def test_act_backward_rejects_bad_arguments(L):
    lib = L.lib()

    def run(n=2, hw=12, c=16, act=None, dy=None, y=None, dpre=None):
        return lib.dbsr_act_backward(n, hw, c, L.ACT_LRELU if act is None else act, dy or _t(L), y or _t(L),
                                     dpre or _t(L), None)

    for kw in (dict(n=0), dict(hw=0), dict(c=-8)):
        _refused(lib, run(**kw), b'must be > 0')
    for act in (L.ACT_NONE, 3, -1):
        _refused(lib, run(act=act), b'neither ReLU nor LeakyReLU')
    for kw in (dict(dy=_t(L, ptr=None)), dict(y=_t(L, ptr=None)), dict(dpre=_t(L, ptr=None)), dict(y=_t(L, fpg=0))):
        _refused(lib, run(**kw), b'is null')
    for kw in (dict(dy=_t(L, dtype=L.DBSR_F16)), dict(y=_t(L, dtype=L.DBSR_F32)), dict(dpre=_t(L, dtype=L.DBSR_F16))):
        _refused(lib, run(**kw), b'dtype')
    for kw in (dict(dy=_t(L, ld=20)), dict(dpre=_t(L, ld=24, c0=4))):
        _refused(lib, run(**kw), b'multiples of 16 bytes')
    _refused(lib, run(c=17), b'leave the pixel')
    _refused(lib, run(y=_t(L, ld=16, c0=8)), b'leave the pixel')
    # fp32: 16 bytes are 4 channels, a thread owns 8
    f = L.DBSR_F32
    _refused(lib, run(c=12, dy=_t(L, dtype=f, ld=12), y=_t(L, dtype=f, ld=12), dpre=_t(L, dtype=f, ld=12)),
             b'rounded up to 8 leave the pixel')


def test_flow_finalize_backward_rejects_bad_arguments(L):
    lib = L.lib()
    f = L.DBSR_F32

    def run(Pn=2, hf=4, wf=4, H=8, W=12, Hp=16, Wp=16, doff=P, dflow=None):
        return lib.dbsr_flow_finalize_backward(Pn, hf, wf, H, W, Hp, Wp, doff, dflow or _t(L, dtype=f, ld=2), None)

    _refused(lib, run(doff=None), b'null')
    _refused(lib, run(dflow=_t(L, ptr=None, dtype=f, ld=2)), b'null')
    _refused(lib, run(dflow=_t(L, ld=2)), b'must be f32')
    for kw in (dict(Pn=0), dict(hf=0), dict(wf=-1), dict(H=0), dict(W=0), dict(Hp=0), dict(Wp=-64)):
        _refused(lib, run(**kw), b'must be > 0')
    _refused(lib, run(dflow=_t(L, dtype=f, ld=1)), b'leave the pixel')
    _refused(lib, run(dflow=_t(L, dtype=f, ld=4, c0=3)), b'leave the pixel')


def test_python_surface():
    """PWCNet.differentiable defaults to False and follows train_alignmentnet; the trainer has the new keyword; the
    new operators refuse host tensors."""
    import inspect
    import torch
    import dbsr_amd
    from dbsr_amd import torch_ops
    from dbsr_amd.pwcnet import PWCNet
    from dbsr_amd.training import DBSRTrainer
    assert PWCNet(load_pretrained=False).differentiable is False
    kw = dbsr_amd.DBSR_SYNTHETIC_KWARGS
    assert dbsr_amd.dbsrnet_cvpr2021(**kw).encoder.alignment_net.differentiable is False
    assert dbsr_amd.dbsrnet_cvpr2021(**dict(kw, train_alignmentnet=True)).encoder.alignment_net.differentiable is True
    assert inspect.signature(DBSRTrainer.__init__).parameters['alignment_grad'].default is False
    ops = torch_ops.load()
    x, w = torch.zeros(1, 8, 4, 4), torch.zeros(8, 8, 3, 3)
    refused = (RuntimeError, NotImplementedError)
    with pytest.raises(refused):
        ops.conv2d_backward(x, x, w, x, 1, 1, 1, 0, True, True, True)
    with pytest.raises(refused):
        ops.conv_transpose2d_k4s2(x, torch.zeros(8, 2, 4, 4), None)
    with pytest.raises(refused):
        ops.conv_transpose2d_k4s2_backward(torch.zeros(1, 2, 8, 8), x, torch.zeros(8, 2, 4, 4), True, True, True)
    with pytest.raises(refused):
        ops.flow_finalize(torch.zeros(1, 2, 4, 4), 8, 8)
    with pytest.raises(refused):
        ops.flow_finalize_backward(torch.zeros(1, 2, 8, 8), 4, 4)
    with pytest.raises(refused):
        ops.resize_bilinear(x, 8, 8)


def test_differentiable_pwc_is_fp32_only():
    """compute_dtype != float32 on the differentiable path raises before any kernel runs."""
    import torch
    from dbsr_amd.pwcnet import PWCNet
    net = PWCNet(load_pretrained=False).train()
    net.differentiable = True
    net.compute_dtype = torch.bfloat16
    x = torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match='float32 only'):
        net(x, x)
