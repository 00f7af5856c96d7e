"""CPU-only checks of the flow-gradient C ABI (csrc/flow_grad.hip; exports added under ABI 23): the exports exist,
every bad argument is refused with DBSR_E_ARG and a message before any launch, and the Python surface refuses host
tensors and has the new keyword arguments."""
import ctypes

import pytest

NEW = ['dbsr_warp_flow_backward', 'dbsr_backwarp_backward', 'dbsr_offsets_export']
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


def test_warp_flow_backward_rejects_bad_arguments(L):
    lib = L.lib()

    def run(n=2, h=3, w=4, c=16, feat=None, dout=None, flow=P, fis=24, dflow=P, dis=24, acc=0):
        return lib.dbsr_warp_flow_backward(n, h, w, c, feat or _t(L), dout or _t(L), flow, fis, dflow, dis, acc, None)

    for kw in (dict(feat=_t(L, ptr=None)), dict(dout=_t(L, ptr=None)), dict(flow=None), dict(dflow=None),
               dict(feat=_t(L, fpg=0))):
        assert run(**kw) == -1, kw
        assert b'warp_flow_backward: null' in lib.dbsr_last_error()
    for kw in (dict(dout=_t(L, dtype=L.DBSR_F16)), dict(feat=_t(L, dtype=L.DBSR_F32)),
               dict(feat=_t(L, dtype=7), dout=_t(L, dtype=7))):
        assert run(**kw) == -1, kw
        assert b'dtype' in lib.dbsr_last_error()
    for kw in (dict(n=0), dict(h=0), dict(w=-1), dict(c=0), dict(c=-8)):
        assert run(**kw) == -1, kw
        assert b'must be > 0' in lib.dbsr_last_error()
    for c in (4, 12, 15):
        assert run(c=c) == -1 and b'c must be a multiple of 8' in lib.dbsr_last_error()
    # ld or c0 off 16 bytes
    for kw in (dict(feat=_t(L, ld=20)), dict(dout=_t(L, ld=20)), dict(feat=_t(L, ld=24, c0=4)),
               dict(dout=_t(L, ld=24, c0=2))):
        assert run(**kw) == -1, kw
        assert b'ld/c0 must be multiples of 8' in lib.dbsr_last_error()
    # the slice leaves the pixel
    assert run(feat=_t(L, ld=16, c0=8)) == -1 and b'exceeds ld' in lib.dbsr_last_error()
    assert run(c=24) == -1 and b'exceeds ld' in lib.dbsr_last_error()
    # image strides shorter than the two planes
    assert run(fis=23) == -1 and b'image strides' in lib.dbsr_last_error()
    assert run(dis=12) == -1 and b'image strides' in lib.dbsr_last_error()


def test_backwarp_backward_rejects_bad_arguments(L):
    lib = L.lib()
    f32 = L.DBSR_F32

    def run(n=2, h=3, w=4, c=16, inp=None, flow=None, scale=1.0, dout=None, din=None, dflow=None):
        return lib.dbsr_backwarp_backward(n, h, w, c, inp or _t(L), flow or _t(L, dtype=f32, ld=2), scale,
                                          dout or _t(L), din if din is not None else _t(L, dtype=f32),
                                          dflow if dflow is not None else _t(L, dtype=f32, ld=2), None)

    assert run(din=L.NULL_TENSOR, dflow=L.NULL_TENSOR) == -1
    assert b'din and dflow are both null' in lib.dbsr_last_error()
    for kw in (dict(flow=_t(L, ptr=None, dtype=f32, ld=2)), dict(dout=_t(L, ptr=None))):
        assert run(**kw) == -1, kw
        assert b'backwarp_backward: null' in lib.dbsr_last_error()
    for kw in (dict(flow=_t(L, ld=2)), dict(dout=_t(L, dtype=9))):
        assert run(**kw) == -1, kw
        assert b'flow is f32' in lib.dbsr_last_error()
    for kw in (dict(n=0), dict(h=-2), dict(w=0), dict(c=0)):
        assert run(**kw) == -1, kw
        assert b'must be > 0' in lib.dbsr_last_error()
    assert run(flow=_t(L, dtype=f32, ld=1)) == -1 and b'slice exceeds ld' in lib.dbsr_last_error()
    assert run(c=24) == -1 and b'slice exceeds ld' in lib.dbsr_last_error()
    # dflow needs the forward's input, in dout's dtype; outputs are fp32
    assert run(inp=_t(L, ptr=None)) == -1 and b'needs the forward' in lib.dbsr_last_error()
    assert run(inp=_t(L, dtype=L.DBSR_F16)) == -1 and b'needs the forward' in lib.dbsr_last_error()
    assert run(dflow=_t(L, ld=2)) == -1 and b'dflow is an f32' in lib.dbsr_last_error()
    assert run(dflow=_t(L, dtype=f32, ld=1)) == -1 and b'dflow is an f32' in lib.dbsr_last_error()
    assert run(din=_t(L)) == -1 and b'din is an f32' in lib.dbsr_last_error()
    assert run(din=_t(L, dtype=f32, ld=8)) == -1 and b'din is an f32' in lib.dbsr_last_error()


def test_offsets_export_rejects_bad_arguments(L):
    lib = L.lib()

    def run(B=1, N=3, H=3, W=4, flow=P, fis=24, offs=P, modulo=1.0, om=None):
        return lib.dbsr_offsets_export(B, N, H, W, flow, fis, offs, modulo, om if om is not None else _t(L, ld=8), None)

    assert run(flow=None) == -1 and b'offsets_export: null flow' in lib.dbsr_last_error()
    assert run(offs=None, om=L.NULL_TENSOR) == -1 and b'nothing to write' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(N=1), dict(H=0), dict(W=-3)):
        assert run(**kw) == -1, kw
        assert b'offsets_export: B, H, W > 0 and N > 1' in lib.dbsr_last_error()
    assert run(fis=20) == -1 and b'image stride' in lib.dbsr_last_error()
    for om in (_t(L, ld=1), _t(L, ld=8, c0=7), _t(L, ld=8, fpg=0), _t(L, ld=8, dtype=5)):
        assert run(om=om) == -1 and b'bad offs_mod' in lib.dbsr_last_error()


def test_python_surface():
    """Host tensors are an error (no torch fall-back); the new keyword arguments exist with the old defaults."""
    import inspect
    import torch
    from dbsr_amd import ops
    from dbsr_amd.dbsrnet import DBSRNet
    from dbsr_amd.training import DBSRRealWorldTrainer, DBSRTrainer, train_forward
    x, fl = torch.zeros(1, 8, 4, 4), torch.zeros(1, 2, 4, 4)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.warp_flow_backward(x, x, fl)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.backwarp_backward(x, fl, x)
    assert inspect.signature(DBSRTrainer.__init__).parameters['flow_grad'].default is False
    for cls in (DBSRTrainer, DBSRRealWorldTrainer):
        for fn in (cls.step, cls.forward_backward):
            assert inspect.signature(fn).parameters['flow'].default is None
    assert inspect.signature(DBSRTrainer.forward_saved).parameters['flow'].default is None
    assert inspect.signature(train_forward).parameters['flow'].default is None
    assert inspect.signature(DBSRNet.forward).parameters['flow'].default is None
    assert callable(DBSRTrainer.flow_grad)


def test_eval_mode_refuses_external_flow():
    """The inference engine takes no external flows: eval-mode forward(flow=...) names the training forward."""
    import torch
    import dbsr_amd
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS).eval()
    with pytest.raises(NotImplementedError, match='DBSRTrainer.forward_saved'):
        net(torch.zeros(1, 3, 4, 8, 8), flow=torch.zeros(1, 2, 2, 8, 8))
