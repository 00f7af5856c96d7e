"""CPU-only checks of the SSIM metric's C ABI (csrc/metrics.hip; exports added under ABI 23): the exports exist,
the workspace query answers, and bad arguments are refused with DBSR_E_ARG and a message before any launch."""
import ctypes

import pytest

NEW = ['dbsr_ssim_workspace_bytes', 'dbsr_ssim_forward', 'dbsr_ssim_backward']


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


def test_workspace_query(L):
    ws = L.lib().dbsr_ssim_workspace_bytes
    # two floats per (image, channel, 32 x 32 tile of the [H - 2 bi - 10, W - 2 bi - 10] map)
    assert ws(1, 3, 640, 640, 40) == 3 * 18 * 18 * 8                           # the BurstSR scoring shape: 550^2 map
    assert ws(12, 3, 640, 640, 40) == 12 * ws(1, 3, 640, 640, 40)
    assert ws(1, 1, 11, 11, 0) == 8 and ws(2, 4, 43, 43, 0) == 2 * 4 * 4 * 8     # 1 x 1 map; 33 x 33 map: 2 x 2 tiles
    assert ws(1, 3, 31, 31, 10) == 3 * 8 and ws(1, 3, 30, 31, 10) == 0
    assert ws(0, 3, 64, 64, 0) == 0 and ws(1, 5, 64, 64, 0) == 0 and ws(1, 3, 64, 64, -1) == 0
    assert ws(1 << 11, 1, 1 << 10, 1 << 10, 0) == 0                             # B C H W >= 2^31


def test_forward_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20                                          # a fake device address: nothing is launched
    need = lib.dbsr_ssim_workspace_bytes(1, 3, 100, 100, 40)
    assert need > 0

    def fwd(B=1, C=3, H=100, W=100, bi=40, pred=P, gt=P, valid=P, vr=1.0, smap=P, sums=P, result=P, ws=P, wsb=need):
        return lib.dbsr_ssim_forward(B, C, H, W, bi, pred, gt, valid, vr, smap, sums, result, ws, wsb, None)

    for kw in (dict(pred=None), dict(gt=None), dict(sums=None), dict(result=None)):
        assert fwd(**kw) == -1, kw
        assert b'ssim_forward: null pointer' in lib.dbsr_last_error()
    for kw in (dict(C=0), dict(C=5)):
        assert fwd(**kw) == -1, kw
        assert b'ssim_forward: C =' in lib.dbsr_last_error()
    for kw in (dict(H=90), dict(W=90), dict(H=90, W=200), dict(bi=45)):          # the crop must hold one 11 x 11 window
        assert fwd(**kw) == -1, kw
        assert b'smaller than the 11 x 11 window' in lib.dbsr_last_error()
    assert fwd(bi=-1) == -1 and b'boundary_ignore' in lib.dbsr_last_error()
    for vr in (0.0, -1.0):
        assert fwd(vr=vr) == -1 and b'val_range' in lib.dbsr_last_error()
    assert fwd(ws=None) == -1 and b'workspace' in lib.dbsr_last_error()
    assert fwd(wsb=need - 4) == -1 and b'workspace' in lib.dbsr_last_error()
    assert fwd(B=1 << 11, C=1, H=1 << 10, W=1 << 10, bi=0) == -1
    assert b'2^31' in lib.dbsr_last_error()
    assert fwd(B=0) == -1 and b'bad sizes' in lib.dbsr_last_error()


def test_backward_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20

    def bwd(B=1, C=3, H=100, W=100, bi=40, pred=P, gt=P, valid=P, vr=1.0, scale=P, gpred=P):
        return lib.dbsr_ssim_backward(B, C, H, W, bi, pred, gt, valid, vr, scale, gpred, None, 0, None)

    for kw in (dict(pred=None), dict(gt=None), dict(scale=None), dict(gpred=None)):
        assert bwd(**kw) == -1, kw
        assert b'ssim_backward: null pointer' in lib.dbsr_last_error()
    for kw in (dict(C=0), dict(C=5)):
        assert bwd(**kw) == -1 and b'ssim_backward: C =' in lib.dbsr_last_error()
    for kw in (dict(H=90), dict(W=90), dict(bi=45)):
        assert bwd(**kw) == -1 and b'smaller than the 11 x 11 window' in lib.dbsr_last_error()
    assert bwd(bi=-1) == -1 and b'boundary_ignore' in lib.dbsr_last_error()
    assert bwd(vr=0.0) == -1 and b'val_range' in lib.dbsr_last_error()
    assert bwd(B=1 << 11, C=1, H=1 << 10, W=1 << 10, bi=0) == -1 and b'2^31' in lib.dbsr_last_error()


def test_python_surface_refuses_cpu_tensors():
    """ops.ssim* are the HIP kernels: host tensors are an error, never a silent torch fall-back."""
    import torch
    from dbsr_amd import ops
    x = torch.rand(1, 3, 16, 16)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.ssim_forward(x, x)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.ssim_backward(x, x)
