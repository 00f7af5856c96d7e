"""CPU-only checks of the real-world objective's C ABI (ABI 23, csrc/sca_train.hip): the exports exist, the
workspace query answers, and bad arguments are refused with DBSR_E_ARG and a message before any launch."""
import ctypes

import pytest

NEW = ['dbsr_aligned_l1_workspace_bytes', 'dbsr_aligned_l1_forward', 'dbsr_aligned_l1_backward']


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
    assert L.ABI_VERSION == 23 and L.lib().dbsr_abi_version() == 23


def test_workspace_query(L):
    ws = L.lib().dbsr_aligned_l1_workspace_bytes
    # backward: 3 fp32 planes per image; forward: ceil(B H W / 256) blocks x (1 + 2 slots) floats (2 slots once
    # an image has >= 256 pixels) -- the larger of the two
    assert ws(12, 448, 448) == 12 * 3 * 448 * 448 * 4
    assert ws(1, 128, 128) == 3 * 128 * 128 * 4
    assert ws(4, 3, 3) == 4 * 3 * 9 * 4                 # tiny images (one block spans all four): still the planes
    assert ws(0, 8, 8) == 0 and ws(1, -1, 8) == 0
    assert ws(1 << 11, 1 << 10, 1 << 10) == 0           # B H W >= 2^31: refused by both entry points


def test_forward_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20                                          # a fake device address: nothing is launched
    need = lib.dbsr_aligned_l1_workspace_bytes(1, 100, 100)

    def fwd(B=1, H=100, W=100, bi=40, pred=P, flow=P, cmat=P, valid=P, gt=P, g=P, loss=P, stats=P, ws=P, wsb=need):
        return lib.dbsr_aligned_l1_forward(B, H, W, bi, pred, flow, cmat, valid, gt, 10.0, g, loss, stats, ws, wsb, None)

    for kw in (dict(pred=None), dict(gt=None), dict(g=None), dict(loss=None), dict(ws=None)):
        assert fwd(**kw) == -1, kw
        assert b'aligned_l1_forward: null pointer' in lib.dbsr_last_error()
    for kw in (dict(H=80), dict(W=80), dict(H=79, W=200), dict(bi=-1), dict(B=0)):      # H, W must exceed 2 bi
        assert fwd(**kw) == -1, kw
        assert b'aligned_l1_forward: bad sizes' in lib.dbsr_last_error()
    assert fwd(wsb=need // 1024) == -1
    assert b'workspace' in lib.dbsr_last_error()
    assert fwd(B=1 << 11, H=1 << 10, W=1 << 10, bi=0) == -1
    assert b'2^31' in lib.dbsr_last_error()


def test_backward_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20
    need = lib.dbsr_aligned_l1_workspace_bytes(1, 100, 100)
    ident = L.FrameMap(1, 1, 0, 1)
    dp = lambda dtype=L.DBSR_BF16, ld=8, c0=0, ptr=P: L.Tensor(ptr, dtype, 100 * 100 * ld, ld, c0, ident)   # noqa: E731

    def bwd(B=1, H=100, W=100, pred=P, flow=P, g=P, cmat=None, scale=P, gpred=P, dpre=None, ws=P, wsb=need):
        return lib.dbsr_aligned_l1_backward(B, H, W, pred, flow, g, cmat, scale, gpred,
                                            dpre if dpre is not None else L.NULL_TENSOR, ws, wsb, None)

    assert bwd(g=None) == -1
    assert b'aligned_l1_backward: null pointer' in lib.dbsr_last_error()
    assert bwd(gpred=None) == -1                                      # neither output requested
    assert b'aligned_l1_backward: null pointer' in lib.dbsr_last_error()
    assert bwd(H=0) == -1
    assert b'bad sizes' in lib.dbsr_last_error()
    assert bwd(gpred=None, dpre=dp(), pred=None) == -1                # the ReLU gate needs pred
    assert b'needs pred' in lib.dbsr_last_error()
    assert bwd(dpre=dp(ld=8, c0=6)) == -1                             # 3 channels do not fit the pixel
    assert b'bad dpre' in lib.dbsr_last_error()
    assert bwd(dpre=dp(dtype=7)) == -1
    assert b'unsupported dtype' in lib.dbsr_last_error()
    assert bwd(ws=None) == -1 and b'workspace' in lib.dbsr_last_error()
    assert bwd(wsb=need - 16) == -1 and b'workspace' in lib.dbsr_last_error()
    assert bwd(ws=P + 4) == -1 and b'16-B aligned' in lib.dbsr_last_error()


def test_color_apply_mask_only_arguments(L):
    """dbsr_color_apply takes test and out both NULL (the mask alone, for the training objective) and refuses one
    without the other."""
    lib = L.lib()
    P = 1 << 20
    assert lib.dbsr_color_apply(1, 16, 16, 5, P, P, P, 20.0, P, 128, 128, 0.125, 0.125, None, P, None) == -1
    assert b'color_apply' in lib.dbsr_last_error()
    assert lib.dbsr_color_apply(1, 16, 16, 5, P, P, P, 20.0, None, 128, 128, 0.125, 0.125, P, P, None) == -1


def test_realworld_surface_refuses_cpu():
    import torch
    import dbsr_amd
    from dbsr_amd.training import DBSRRealWorldTrainer
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    with pytest.raises(RuntimeError, match='HIP device'):
        DBSRRealWorldTrainer(net, dbsr_amd.PWCNet(load_pretrained=False))
    from dbsr_amd import burstsr
    assert burstsr.PixelWiseError(metric='l1', boundary_ignore=40).boundary_ignore == 40
    with pytest.raises(NotImplementedError, match='HIP'):
        burstsr.SpatialColorAlignment(None)(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 1, 4, 1, 1))
