"""CPU-only checks of the LPIPS kernels' C ABI (csrc/lpips.hip; exports added under ABI 23): the exports exist, the
workspace query answers, and bad arguments are refused with DBSR_E_ARG and a message before any launch."""
import ctypes

import pytest

NEW = ['dbsr_lpips_prep', 'dbsr_maxpool2d', 'dbsr_lpips_layer_workspace_bytes', 'dbsr_lpips_layer']


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
    ws = L.lib().dbsr_lpips_layer_workspace_bytes
    # one float per (image, block of 32 pixel pairs)
    assert ws(1, 75, 75, 64) == 176 * 4                    # alex tap 0 of the 304 x 304 scoring crop: 5625 pixels
    assert ws(8, 75, 75, 64) == 8 * ws(1, 75, 75, 64)
    assert ws(1, 1, 1, 512) == 4 and ws(3, 4, 8, 128) == 3 * 4 and ws(1, 3, 11, 192) == 2 * 4
    assert ws(1, 304, 304, 64) == 2888 * 4                 # vgg tap 0 of the same crop
    for c in (64, 128, 192, 256, 384, 512):
        assert ws(2, 5, 7, c) == 2 * 2 * 4
    for c in (0, 3, 32, 96, 320, 448, 576, 1024):
        assert ws(2, 5, 7, c) == 0
    assert ws(0, 5, 7, 64) == 0 and ws(1, 0, 7, 64) == 0 and ws(1, 5, -1, 64) == 0
    assert ws(1, 1 << 11, 1 << 11, 256) == 0               # 2 B h w C >= 2^31
    assert ws(1, 1 << 11, 1 << 10, 256) > 0


def test_prep_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20                                            # a fake device address: nothing is launched

    def prep(B=1, H=100, W=100, bi=20, net=0, flip=0, norm=0, pred=P, gt=P, out=P):
        return lib.dbsr_lpips_prep(B, H, W, bi, net, flip, norm, pred, gt, out, None)

    for kw in (dict(pred=None), dict(gt=None), dict(out=None)):
        assert prep(**kw) == -1, kw
        assert b'lpips_prep: null pointer' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-3)):
        assert prep(**kw) == -1 and b'bad sizes' in lib.dbsr_last_error()
    for net in (-1, 2):
        assert prep(net=net) == -1 and b'net must be' in lib.dbsr_last_error()
    assert prep(bi=-1) == -1 and b'boundary_ignore' in lib.dbsr_last_error()
    for kw in (dict(H=70), dict(W=70), dict(bi=35), dict(H=30, W=30, bi=0)):   # alex needs a 31 x 31 crop
        assert prep(**kw) == -1, kw
        assert b'smaller than 31 x 31 (alex)' in lib.dbsr_last_error()
    for kw in (dict(H=55, net=1), dict(bi=43, net=1), dict(H=15, W=16, bi=0, net=1)):   # vgg a 16 x 16 one
        assert prep(**kw) == -1, kw
        assert b'smaller than 16 x 16 (vgg)' in lib.dbsr_last_error()
    assert prep(B=1 << 10, H=1 << 10, W=1 << 10, bi=0) == -1 and b'2^31' in lib.dbsr_last_error()
    assert prep(B=150, H=1 << 10, W=1 << 10, bi=0) == -1 and b'2^31' in lib.dbsr_last_error()   # the 8-channel output


def test_maxpool_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20

    def pool(N=2, H=8, W=11, C=64, k=3, s=2, x=P, ldx=64, y=P, ldy=64):
        return lib.dbsr_maxpool2d(N, H, W, C, k, s, x, ldx, y, ldy, None)

    for kw in (dict(x=None), dict(y=None)):
        assert pool(**kw) == -1 and b'maxpool2d: null pointer' in lib.dbsr_last_error()
    for kw in (dict(N=0), dict(H=0), dict(C=0)):
        assert pool(**kw) == -1 and b'bad sizes' in lib.dbsr_last_error()
    for kw in (dict(C=62, ldx=62, ldy=62), dict(ldx=66), dict(ldy=70), dict(ldx=60), dict(ldy=32)):
        assert pool(**kw) == -1, kw
        assert b'multiples of 4' in lib.dbsr_last_error()
    for kw in (dict(k=0), dict(k=9), dict(s=0), dict(s=9)):
        assert pool(**kw) == -1 and b'window' in lib.dbsr_last_error()
    for kw in (dict(H=2), dict(W=2)):
        assert pool(**kw) == -1 and b'smaller than the 3 x 3 window' in lib.dbsr_last_error()
    assert pool(N=1 << 10, H=1 << 10, W=1 << 10, C=4, ldx=4, ldy=4) == -1 and b'2^31' in lib.dbsr_last_error()


def test_layer_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20
    need = lib.dbsr_lpips_layer_workspace_bytes(2, 18, 11, 192)
    assert need == 2 * 7 * 4

    def layer(B=2, h=18, w=11, C=192, layer=1, feat=P, lin=P, dmap=P, per_layer=P, value=P, ws=P, wsb=need):
        return lib.dbsr_lpips_layer(B, h, w, C, layer, feat, lin, dmap, per_layer, value, ws, wsb, None)

    for kw in (dict(feat=None), dict(lin=None), dict(per_layer=None), dict(value=None)):
        assert layer(**kw) == -1, kw
        assert b'lpips_layer: null pointer' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(h=0), dict(w=-1)):
        assert layer(**kw) == -1 and b'bad sizes' in lib.dbsr_last_error()
    for c in (0, 32, 96, 200, 1024):
        assert layer(C=c) == -1 and b'lpips_layer: C =' in lib.dbsr_last_error()
    for lay in (-1, 5):
        assert layer(layer=lay) == -1 and b'layer =' in lib.dbsr_last_error()
    assert layer(ws=None) == -1 and b'workspace' in lib.dbsr_last_error()
    assert layer(wsb=need - 4) == -1 and b'workspace' in lib.dbsr_last_error()
    assert layer(B=1, h=1 << 11, w=1 << 11, C=256, wsb=1 << 30) == -1 and b'2^31' in lib.dbsr_last_error()


def test_python_surface_refuses_cpu_tensors():
    """ops.lpips_* and the plan are the HIP kernels: host tensors are an error, never a silent torch fall-back."""
    import torch
    from dbsr_amd import evaluation as ev, ops
    x = torch.rand(1, 3, 40, 40)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.lpips_prep(x, x)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.maxpool2d(torch.rand(1, 5, 5, 64), 3, 2)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.lpips_layer(torch.rand(2, 3, 3, 64), torch.rand(64))
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.LPIPSPlan(ev.load_lpips_weights(ev.generate_lpips_state_dict('alex'), 'alex'))
