"""CPU-only checks of the LPIPS gradient's C ABI (csrc/lpips_grad.hip; exports added under ABI 23): the exports
exist, bad arguments are refused with DBSR_E_ARG and a message before any launch, and the module's new flag changes
nothing on CPU tensors.  None of the three entry points takes a workspace (every output element has one owner), so
there is no workspace query; the plan's gradient buffers are sized in ops.LPIPSPlan._build_backward."""
import ctypes
import inspect

import pytest

NEW = ['dbsr_lpips_layer_backward', 'dbsr_maxpool2d_backward', 'dbsr_lpips_stem_backward']
P = 1 << 20                                                # a fake device address: nothing is launched


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
    # no workspace anywhere in the new calls: the argument lists end with the stream
    assert len(L.lib().dbsr_lpips_layer_backward.argtypes) == 10
    assert len(L.lib().dbsr_maxpool2d_backward.argtypes) == 10
    assert len(L.lib().dbsr_lpips_stem_backward.argtypes) == 11


def test_layer_backward_rejects_bad_arguments(L):
    lib = L.lib()

    def call(B=2, h=18, w=11, C=192, feat=P, lin=P, gvalue=P, gfeat=P, acc=0):
        return lib.dbsr_lpips_layer_backward(B, h, w, C, feat, lin, gvalue, gfeat, acc, None)

    for kw in (dict(feat=None), dict(lin=None), dict(gvalue=None), dict(gfeat=None)):
        assert call(**kw) == -1, kw
        assert b'lpips_layer_backward: null pointer' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(h=0), dict(w=-1)):
        assert call(**kw) == -1 and b'bad sizes' in lib.dbsr_last_error()
    for c in (0, 30, 32, 96, 200, 1024):                   # C % 4 != 0 and multiples of 4 the taps never have
        assert call(C=c) == -1 and b'lpips_layer_backward: C =' in lib.dbsr_last_error()
    assert call(B=1, h=1 << 11, w=1 << 11, C=256) == -1 and b'2^31' in lib.dbsr_last_error()


def test_pool_backward_rejects_bad_arguments(L):
    lib = L.lib()

    def call(N=2, H=8, W=11, C=64, k=3, s=2, x=P, dy=P, dx=P):
        return lib.dbsr_maxpool2d_backward(N, H, W, C, k, s, x, dy, dx, None)

    for kw in (dict(x=None), dict(dy=None), dict(dx=None)):
        assert call(**kw) == -1 and b'maxpool2d_backward: null pointer' in lib.dbsr_last_error()
    for kw in (dict(N=0), dict(H=0), dict(W=-2), dict(C=0)):
        assert call(**kw) == -1 and b'bad sizes' in lib.dbsr_last_error()
    for c in (62, 65, 3):
        assert call(C=c) == -1 and b'a multiple of 4' in lib.dbsr_last_error()
    for k, s in ((0, 2), (1, 1), (2, 1), (3, 1), (3, 3), (4, 2), (5, 2), (3, 0), (2, 4)):    # served: 3 / 2 and 2 / 2
        assert call(k=k, s=s) == -1, (k, s)
        assert b'3 / 2 or 2 / 2' in lib.dbsr_last_error()
    for kw in (dict(H=2), dict(W=2)):
        assert call(**kw) == -1 and b'smaller than the 3 x 3 window' in lib.dbsr_last_error()
    assert call(H=1, k=2) == -1 and b'smaller than the 2 x 2 window' in lib.dbsr_last_error()
    assert call(N=1 << 10, H=1 << 10, W=1 << 10, C=4) == -1 and b'2^31' in lib.dbsr_last_error()


def test_stem_backward_rejects_bad_arguments(L):
    lib = L.lib()

    def call(B=1, H=100, W=100, bi=20, net=0, flip=0, norm=0, dy=P, w=P, gpred=P):
        return lib.dbsr_lpips_stem_backward(B, H, W, bi, net, flip, norm, dy, w, gpred, None)

    for kw in (dict(dy=None), dict(w=None), dict(gpred=None)):
        assert call(**kw) == -1, kw
        assert b'lpips_stem_backward: null pointer' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(H=0), dict(W=-3)):
        assert call(**kw) == -1 and b'bad sizes' in lib.dbsr_last_error()
    for net in (-1, 2):
        assert call(net=net) == -1 and b'net must be' in lib.dbsr_last_error()
    assert call(bi=-1) == -1 and b'boundary_ignore' in lib.dbsr_last_error()
    for kw in (dict(H=70), dict(W=70), dict(bi=35), dict(H=30, W=30, bi=0)):   # alex needs a 31 x 31 crop
        assert call(**kw) == -1, kw
        assert b'smaller than 31 x 31 (alex)' in lib.dbsr_last_error()
    for kw in (dict(H=55, net=1), dict(bi=43, net=1), dict(H=15, W=16, bi=0, net=1)):   # vgg a 16 x 16 one
        assert call(**kw) == -1, kw
        assert b'smaller than 16 x 16 (vgg)' in lib.dbsr_last_error()
    assert call(B=1 << 10, H=1 << 10, W=1 << 10, bi=0) == -1 and b'2^31' in lib.dbsr_last_error()
    # vgg's dy holds 64 channels per pixel: 64 B oh ow passes 2^31 before 3 B H W does
    assert call(B=40, H=1 << 10, W=1 << 10, bi=0, net=1) == -1 and b'64 must be < 2^31' in lib.dbsr_last_error()


def test_python_surface_refuses_cpu_tensors():
    """The new ops are the HIP kernels: host tensors are an error, never a silent torch fall-back."""
    import torch
    from dbsr_amd import ops
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.lpips_layer_backward(torch.rand(2, 3, 3, 64), torch.rand(64))
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.maxpool2d_backward(torch.rand(1, 5, 5, 64), torch.rand(1, 2, 2, 64), 3, 2)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.lpips_stem_backward(torch.rand(1, 16, 16, 64), torch.rand(64, 3, 3, 3), (1, 3, 16, 16), net='vgg')
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.lpips_conv_dgrad(torch.rand(1, 2, 2, 64), torch.rand(64, 64, 3, 3), 1)


def test_differentiable_flag_is_ignored_on_cpu_tensors():
    import torch
    from dbsr_amd import evaluation as ev
    assert inspect.signature(ev.LPIPS.__init__).parameters['differentiable'].default is False
    sd = ev.generate_lpips_state_dict('alex', seed=11)
    gen = torch.Generator().manual_seed(3)
    gt = torch.rand(2, 3, 41, 39, generator=gen)
    pred = (gt + 0.1 * torch.randn(2, 3, 41, 39, generator=gen)).clamp(0, 1)
    for kw in (dict(), dict(per_image=True, bgr2rgb=True, normalize=True)):
        plain = ev.LPIPS(boundary_ignore=4, type='alex', weights=sd, **kw)
        diff = ev.LPIPS(boundary_ignore=4, type='alex', weights=sd, differentiable=True, **kw)
        assert torch.equal(plain(pred, gt), diff(pred, gt))
        a, b = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
        plain(a, gt).sum().backward()
        diff(b, gt).sum().backward()
        assert torch.equal(a.grad, b.grad) and float(a.grad.abs().max()) > 0
