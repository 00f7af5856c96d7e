"""CPU-only checks of the synthetic-data C ABI (csrc/synth_ops.hip; exports added under ABI 23): the exports exist,
and every bad argument is refused with DBSR_E_ARG and a message before anything is launched."""
import ctypes

import pytest

NEW = ['dbsr_unprocess_rgb', 'dbsr_burst_synth', 'dbsr_postprocess_rgb']
P = 1 << 20                                              # a fake device address: nothing is launched


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


def test_unprocess_rejects_bad_arguments(L):
    lib = L.lib()

    def un(B=2, Hc=48, Wc=64, src=P, fmt=0, params=P, lin=P):
        return lib.dbsr_unprocess_rgb(B, Hc, Wc, src, fmt, params, lin, None)

    for kw in (dict(src=None), dict(params=None), dict(lin=None)):
        assert un(**kw) == -1, kw
        assert b'unprocess_rgb: null pointer' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(Hc=0), dict(Wc=-3)):
        assert un(**kw) == -1, kw
        assert b'unprocess_rgb: bad sizes' in lib.dbsr_last_error()
    for fmt in (2, -1):
        assert un(fmt=fmt) == -1 and b'unknown src_format' in lib.dbsr_last_error()
    assert un(B=1 << 10, Hc=1 << 10, Wc=1 << 10) == -1 and b'2^31' in lib.dbsr_last_error()


def test_burst_synth_rejects_bad_arguments(L):
    lib = L.lib()

    def bs(B=2, N=3, Hc=48, Wc=64, bc=4, f=4, lin=P, ainv=P, nl=P, z=P, burst=P, rgb=P, flow=P):
        return lib.dbsr_burst_synth(B, N, Hc, Wc, bc, f, lin, ainv, nl, z, burst, rgb, flow, None)

    for kw in (dict(lin=None), dict(ainv=None), dict(burst=None)):
        assert bs(**kw) == -1, kw
        assert b'burst_synth: null pointer' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(N=0), dict(Hc=0), dict(Wc=-1)):
        assert bs(**kw) == -1, kw
        assert b'burst_synth: bad sizes' in lib.dbsr_last_error()
    for f in (0, -2):
        assert bs(f=f) == -1 and b'must be >= 1' in lib.dbsr_last_error()
    for kw in (dict(bc=24), dict(bc=30), dict(bc=-1), dict(Hc=64, Wc=8, bc=4)):          # 2 bc >= min(Hc, Wc)
        assert bs(**kw) == -1, kw
        assert b'border_crop' in lib.dbsr_last_error()
    for kw in (dict(Hc=50), dict(Wc=66), dict(f=3, Hc=48, Wc=64, bc=4)):                 # not divisible by f
        assert bs(**kw) == -1, kw
        assert b'not divisible' in lib.dbsr_last_error()
    for kw in (dict(Hc=44, Wc=64), dict(Hc=48, Wc=60), dict(f=1, Hc=49, Wc=64, bc=0)):   # odd H2 or W2
        assert bs(**kw) == -1, kw
        assert b'must be even' in lib.dbsr_last_error()
    for kw in (dict(z=None), dict(nl=None)):
        assert bs(**kw) == -1, kw
        assert b'go together' in lib.dbsr_last_error()
    assert bs(B=1 << 10, Hc=1 << 10, Wc=1 << 10, bc=0, f=1) == -1 and b'2^31' in lib.dbsr_last_error()


def test_postprocess_rejects_bad_arguments(L):
    lib = L.lib()

    def pp(B=1, H=24, W=40, img=P, params=P, flags=15, f32=P, u8=P):
        return lib.dbsr_postprocess_rgb(B, H, W, img, params, flags, f32, u8, None)

    for kw in (dict(img=None), dict(params=None)):
        assert pp(**kw) == -1, kw
        assert b'postprocess_rgb: null pointer' in lib.dbsr_last_error()
    assert pp(f32=None, u8=None) == -1 and b'no output' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(H=-1), dict(W=0)):
        assert pp(**kw) == -1, kw
        assert b'postprocess_rgb: bad sizes' in lib.dbsr_last_error()
    for flags in (16, -1):
        assert pp(flags=flags) == -1 and b'flags' in lib.dbsr_last_error()
    assert pp(B=1 << 10, H=1 << 10, W=1 << 10) == -1 and b'2^31' in lib.dbsr_last_error()


def test_python_surface_refuses_cpu_tensors():
    """ops.unprocess_rgb / burst_synth / postprocess_rgb are the HIP kernels: host tensors are an error."""
    import torch
    from dbsr_amd import ops
    x = torch.rand(1, 3, 16, 16)
    p = torch.zeros(1, 16)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.unprocess_rgb(x, p)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.burst_synth(x, torch.zeros(1, 2, 2, 3), 0, 1)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.postprocess_rgb(x, p)
