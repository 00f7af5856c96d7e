"""CPU-only checks of the loss-scaling C ABI (csrc/loss_scale.hip; exports added under ABI 23): the exports exist,
bad arguments are refused with DBSR_E_ARG and a message before any launch, and the Python surface refuses host
tensors (the ops are HIP kernels: there is no torch fall-back)."""
import ctypes

import pytest

NEW = ['dbsr_l1_loss_backward_scaled', 'dbsr_grad_unscale_check', 'dbsr_adam_step_guarded', 'dbsr_loss_scale_update']


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


def test_state_layout_matches_header(L):
    """_lib's word indices are the header's DBSR_LS_* enum."""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dbsr_hip.h')).read()
    vals = {k: int(v) for k, v in re.findall(r'DBSR_LS_([A-Z_]+) = (\d+)', hdr)}
    assert vals == {'SCALE': L.LS_SCALE, 'GROWTH_TRACKER': L.LS_GROWTH_TRACKER, 'FOUND_INF': L.LS_FOUND_INF,
                    'ADAM_STEP': L.LS_ADAM_STEP, 'SKIPPED': L.LS_SKIPPED, 'WORDS': L.LS_WORDS}


def test_l1_scaled_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20                                          # a fake device address: nothing is launched

    def desc(ptr=P, ld=8):
        return L.Tensor(ptr, L.DBSR_F16, 100 * 100 * ld, ld, 0, L.FrameMap(1, 1, 0, 1))

    def run(B=1, C=3, H=100, W=100, bi=40, pred=P, gt=P, state=P, dpre=None, loss=P, ws=P, wsb=4 * 40):
        return lib.dbsr_l1_loss_backward_scaled(B, C, H, W, bi, pred, gt, state, dpre or desc(), loss, ws, wsb, None)

    for kw in (dict(pred=None), dict(gt=None), dict(state=None), dict(loss=None), dict(ws=None),
               dict(dpre=desc(ptr=None))):
        assert run(**kw) == -1, kw
        assert b'l1_loss_backward_scaled: null pointer' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(C=0), dict(H=80), dict(W=80), dict(bi=-1), dict(C=9)):
        assert run(**kw) == -1, kw
        assert b'l1_loss_backward_scaled: bad sizes' in lib.dbsr_last_error()
    assert run(wsb=4 * 39) == -1 and b'workspace' in lib.dbsr_last_error()


def test_unscale_check_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20
    assert lib.dbsr_grad_unscale_check(16, None, P, None) == -1
    assert b'grad_unscale_check: null pointer' in lib.dbsr_last_error()
    assert lib.dbsr_grad_unscale_check(16, P, None, None) == -1
    assert b'grad_unscale_check: null pointer' in lib.dbsr_last_error()
    for n in (0, -5):
        assert lib.dbsr_grad_unscale_check(n, P, P, None) == -1
        assert b'n must be > 0' in lib.dbsr_last_error()
    assert lib.dbsr_grad_unscale_check(16, P + 2, P, None) == -1                  # not a float address
    assert b'4-B aligned' in lib.dbsr_last_error()


def test_adam_guarded_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20

    def run(n=16, p=P, g=P, m=P, v=P, state=P):
        return lib.dbsr_adam_step_guarded(n, p, g, m, v, 1e-4, 0.9, 0.999, 1e-8, 1.0, state, None)

    for kw in (dict(p=None), dict(g=None), dict(m=None), dict(v=None), dict(state=None)):
        assert run(**kw) == -1, kw
        assert b'adam_step_guarded: null pointer' in lib.dbsr_last_error()
    for n in (0, -1):
        assert run(n=n) == -1 and b'n must be > 0' in lib.dbsr_last_error()


def test_update_rejects_bad_arguments(L):
    lib = L.lib()
    P = 1 << 20
    assert lib.dbsr_loss_scale_update(None, 2.0, 0.5, 2000, None) == -1
    assert b'loss_scale_update: null pointer' in lib.dbsr_last_error()
    for g, b in ((0.0, 0.5), (-2.0, 0.5), (2.0, 0.0), (2.0, -0.5), (float('nan'), 0.5)):
        assert lib.dbsr_loss_scale_update(P, g, b, 2000, None) == -1, (g, b)
        assert b'factors must be > 0' in lib.dbsr_last_error()
    for iv in (0, -3):
        assert lib.dbsr_loss_scale_update(P, 2.0, 0.5, iv, None) == -1
        assert b'growth_interval must be >= 1' in lib.dbsr_last_error()


def test_python_surface_refuses_cpu_tensors():
    """Host tensors are an error, never a launch on a host pointer or a silent torch fall-back."""
    import torch
    from dbsr_amd import ops
    st = torch.zeros(8, dtype=torch.int32)
    x = torch.zeros(64)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.grad_unscale_check(x, st)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.adam_step_guarded(x, x.clone(), x.clone(), x.clone(), st)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.loss_scale_update(st)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.l1_loss_backward(torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16), 2, state=st)


def test_trainer_signature():
    """The scaler's constructor arguments, with GradScaler's defaults."""
    import inspect
    from dbsr_amd.training import DBSRTrainer
    p = inspect.signature(DBSRTrainer.__init__).parameters
    assert p['loss_scale'].default is None and p['init_scale'].default == 65536.0
    assert (p['growth_factor'].default, p['backoff_factor'].default, p['growth_interval'].default) == (2.0, 0.5, 2000)
    assert callable(DBSRTrainer.loss_scale_state)
