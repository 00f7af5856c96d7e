"""CPU-only checks of the objective C ABI (csrc/objective.hip; exports added under ABI 23): the exports exist, bad
arguments are refused with DBSR_E_ARG and a message before any launch, and the Python surface refuses host tensors
and what the trainer cannot combine (the ops are HIP kernels: there is no torch fall-back)."""
import ctypes
import os
import re

import pytest

NEW = ['dbsr_objective_workspace_bytes', 'dbsr_objective_step', 'dbsr_objective_forward', 'dbsr_psnr_from_stats',
       'dbsr_relu_grad_scaled']
P = 1 << 20                                          # a fake, 16-B aligned device address: nothing is launched


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


def test_metric_codes_match_header(L):
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dbsr_hip.h')).read()
    vals = {k.lower(): int(v) for k, v in re.findall(r'DBSR_METRIC_([A-Z0-9_]+) = (\d+)', hdr)}
    assert vals == L.METRIC_CODES


def test_workspace_bytes(L):
    lib = L.lib()
    assert lib.dbsr_objective_workspace_bytes(0, 8, 8) == 0 and lib.dbsr_objective_workspace_bytes(1, 0, 8) == 0
    small, big = lib.dbsr_objective_workspace_bytes(1, 9, 9), lib.dbsr_objective_workspace_bytes(3, 75, 90)
    assert 0 < small < big and small % 16 == 0 and big % 16 == 0


def _desc(L, ptr=P, ld=8, dtype=None, c0=0):
    return L.Tensor(ptr, L.DBSR_F16 if dtype is None else dtype, 100 * 100 * ld, ld, c0, L.FrameMap(1, 1, 0, 1))


def test_step_rejects_bad_arguments(L):
    lib = L.lib()
    need = lib.dbsr_objective_workspace_bytes(1, 100, 100)

    def run(B=1, H=100, W=100, bi=40, metric=0, pred=P, gt=P, gextra=None, state=None, dpre=None, loss=P, stats=P,
            ws=P, wsb=need):
        return lib.dbsr_objective_step(B, H, W, bi, metric, 1.0, pred, gt, gextra, state, dpre or _desc(L), loss, stats,
                                       ws, wsb, None)

    for kw in (dict(pred=None), dict(gt=None), dict(loss=None), dict(stats=None), dict(ws=None),
               dict(dpre=_desc(L, ptr=None))):
        assert run(**kw) == -1, kw
        assert b'objective_step: null pointer' in lib.dbsr_last_error()
    for metric in (-1, 4, 99):
        assert run(metric=metric) == -1
        assert b'unknown metric code' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(H=80), dict(W=80), dict(bi=-1), dict(dpre=_desc(L, ld=2)), dict(dpre=_desc(L, c0=6))):
        assert run(**kw) == -1, kw
        assert b'objective_step: bad sizes' in lib.dbsr_last_error()
    assert run(wsb=need - 1) == -1 and b'workspace' in lib.dbsr_last_error()          # short workspace
    assert run(ws=P + 8) == -1 and b'workspace' in lib.dbsr_last_error()              # not 16-B aligned
    # misaligned dpre: the 16-bit ld 8 layout stores 16 B per pixel; the generic one stores elements
    assert run(dpre=_desc(L, ptr=P + 8)) == -1 and b'misaligned' in lib.dbsr_last_error()
    assert run(dpre=_desc(L, ptr=P + 1, ld=16)) == -1 and b'misaligned' in lib.dbsr_last_error()
    assert run(dpre=_desc(L, ptr=P + 2, ld=8, dtype=L.DBSR_F32)) == -1 and b'misaligned' in lib.dbsr_last_error()
    assert run(dpre=_desc(L, dtype=7)) == -1 and b'unsupported dtype' in lib.dbsr_last_error()


def test_forward_rejects_bad_arguments(L):
    lib = L.lib()
    need = lib.dbsr_objective_workspace_bytes(2, 37, 29)

    def run(B=2, H=37, W=29, bi=3, metric=0, pred=P, gt=P, valid=None, g=P, loss=P, stats=P, ws=P, wsb=need):
        return lib.dbsr_objective_forward(B, H, W, bi, metric, 1.0, pred, gt, valid, g, loss, stats, ws, wsb, None)

    for kw in (dict(pred=None), dict(gt=None), dict(loss=None), dict(stats=None), dict(ws=None)):
        assert run(**kw) == -1, kw
        assert b'objective_forward: null pointer' in lib.dbsr_last_error()
    assert run(metric=5) == -1 and b'unknown metric code' in lib.dbsr_last_error()
    for name in ('l2_sqrt', 'charbonnier'):                                # the reference cannot mask these either
        assert run(metric=L.METRIC_CODES[name], valid=P) == -1
        assert b'a mask goes with l1 and l2 only' in lib.dbsr_last_error()
    for kw in (dict(B=0), dict(H=6), dict(W=6), dict(bi=-2)):
        assert run(**kw) == -1, kw
        assert b'objective_forward: bad sizes' in lib.dbsr_last_error()
    assert run(wsb=need - 16) == -1 and b'workspace' in lib.dbsr_last_error()


def test_psnr_and_gate_reject_bad_arguments(L):
    lib = L.lib()
    assert lib.dbsr_psnr_from_stats(2, None, 0, 1.0, None, P, None, None) == -1
    assert b'psnr_from_stats: null pointer' in lib.dbsr_last_error()
    assert lib.dbsr_psnr_from_stats(2, P, 0, 1.0, None, None, None, None) == -1
    assert lib.dbsr_psnr_from_stats(0, P, 0, 1.0, None, P, None, None) == -1
    assert b'B must be > 0' in lib.dbsr_last_error()
    assert lib.dbsr_psnr_from_stats(2, P, 0, 0.0, None, P, None, None) == -1
    assert b'max_value must be > 0' in lib.dbsr_last_error()
    for kw in (dict(pred=None), dict(gout=None), dict(state=None), dict(dpre=_desc(L, ptr=None))):
        a = dict(pred=P, gout=P, state=P, dpre=_desc(L))
        a.update(kw)
        assert lib.dbsr_relu_grad_scaled(1, 3, 100, 100, a['pred'], a['gout'], a['state'], a['dpre'], None) == -1, kw
        assert b'relu_grad_scaled: null pointer' in lib.dbsr_last_error()
    assert lib.dbsr_relu_grad_scaled(1, 9, 100, 100, P, P, P, _desc(L), None) == -1
    assert b'relu_grad_scaled: bad sizes' in lib.dbsr_last_error()


def test_python_surface_refuses_cpu_tensors():
    """Host tensors are an error, never a launch on a host pointer or a silent torch fall-back."""
    import torch
    from dbsr_amd import ops
    a, b = torch.rand(1, 3, 16, 16), torch.rand(1, 3, 16, 16)
    st = torch.zeros(8, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.objective_step(a, b, 2, 'l2')
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.objective_forward(a, b, 2, 'charbonnier')
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.psnr_from_stats(torch.zeros(1, 2, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='HIP device'):
        ops.relu_grad_scaled(a, b, st, torch.zeros(1, 16, 16, 8))


def test_trainer_signature_and_refusals():
    import inspect
    from dbsr_amd.training import DBSRRealWorldTrainer, DBSRTrainer
    assert inspect.signature(DBSRTrainer.__init__).parameters['objective'].default is None
    assert isinstance(DBSRTrainer.last_stats, property)

    class Net:                                       # refused before anything touches the network
        compute_dtype = None

    with pytest.raises(ValueError, match='objective= belongs to DBSRTrainer'):
        DBSRRealWorldTrainer(Net(), None, objective='l2')
