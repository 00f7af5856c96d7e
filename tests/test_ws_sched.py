"""Host-side checks of the weight-stationary kernel's row-rolling body (csrc/ws_sched.hpp, the constexpr functions the
kernel's unrolled stream is generated from): tools/ws_sched_check.cpp is built as a stand-alone program with the host
address and undefined-behaviour sanitizers and replays one tile of each instantiated shape -- DMA placement, fragment
reads, the row-rolling MFMA order, the side-work positions -- against a direct convolution.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'deep-rawburst-sr_amd', 'csrc')
SRC = os.path.join(REPO, 'tools', 'ws_sched_check.cpp')


def _cxx():
    for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('c++'), shutil.which('g++'), shutil.which('clang++')):
        if c and os.path.exists(c):
            return c
    raise AssertionError('no host C++ compiler')


def _build(tmp_path, flags):
    exe = str(tmp_path / 'ws_sched_check')
    r = subprocess.run([_cxx(), '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I', CSRC, SRC, '-o', exe] + flags,
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ws_rows')
    exe, r = _build(tmp, ['-fsanitize=address,undefined', '-fno-sanitize-recover=all'])
    sanitized = r.returncode == 0
    if not sanitized:                     # a toolchain without the sanitizer runtimes: the same checks, plain
        exe, r = _build(tmp, [])
    assert r.returncode == 0, r.stderr
    return exe, sanitized


def test_schedule_replay(program):
    exe, _ = program
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    # half the tile body's 72 reads per wave at cin 64
    assert 'ws rows 16x16 nch 2: 36 reads, 144 MFMAs per wave per tile' in r.stdout
    assert 'ws rows 16x16 nch 1: 18 reads, 72 MFMAs per wave per tile' in r.stdout
    assert 'ws rows 16x8 nch 2: 24 reads, 72 MFMAs per wave per tile' in r.stdout
    assert 'ws rows schedule ok' in r.stdout


def test_schedule_header():
    """The kernel is generated from the checked header, and the header checks itself at compile time."""
    txt = open(os.path.join(CSRC, 'ws_sched.hpp')).read()
    for needle in ('static_assert(Sched<16, 2>::schedule_ok() && Sched<16, 1>::schedule_ok() && Sched<8, 2>::schedule_ok()',
                   'static_assert(Sched<16, 2>::READS == 36 && Sched<16, 2>::MFMAS == 144'):
        assert needle in txt, needle
    src = open(os.path.join(CSRC, 'conv2d.hip')).read()
    assert 'using S = wsr::Sched<TH, NCH>;' in src and 'DBSR_VM_WAIT(S::STORES)' in src
