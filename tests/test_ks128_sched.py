"""Host-side checks of the 128 -> 128 weight-stationary kernel's tile and row bookkeeping (csrc/ks128_sched.hpp, the
constexpr functions the kernel's unrolled stream is generated from and the launch checks): tools/ks128_sched_check.cpp
is built as a stand-alone program with the host address and undefined-behaviour sanitizers and replays one tile --
DMA placement, fragment reads, the row-rolling MFMA order, the lane-pair swap -- against a direct convolution.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'deep-rawburst-sr_amd', 'csrc')
SRC = os.path.join(REPO, 'tools', 'ks128_sched_check.cpp')


def _cxx():
    for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('c++'), shutil.which('g++'), shutil.which('clang++')):
        if c and os.path.exists(c):
            return c
    raise AssertionError('no host C++ compiler')


def _build(tmp_path, flags):
    exe = str(tmp_path / 'ks128_sched_check')
    r = subprocess.run([_cxx(), '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I', CSRC, SRC, '-o', exe] + flags,
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('ks128')
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
    assert 'ks128 schedule ok: 120 reads, 288 MFMAs' in r.stdout


def test_schedule_constants():
    """The figures DESIGN.md (4) quotes, read from the header the kernel is built from."""
    txt = open(os.path.join(CSRC, 'ks128_sched.hpp')).read()
    for needle in ('constexpr int TW = 16, TH = 8;', 'constexpr int NW = 8;', 'constexpr int NBUF = 2;',
                   'static_assert(schedule_ok()', 'static_assert(gather_ok()', 'static_assert(swizzle_ok()'):
        assert needle in txt, needle
    # the old K-split body's experiment macros are gone from the sources
    for f in os.listdir(CSRC):
        if f.endswith(('.hip', '.hpp')):
            src = open(os.path.join(CSRC, f)).read()
            assert 'DBSR_KS_ABL' not in src and 'DBSR_KS_NB' not in src and 'DBSR_KS_RING' not in src, f
