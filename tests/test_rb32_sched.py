"""Host-side checks of the fused 32-channel ResBlock kernel's row-rolling body (csrc/rb32_sched.hpp, the constexpr
functions the kernel's unrolled streams are generated from): tools/rb32_sched_check.cpp is built as a stand-alone
program with the host address and undefined-behaviour sanitizers and replays one tile -- DMA placement, both convs'
fragment reads, the row-rolling MFMA order, the epilogue positions -- against a scalar ResBlock.  No GPU."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'deep-rawburst-sr_amd', 'csrc')
SRC = os.path.join(REPO, 'tools', 'rb32_sched_check.cpp')


def _cxx():
    for c in ('/opt/rocm/lib/llvm/bin/clang++', shutil.which('c++'), shutil.which('g++'), shutil.which('clang++')):
        if c and os.path.exists(c):
            return c
    raise AssertionError('no host C++ compiler')


def _build(tmp_path, flags):
    exe = str(tmp_path / 'rb32_sched_check')
    r = subprocess.run([_cxx(), '-std=c++17', '-O1', '-g', '-Wall', '-Werror', '-I', CSRC, SRC, '-o', exe] + flags,
                       capture_output=True, text=True)
    return exe, r


@pytest.fixture(scope='module')
def program(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('rb32_rows')
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
    # per wave: conv1 reads + conv2 items / conv1 MFMAs + conv2 MFMAs; the batch body read 85 for 162
    for frame in ('frame 32x16 tile (0, 0)', 'frame 96x48 tile (32, 16)'):
        line = [ln for ln in r.stdout.splitlines() if frame in ln]
        assert len(line) == 1, r.stdout
        for w in range(4):
            assert ' w%d 21+22/90+72' % w in line[0], line[0]
        for w in (4, 5, 6):
            assert ' w%d 27+22/90+72' % w in line[0], line[0]
        assert ' w7 18+22/72+72' in line[0], line[0]
    assert 'rb32 rows: at most 49 LDS reads for 162 MFMAs per wave per tile' in r.stdout
    assert 'rb32 rows schedule ok' in r.stdout


def test_schedule_header():
    """The kernel is generated from the checked header, and the header checks itself at compile time."""
    txt = open(os.path.join(CSRC, 'rb32_sched.hpp')).read()
    for needle in ('static_assert(Rows<5>::schedule_ok() && Rows<4>::schedule_ok()',
                   'static_assert(conv1_ok()', 'static_assert(Conv2::schedule_ok()'):
        assert needle in txt, needle
    src = open(os.path.join(CSRC, 'conv2d.hip')).read()
    assert 'using namespace rb32;' in src and 'DBSR_VM_WAIT(STORES)' in src
    assert 'using S = Rows<NR>;' in src and 'using S = Conv2;' in src
