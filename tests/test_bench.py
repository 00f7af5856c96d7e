"""bench.py's command line and --dump-outputs writer (CPU side; the GPU legs are run by the benchmark itself)."""
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def bench():
    spec = importlib.util.spec_from_file_location('dbsr_bench', os.path.join(REPO, 'bench.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_outputs_whole_and_sampled(bench, tmp_path):
    """A small output is written whole, one above DUMP_MAX_ELEMS as the same seeded sample in every call; all
    float32 and within 64 MB for the three arrays of a forward."""
    n = bench.DUMP_MAX_ELEMS
    assert 3 * n * 4 <= 64 << 20
    small = torch.arange(24, dtype=torch.float16).reshape(2, 3, 4)
    big = torch.arange(n + 1000, dtype=torch.float32) * 0.5
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), {'small': small, 'big': big})
    a_small, a_big = np.load(tmp_path / 'a' / 'small.npy'), np.load(tmp_path / 'a' / 'big.npy')
    assert a_small.dtype == np.float32 and a_big.dtype == np.float32
    np.testing.assert_array_equal(a_small, np.arange(24, dtype=np.float32).reshape(2, 3, 4))
    assert a_big.shape == (n,)
    np.testing.assert_array_equal(a_big, np.load(tmp_path / 'b' / 'big.npy'))
    # every sampled value is an element of `big`, taken in index order, and the sample reaches across the array
    idx = a_big * 2
    assert np.all(idx == np.round(idx)) and idx.min() >= 0 and idx.max() <= n + 999
    assert np.all(np.diff(idx) >= 0) and idx.min() < 1000 and idx.max() > n - 1000


def test_kernel_breakdown_needs_full():
    out = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--kernel-breakdown'],
                         capture_output=True, text=True, timeout=120, cwd=REPO)
    assert out.returncode == 2 and '--full' in out.stderr
