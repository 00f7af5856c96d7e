"""dbsr_conv2d's dispatch, pinned (host logic only, no GPU): for every descriptor of the synthetic grid of
tests/golden/make_golden_conv_dispatch.py the library's host queries -- dbsr_conv_kernel_for,
dbsr_conv_dispatch_variant, dbsr_conv_workspace_bytes, dbsr_conv_lane_reach (which 0, 1, 2), dbsr_conv_head_ok --
answer exactly what tests/golden/conv_dispatch.npz recorded.  The queries read the plan dbsr_conv2d launches
(csrc/conv2d.hip: conv_plan), so a change of any kernel's, tile's or K split's choice shows here."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


@pytest.fixture(scope='module')
def grid():
    spec = importlib.util.spec_from_file_location('make_golden_conv_dispatch',
                                                  os.path.join(GOLDEN, 'make_golden_conv_dispatch.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_conv_dispatch_table(grid, golden):
    from dbsr_amd import _lib as L
    want = golden('conv_dispatch')
    rows, out = grid.table(L)
    assert np.array_equal(rows, want['rows']), 'the grid changed: regenerate the table at the commit it pins'
    grid.check_coverage(rows, want['out'])
    bad = np.nonzero((out != want['out']).any(axis=1))[0]
    report = ['%s: %s, recorded %s' % (dict(zip(grid.COLS, rows[i].tolist())), dict(zip(grid.OUT, out[i].tolist())),
                                       want['out'][i].tolist()) for i in bad[:10]]
    assert bad.size == 0, '%d of %d descriptors differ:\n%s' % (bad.size, len(rows), '\n'.join(report))
