"""The GPU tests of the objectives (csrc/objective.hip, dbsr_amd.objectives, DBSRTrainer(objective=...)), run in a
process of their own.

The cases are tests/gpu_objective_cases.py (its docstring states the oracles and the bounds).  They are not collected
into the suite's process: one child `pytest` runs that file once, and every test here reports the cases of one of its
test functions from the child's JUnit record (outcome, message and what the case printed: the measured figures).

Why: tests/test_gpu_ssim.py's 1x1x75x90 case runs torch's own convolution backward on the device, and that backward
has ended in a GPU fault or an abort when GPU tests that allocate device memory were added ahead of it in the same
process ('MS-SSIM', 'Not built'; 'Objectives on the fused step', 'Tests').  No kernel of this package is in
flight there; what the earlier tests change is where torch's allocator places that test's tensors.  The cause inside
torch's backward is not known, so these tests leave the suite's process exactly as the parent's suite leaves it: they
allocate nothing in it."""
import ast
import os
import subprocess
import sys
import xml.etree.ElementTree as ET

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CASES = os.path.join(HERE, 'gpu_objective_cases.py')

NAMES = ['test_step_vs_fixture', 'test_step_16bit_dpre_within_one_ulp', 'test_l1_bitwise_equals_l1_loss_backward',
         'test_two_runs_bitwise_equal', 'test_l2_sqrt_zero_distance_pixel_is_zero', 'test_psnr_vs_fixture_and_drop_rule',
         'test_module_autograd_vs_fixture', 'test_relu_grad_scaled', 'test_trainer_l1_objective_is_todays_plan',
         'test_trainer_metric_grads_vs_oracle', 'test_trainer_extra_callable_matches_builtin',
         'test_trainer_ssim_term_graph_equals_eager', 'test_trainer_fp16_lpips_extra_step',
         'test_trainer_fp16_overflow_step_is_skipped', 'test_trainer_refusals',
         'test_two_ranks_charbonnier_equal_one_process']


def test_case_list_is_complete():
    """Every test function of the cases file is reported by a test of this file (CPU: reads the source)."""
    tree = ast.parse(open(CASES).read())
    found = [n.name for n in tree.body if isinstance(n, ast.FunctionDef) and n.name.startswith('test_')]
    assert found == NAMES


@pytest.fixture(scope='module')
def child(tmp_path_factory):
    """{test function: [(case id, outcome, text)]} of one child pytest over the cases file, and its console output."""
    xml = str(tmp_path_factory.mktemp('objective') / 'cases.xml')
    cmd = [sys.executable] + (['-s'] if sys.flags.no_user_site else []) + \
        ['-m', 'pytest', '-q', '-m', 'gpu', '-p', 'no:cacheprovider', '-o', 'junit_logging=system-out',
         '--junitxml', xml, CASES]
    run = subprocess.run(cmd, cwd=REPO, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    res = {}
    if os.path.exists(xml):
        for tc in ET.parse(xml).getroot().iter('testcase'):
            name = tc.get('name')
            outcome, text = 'passed', ''
            for el in tc:
                if el.tag in ('failure', 'error', 'skipped'):
                    outcome = el.tag
                    text += (el.get('message') or '') + '\n' + (el.text or '') + '\n'
                elif el.tag == 'system-out':
                    text += el.text or ''
            res.setdefault(name.split('[')[0], []).append((name, outcome, text))
    return res, 'child pytest exit %d\n%s' % (run.returncode, run.stdout[-4000:])


@pytest.mark.gpu
@pytest.mark.parametrize('name', NAMES)
def test_objective(child, name):
    res, console = child
    cases = res.get(name)
    assert cases, 'the cases of %s did not run\n%s' % (name, console)
    for case, outcome, text in cases:
        print('%s: %s\n%s' % (case, outcome, text))
    bad = [(case, outcome) for case, outcome, _ in cases if outcome != 'passed']
    assert not bad, bad
