import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)
GOLDEN = os.path.join(REPO, 'tests', 'golden')


def pytest_configure(config):
    config.addinivalue_line('markers', 'gpu: needs an MI355X (HIP) device and the built libdbsr_hip.so')


@pytest.fixture(scope='session')
def golden():
    """golden(name): the arrays of fixture `name`, stored as tests/golden/name.npz or, above the size limit for a
    committed file, as name.part*.npz (tests/golden/npz_parts.py)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('golden_npz_parts', os.path.join(GOLDEN, 'npz_parts.py'))
    parts = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(parts)

    def load(name):
        return parts.load(GOLDEN, name)
    return load


@pytest.fixture(scope='session')
def synth_sd():
    """Seeded synthetic weights (seed 0) for the default_synthetic architecture, as torch CPU fp32."""
    import torch
    import dbsr_amd
    from dbsr_amd import arch
    from dbsr_amd.weights import generate_state_dict
    net = dbsr_amd.dbsrnet_cvpr2021(**dbsr_amd.DBSR_SYNTHETIC_KWARGS)
    sd = generate_state_dict(arch.state_dict_shapes(net), seed=0)
    return {k: torch.from_numpy(v) for k, v in sd.items()}
