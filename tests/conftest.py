import glob
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "differentiable-ilqr_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an MI355X (runs through the HIP C-ABI library)")
    config.addinivalue_line("markers", "slow: long CPU case")


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    cache = {}

    def load(name):
        # name.npz plus name.part1.npz, ...: a set above 1 MiB is stored in parts (gen_golden.py save)
        if name not in cache:
            cache[name] = {}
            for path in [os.path.join(GOLDEN, name + ".npz")] + sorted(
                    glob.glob(os.path.join(GOLDEN, name + ".part*.npz"))):
                cache[name].update(np.load(path))
        return cache[name]

    return load
