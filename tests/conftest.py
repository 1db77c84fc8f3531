import os
import sys

import pytest

# The CPU oracle is compared with the reference's fp32 outputs at fp32 rounding: oneDNN must not run its fp32 convolutions and
# matmuls in a reduced-precision math mode (bf16 / tf32) that a machine's environment may select by default.  Set before torch
# initialises oneDNN; the tests' subprocesses (gloo ranks, bench.py) inherit it.
os.environ["ONEDNN_DEFAULT_FPMATH_MODE"] = "STRICT"

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "masked-diffusion-model_amd")
for p in (ROOT, PKG):
    if p not in sys.path:
        sys.path.insert(0, p)

GOLDEN = os.path.join(ROOT, "tests", "golden")


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    # The oracle (torch on the CPU) is the slow side of the long sampler tests.  A GPU box shows all of the host's cores but
    # gives one GPU a 16-core share: torch's default thread count oversubscribes it ~10x (a 250-step oracle run took 25 s there
    # against 2.5 s on 8 threads here).
    import torch
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    torch.set_num_threads(max(1, min(16, n)))


@pytest.fixture(scope="session")
def golden():
    import numpy as np

    def load(name):
        return np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    return load
