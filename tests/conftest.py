import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")
    config.addinivalue_line("markers", "slow: long-running test")


def gpu_available():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture
def short_tmp_path():
    """A temporary directory whose path is short enough to hold unix sockets.

    ``sockaddr_un.sun_path`` is 108 bytes; pytest's ``tmp_path`` (base temp +
    ``pytest-of-<user>/pytest-N/<test name>``) plus ``<node>/zygote.sock`` runs
    past that under a deep base temp, and the warm launcher then cannot bind."""
    import pathlib
    import shutil
    import tempfile
    base = tempfile.gettempdir()
    if len(base) > 64:  # + /pdo-t-XXXXXXXX/<node>/zygote.sock must stay under 108
        base = "/tmp"
    d = tempfile.mkdtemp(prefix="pdo-t-", dir=base)
    try:
        yield pathlib.Path(d)
    finally:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch.device("cuda", 0)
