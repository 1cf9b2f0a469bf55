"""Module-scoped fixtures that most test modules use, written once. A test module imports the ones it needs by name (pytest takes
a fixture from the importing module's namespace), so every module still gets an instance of its own, as when each wrote them out.
`amd` here only opens the library (load(); lib()): for the modules that run on a built tree. tests/fixtures_built.py holds the
variant that builds first."""
import pytest

from amd_lib import load


@pytest.fixture(scope="module")
def amd():
    m = load()
    m.lib()
    return m


@pytest.fixture(scope="module")
def torch_dev():
    import torch
    return torch, torch.device("cuda", 0)
