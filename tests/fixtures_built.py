"""The `amd` fixture of the modules that build the library themselves (load(); build()): the CPU-only host tests,
tests/test_gpu_tx_bank.py and tests/test_gpu_tx_bank_limits.py. The variant that only opens the library is in tests/fixtures.py; both are module-scoped and imported by name."""
import pytest

from amd_lib import load


@pytest.fixture(scope="module")
def amd():
    m = load()
    m.build()
    return m
