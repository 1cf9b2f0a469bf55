"""The blob-shift probe of the far-position tests, one definition (tests/test_gpu_far_positions.py,
tests/test_gpu_diversity_limits.py): tests/stream_rules_probe.cpp compiled against csrc/opv_stream_rules.h moves every absolute
index of an exported stream's carry forward by a constant, so that a stream reaches symbol 2^32 in milliseconds. A test module
imports the fixture by name, like those of tests/fixtures.py."""
import ctypes as C
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "opv-cxx-demod_amd" / "csrc"


@pytest.fixture(scope="module")
def probe(tmp_path_factory):
    so = tmp_path_factory.mktemp("far") / "libprobe.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-ffp-contract=off", "-shared", "-I", str(CSRC), "-o", str(so),
                    str(ROOT / "tests" / "stream_rules_probe.cpp"), str(CSRC / "opv_stream_rules.cpp")], check=True)
    L = C.CDLL(str(so))
    L.probe_blob_shift.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint64]
    L.probe_offset.restype = C.c_long
    L.probe_offset.argtypes = [C.c_char_p]
    return L


def shifted_blob(probe, blob, d_sym, d_samp):
    buf = (C.c_char * len(blob)).from_buffer_copy(bytes(blob))
    rc = probe.probe_blob_shift(buf, len(blob), d_sym, d_samp)
    return rc, bytes(buf.raw)
