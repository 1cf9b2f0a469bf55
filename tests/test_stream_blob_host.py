"""CPU-only: opv_blob_streams reads a blob's header on the host - no device is needed, and anything that is not a blob of this
build is OPV_EINVAL (the device half of stream migration is tests/test_gpu_stream_migration.py)."""
import numpy as np
import pytest

from fixtures_built import amd  # noqa: F401

EINVAL = -1


def test_blob_streams_refuses_what_is_not_a_blob_without_a_device(amd):
    L = amd.lib()
    assert L.opv_blob_streams(None, 0) == EINVAL
    assert L.opv_blob_streams(None, 4096) == EINVAL
    junk = np.random.default_rng(20261017).integers(0, 256, 4096, dtype=np.uint8)
    assert L.opv_blob_streams(junk.ctypes.data, 0) == EINVAL
    assert L.opv_blob_streams(junk.ctypes.data, junk.size) == EINVAL
    assert "magic" in L.opv_last_error().decode()
    for blob in (None, b"", junk, bytes(junk[:7])):
        with pytest.raises(amd.OpvError):
            amd.blob_streams(blob)
    # the right magic in front of junk is still refused: every header field has to match this build
    junk[:8] = np.frombuffer(b"OPVBLOB1", np.uint8)
    assert L.opv_blob_streams(junk.ctypes.data, junk.size) == EINVAL
