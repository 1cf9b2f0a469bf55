"""CPU-only: csrc/opv_frame_code.h - the frame code that the host modulator, the device modulator, the decoder and the link report
share (randomiser table, interleaver address, code polynomials, 3-bit quantiser) - compiled with g++ into a shared object
(tests/frame_code_probe.cpp gives it a C face) and held against the oracle through ctypes. Every check is exact."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

import soft_log_inputs as S
from amd_lib import load

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "opv-cxx-demod_amd" / "csrc"
FB, CODED = 134, 2144


@pytest.fixture(scope="module")
def code(tmp_path_factory):
    so = tmp_path_factory.mktemp("frame_code") / "libframecode.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-ffp-contract=off", "-shared", "-I", str(CSRC), "-o", str(so),
                    str(ROOT / "tests" / "frame_code_probe.cpp")], check=True)
    L = ctypes.CDLL(str(so))
    L.probe_lfsr_table.argtypes = [ctypes.c_void_p]
    L.probe_interleave_addr.restype = ctypes.c_uint32
    L.probe_interleave_addr.argtypes = [ctypes.c_uint32]
    L.probe_encode_frame.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    L.probe_quantise_payload.restype = ctypes.c_int
    L.probe_quantise_payload.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return L


def test_randomiser_table_is_the_oracles(code, oracle):
    t = np.zeros(FB, np.uint8)
    code.probe_lfsr_table(t.ctypes.data)
    assert np.array_equal(t, oracle.lfsr_table())


def test_address_map_is_the_oracles_permutation(code, oracle):
    got = np.array([code.probe_interleave_addr(i) for i in range(CODED)], np.uint16)
    assert np.array_equal(got, oracle.deinterleave_perm())
    assert np.array_equal(np.sort(got), np.arange(CODED))


def test_three_frames_encode_like_the_oracle_and_the_host_modulator(code, oracle):
    amd = load()                                                         # (the library build() made: opv_tap_tx_frame)
    for f in (np.zeros(FB, np.uint8), np.full(FB, 0xFF, np.uint8), oracle.bert_frames(1, first=5)[0]):
        f = np.ascontiguousarray(f)
        coded, on_air = np.zeros(CODED, np.uint8), np.zeros(CODED, np.uint8)
        code.probe_encode_frame(f.ctypes.data, coded.ctypes.data, on_air.ctypes.data)
        _, tap_coded, tap_on_air = amd.tx_frame_taps(f)
        assert np.array_equal(on_air, oracle.encode_frame(f))
        assert np.array_equal(coded, tap_coded) and np.array_equal(on_air, tap_on_air)


def quantise(code, p):
    p = np.ascontiguousarray(p, np.float64)
    q = np.full(CODED, -1, np.int32)
    return (q if code.probe_quantise_payload(p.ctypes.data, q.ctypes.data) else None)


def test_quantiser_equals_the_oracles_in_every_value(code, oracle):
    """opv_quantise3 behind an index-order mean of |soft| against oracle.frame_decode's q: the decoder's edge payloads (NaN, Inf,
    overflowing sums, every value on a boundary; the ones the oracle drops must be dropped here too) and 200 seeded noisy ones"""
    names, edge = S.decoder_edge_payloads(oracle)
    live = 0
    for name, p in zip(names, edge):
        exp = oracle.frame_decode(p)
        got = quantise(code, p)
        if exp["metric"] < 0:
            assert got is None, name
            continue
        live += 1
        assert got is not None and np.array_equal(got, exp["q"]), (name, int(np.count_nonzero(got != exp["q"])) if got is not None else "dropped")
    assert len(names) == 32 and live == 27
    rng = np.random.default_rng(20260)
    for k in range(200):
        p = S.payload(oracle, k % 50, a=float(rng.choice([0.01, 1.0, 500.0, 3.0e4])), sigma=float(rng.choice([0.0, 60.0, 250.0, 700.0])), rng=rng)
        got = quantise(code, p)
        assert got is not None and np.array_equal(got, oracle.frame_decode(p)["q"]), k
