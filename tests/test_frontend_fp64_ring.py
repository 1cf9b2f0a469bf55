"""GPU: k_msk_frontend_rb's fp64 sample ring (128 threads: a helper wave widens the int16 IQ to fp64 in LDS, automatic while
the context has no more streams than the device has CUs) against its int16 ring (64 threads, forced with the create-time test
hook OPV_FRONTEND_INT16_RING). The interpolation sees the same operands either way, so every result must be identical, bit
for bit: soft symbols, the chunk carry {fo, tf, mu, leftover, nsym}, the stream state (origin included), frames, Viterbi
metrics and tracker events."""
import importlib.util
import sys
from pathlib import Path

import numpy as np
import pytest

from fixtures import amd  # noqa: F401
from stream_runs import CHUNK, assert_same, base_capture, collect_bits, make_demod, state_tuple

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "opv-cxx-demod_amd"


def workload_mod():
    if "workload" not in sys.modules:
        spec = importlib.util.spec_from_file_location("workload", PKG / "workload.py")
        mod = importlib.util.module_from_spec(spec)
        sys.modules["workload"] = mod
        spec.loader.exec_module(mod)
    return sys.modules["workload"]


def run_host(amd, monkeypatch, captures, int16, streaming=True, **kw):
    """one round per context: push + flush every capture, process until no stream is stalled; per-stream results"""
    S = len(captures)
    d = make_demod(amd, monkeypatch, int16, S, max_samples=max(c.size // 2 for c in captures) + 64, streaming=streaming, **kw)
    try:
        out = d.receive(captures)
        name = d.frontend_kernel()
        return [dict(frames=r["frames"], meta=r["meta"], events=r["events"], soft=r["soft"], state=state_tuple(r["state"]),
                     chunks=r["chunks"]) for r in out], name
    finally:
        d.close()


def compare_host(amd, monkeypatch, captures, label, **kw):
    got, name = run_host(amd, monkeypatch, captures, False, **kw)
    exp, name16 = run_host(amd, monkeypatch, captures, True, **kw)
    assert name == name16 == "k_msk_frontend_rb"
    for s in range(len(captures)):
        assert_same(got[s], exp[s], f"{label}: stream {s}")
    return got


def test_fp64_ring_workload_64_streams_bit_identical(amd, monkeypatch):
    """the headline shape at 20 frames: 64 streams of workload.generate at 16 dB, the +/-2 kHz clamp streams included"""
    import torch
    workload = workload_mod()
    F, S = 20, 64
    dev = torch.device("cuda:0")
    n = amd.lib().opv_tx_modulated_samples(F)
    res = {}
    for int16 in (False, True):
        d = make_demod(amd, monkeypatch, int16, S, max_samples=n + 64, streaming=True, device=0)
        try:
            if not res:
                d_iq, tx, n = workload.generate(amd, d, torch, dev, range(S), F, 16.0)
            for k in range(S):
                d.attach(k, d_iq[k].data_ptr(), n, eof=True)
            d.process()
            d.sync()
            assert d.frontend_kernel() == "k_msk_frontend_rb"
            res[int16] = [collect_bits(d, k) for k in range(S)]
            assert all(not r["state"][15] for r in res[int16])   # stalled
        finally:
            d.close()
    for k in range(S):
        assert_same(res[False][k], res[True][k], f"workload stream {k}")
    assert sum(len(r["frames"]) for r in res[False]) > 0


def test_fp64_ring_tiny_captures_and_every_tail(amd, monkeypatch):
    """tails of 1..64 samples behind two whole chunks (streaming), and captures from one sample up, across the ring's and
    the int16 tiles' boundaries"""
    base = base_capture(amd, frames=3, seed=1)
    assert base.size // 2 >= 2 * CHUNK + 64
    tails = [base[: 2 * (2 * CHUNK + t)] for t in range(1, 65)]
    compare_host(amd, monkeypatch, tails, "tail")
    sizes = list(range(1, 12)) + [39, 40, 49, 50, 51, 52, 88, 89, 90, 91, 92, 130, 255, 256, 257, 1000, 2036, 2037, 2047, 2048,
                                  2049, 2105, 4095, 4096, 4097, 6000, 8191, 8192, 8193, CHUNK - 1, CHUNK, CHUNK + 1]
    tiny = [base[: 2 * n] for n in sizes]
    compare_host(amd, monkeypatch, tiny, "tiny")
    compare_host(amd, monkeypatch, tiny[:16] + tiny[-8:], "tiny batch", streaming=False)


def test_fp64_ring_silence_gaps_and_extreme_offsets(amd, monkeypatch):
    base = base_capture(amd, frames=3, seed=2)
    gaps = []
    for k in range(8):
        x = base.reshape(-1, 2).copy()
        rng = np.random.default_rng(10 + k)
        for _ in range(12):                                   # digital silence of 1..3000 samples anywhere
            a = int(rng.integers(0, x.shape[0] - 3000))
            x[a: a + int(rng.integers(1, 3000))] = 0
        gaps.append(x.reshape(-1))
    compare_host(amd, monkeypatch, gaps, "silence gaps")
    for off in (-25000.0, -2500.0, 2001.0, 9000.0):          # -o beyond the +/-2 kHz AFC clamp: the kWide body
        compare_host(amd, monkeypatch, [base, gaps[0]], f"-o {off}", init_offset=off)


def test_fp64_ring_odd_pushes_over_many_calls(amd, monkeypatch):
    """incremental pushes (leftover / origin carried across calls and launches), one round per push"""
    caps = [base_capture(amd, frames=4, seed=20 + s).reshape(-1, 2) for s in range(3)]
    n = min(c.shape[0] for c in caps)
    pieces = [7919, 1, 40, 86719, 3, 20011, 104729, 65537, 2049, 99991]
    res = {}
    for int16 in (False, True):
        d = make_demod(amd, monkeypatch, int16, 3, max_samples=n + 64, streaming=True)
        try:
            rounds, at, p = [], 0, 0
            while at < n:
                m = min(pieces[p % len(pieces)], n - at)
                for s in range(3):
                    d.push(s, caps[s][at: at + m])
                at += m
                p += 1
                if at >= n:
                    for s in range(3):
                        d.flush(s)
                d.process()
                d.sync()
                rounds.append([collect_bits(d, s) for s in range(3)])
            res[int16] = rounds
        finally:
            d.close()
    assert len(res[False]) == len(res[True]) >= 8
    for r, (a, b) in enumerate(zip(res[False], res[True])):
        for s in range(3):
            assert_same(a[s], b[s], f"round {r} stream {s}")


def test_fp64_ring_one_stream_and_256(amd, monkeypatch):
    base = base_capture(amd, frames=3, seed=30)
    compare_host(amd, monkeypatch, [base], "S=1")
    caps = [base_capture(amd, frames=2, seed=100 + s, sigma=200.0 + s) for s in range(256)]
    got = compare_host(amd, monkeypatch, caps, "S=256")
    assert sum(len(r["frames"]) for r in got) >= 256


def test_rb_mapping_names(amd, monkeypatch):
    """the automatic mapping names k_msk_frontend_rb at 1, 64, 256 and 300 streams. The name is the same for the fp64 ring (streams
    <= CUs) and the int16 ring (beyond): both shapes are held to the oracle on either side of that boundary, the int16 ring also
    forced at n_cu streams, by test_gpu_midrange_streams.py::test_every_stream_and_soft_symbol_vs_oracle"""
    iq = base_capture(amd, frames=1, seed=40)[: 2 * 5000]
    for S in (1, 64, 256, 300):
        d = make_demod(amd, monkeypatch, False, S, max_samples=iq.size // 2 + 64, streaming=True)
        try:
            for s in range(S):
                d.push(s, iq)
                d.flush(s)
            d.process()
            d.sync()
            assert d.frontend_kernel() == "k_msk_frontend_rb", S
        finally:
            d.close()
