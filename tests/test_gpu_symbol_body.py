"""GPU: the symbol loop of the one-stream-per-wave front end (csrc/k_frontend.hip: symbol_r and the loop nest around it) after its
instruction diet - X[40] handed out from the spare lane of every row, the dominant-tone select fused into DPP, the soft log's offset
advanced once per loop trip with the ring mask at batch boundaries only, the fp64 ring's tap address as one 16-bit multiply-add.
None of these may move a rounding, so:

 1. its three launch shapes - and the four of the several-streams-per-wave kernels, which share their scheduler and symbol tail in
    csrc/k_frontend_rows.h - reproduce, bit for bit, what the PARENT build computed on a fixed capture set (sha256 digests recorded by
    scripts/symbol_body_record.py in tests/golden/symbol_body_parent.json);
 2. the soft ring wraps three times per stream in the middle of demodulate() calls (the smallest ring a context can have, four
    streams whose starts are staggered by 0 .. 3 symbols, fed in odd pieces with frames popped between rounds), held to the oracle
    in full;
 3. the AFC hand-over (X[40] of one symbol into the next symbol's phase detector) at the clamp, under an out-of-range -o, on captures
    of one symbol and across an export / import, held to the oracle per demodulate() call;
 4. the fp64 ring's addressing with the chunk origin past 2^16, 2^21 (oracle and int16 ring) and 2^27 samples (int16 ring).

Bounds: stream_checks.check_stream as it stands (soft symbols < 1e-9 of their mean, decisions and integer columns ==, the chunk
log's float columns 1e-7); against the int16 ring: identity (stream_runs.assert_same)."""
import importlib.util
import json
from concurrent.futures import ProcessPoolExecutor
from functools import partial
from pathlib import Path

import numpy as np
import pytest

from fixtures import amd  # noqa: F401
from oracle_lib import impair
from soak_inputs import host_workers, oracle_receive_job
from stream_checks import check_stream
from stream_runs import CAP_SOFT, CHUNK, SMALL_M, WRAP_PIECES, assert_same, drain, make_demod, new_acc, result, state_tuple

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
GOLDEN = ROOT / "tests" / "golden" / "symbol_body_parent.json"
WG4_S = 516                                   # the first stream counts k_msk_frontend_rb_wg4 serves: 513 ..
WG4_SLOTS = [0, 1, 2, 3, 257, 258, 514, 515]  # every wave of a workgroup, the first, a middle and the last (full) workgroup


def recorder():
    spec = importlib.util.spec_from_file_location("symbol_body_record", ROOT / "scripts" / "symbol_body_record.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


def oracle_all(caps):
    with ProcessPoolExecutor(host_workers()) as pool:
        return list(pool.map(partial(oracle_receive_job, want_soft=True), caps))


def held(amd, got, exp, tag):
    """check_stream in full; a capture too short for a single symbol (check_stream's soft error has nothing to take a maximum of)
    is held to the oracle's chunk log, symbol and frame counts"""
    assert got["state"].stalled == 0, tag
    if exp["n_soft"]:
        return check_stream(amd, got, exp, tag, edge_ties=0, offset_ties=None)
    assert got["state"].total_symbols == 0 and len(got["soft"]) == 0 and len(got["frames"]) == 0 == len(exp["frames"]), tag
    assert got["chunks"].shape == exp["chunks"].shape and np.array_equal(got["chunks"][:, 3:], exp["chunks"][:, 3:]), tag
    assert np.allclose(got["chunks"][:, :3], exp["chunks"][:, :3], rtol=0, atol=1e-7), tag


def context(amd, monkeypatch, shape, n_caps, **kw):
    """-> (context, the stream of capture j, kernel name): a small context on the fp64 or the int16 ring, or 516 streams of which
    WG4_SLOTS carry the captures (the rest stay idle)"""
    if shape == "wg4":
        assert n_caps <= len(WG4_SLOTS)
        return amd.Demod(WG4_S, **kw), WG4_SLOTS[:n_caps], "k_msk_frontend_rb_wg4"
    return make_demod(amd, monkeypatch, shape == "int16", n_caps, **kw), list(range(n_caps)), "k_msk_frontend_rb"


# ------------------------------------------------------------------ 1. equals the parent
@pytest.fixture(scope="module")
def parent_set(amd):
    rec = recorder()
    names, caps = rec.capture_set(amd)
    golden = json.loads(GOLDEN.read_text())
    assert names == golden["names"] and [c.size // 2 for c in caps] == golden["samples"]
    return rec, names, caps, golden


@pytest.mark.parametrize("shape", ["fp64", "int16", "wg4", "x4_wg4", "x16", "x16_wg4", "x16_wg8"])
def test_equals_the_parent(amd, parent_set, shape):
    """every digest of the recorded set on this launch shape: soft log, chunk log, final state (edge_ties included), frames. The
    shapes of the several-streams-per-wave kernels (csrc/k_frontend_x4.hip, k_frontend_x16.hip, recorded on the parent of the commit
    that moved their shared statements into csrc/k_frontend_rows.h): x4_wg4 and x16 carry the 14 captures whole in one context
    (two idle rows / quads), x16_wg4 is 70 streams (two workgroups), x16_wg8 is 16 400 streams attached to the 14 device-resident
    3-frame cuts. Every stream is held to its capture's digest; of x16_wg8's, the ones that are read back: the first and the last
    workgroup and every 64th stream (symbol_body_record.X16_WG8_READ - all 16 400 would not fit a few seconds). record_shape asserts
    frontend_kernel() on every shape."""
    rec, names, caps, golden = parent_set
    assert tuple(golden["shapes"]) == rec.SHAPES
    got = rec.record_shape(amd, names, caps, shape)
    for name, g, e in zip(names, got, golden["shapes"][shape]):
        assert g == e, f"{shape} {name}: {[k for k in e if g[k] != e[k]]} differ from the parent build"
    assert sum(e["n_frames"] for e in golden["shapes"][shape]) >= 25 and any(e["edge_ties"] for e in golden["shapes"][shape])   # not vacuous


# ------------------------------------------------------------------ 2. the soft ring's wrap at every position of a loop trip
# (SMALL_M, CAP_SOFT, WRAP_PIECES: tests/stream_runs.py)
@pytest.fixture(scope="module")
def wrap_set(oracle):
    """four 12-frame captures (16 dB) whose starts are staggered by 0, 1, 2 and 3 symbols, and the oracle's result for each"""
    base = impair(oracle.modulate(oracle.bert_frames(12, "WRAP", first=77)), amp=3000.0, f0_hz=-640.0, ebn0_db=16.0, seed=8101)
    caps = [np.ascontiguousarray(base[2 * 40 * j:]) for j in range(4)]
    exp = oracle_all(caps)
    # Where the wraps fall, from the oracle's per-call symbol counts alone. A -s call is a whole chunk of 86 720 samples whatever the
    # signal's own clock or start, and the timing loop fits 2167 symbols into every one: ring offset 0 is symbol 8192 m - 2167 c of call
    # c = 3, 7, 11, and (that - 1) % 4 = 2 for all three, on every stream - staggered starts do not move it (they were meant to; a
    # residue other than 2 first appears at the fifth wrap, 19 frames in). What the stagger does move is where the front end's batches
    # of symbols (k_frontend.hip: housekeeping, cut by the sample ring's tile events at fixed SAMPLE positions) begin relative to the
    # wrap, which is what decides the wrap's place in a loop trip; that is not computable from the oracle's counts, so it is not asserted.
    for e in exp:
        ends = np.cumsum(e["chunks"][:, 4]).astype(np.int64)
        wraps = list(range(CAP_SOFT, e["n_soft"], CAP_SOFT))
        assert len(wraps) >= 3 and set(int(v) for v in e["chunks"][:-1, 4]) == {2167}
        calls = [int(np.searchsorted(ends, w, side="right")) for w in wraps]
        assert calls == [3, 7, 11] and all(ends[c - 1] < w < ends[c] - 4 for c, w in zip(calls, wraps))   # well inside a call
    return caps, exp


@pytest.mark.parametrize("shape", ["fp64", "int16", "wg4"])
def test_soft_ring_wraps_inside_calls_on_staggered_streams(amd, wrap_set, monkeypatch, shape):
    caps, exp = wrap_set
    d, ks, kernel = context(amd, monkeypatch, shape, 4, max_samples=SMALL_M, streaming=True)
    try:
        n = [c.size // 2 for c in caps]
        at, accs, rounds = [0] * 4, [new_acc() for _ in range(4)], 0
        while min(a - m for a, m in zip(at, n)) < 0 or rounds == 0:
            piece = WRAP_PIECES[rounds % len(WRAP_PIECES)]
            for j, k in enumerate(ks):
                m = min(piece, n[j] - at[j])
                if m > 0:
                    d.push(k, caps[j][2 * at[j]: 2 * (at[j] + m)])
                    at[j] += m
                    if at[j] == n[j]:
                        d.flush(k)
            d.process()
            d.sync()
            assert d.frontend_kernel() == kernel
            for j, k in enumerate(ks):
                st = drain(d, k, accs[j])                       # frames popped, softs and chunk rows tapped, every round
                assert st.stalled == 0, (shape, rounds, j)
            rounds += 1
        assert rounds >= 30
        for j, k in enumerate(ks):
            held(amd, result(amd, d, k, accs[j]), exp[j], f"{shape} wrap stream {j}")
    finally:
        d.close()


# ------------------------------------------------------------------ 3. the AFC hand-over
CUT = 2 * CHUNK + 12345                       # where the migrated stream changes contexts


@pytest.fixture(scope="module")
def afc_set(oracle):
    """[(name, capture, init_offset)] and the oracle's result for each"""
    items = []
    for f0 in (-2000.0, -1500.0, 1500.0, 2000.0):
        x = impair(oracle.modulate(oracle.bert_frames(4, "AFC", first=int(abs(f0)))), amp=2500.0, f0_hz=f0, ebn0_db=16.0, seed=300 + int(f0) % 97)
        assert x.size // 2 >= 3 * CHUNK
        items.append((f"f0{f0:+.0f}", x, None))
    short = impair(oracle.modulate(oracle.bert_frames(1)), amp=4000.0, f0_hz=300.0, ebn0_db=16.0, seed=44)
    items.append(("60_samples", np.ascontiguousarray(short[: 2 * 60]), None))
    items.append(("50_samples", np.ascontiguousarray(short[: 2 * 50]), None))
    items.append(("migrated", impair(oracle.modulate(oracle.bert_frames(4, "MOVE", first=9)), amp=2000.0, f0_hz=1100.0, ebn0_db=15.0, seed=45), None))
    items.append(("-o2500", impair(oracle.modulate(oracle.bert_frames(4, "WIDE", first=5)), amp=2500.0, f0_hz=1800.0, ebn0_db=16.0, seed=46), 2500.0))
    exp = oracle_all([it[1] for it in items[:-1]]) + [oracle.receive(items[-1][1], streaming=True, init_offset=2500.0)]
    assert all(len(e["chunks"]) >= 3 for e in exp[:4]) and exp[4]["n_soft"] <= 1 and exp[5]["n_soft"] == 0
    return items, exp


@pytest.mark.parametrize("shape", ["fp64", "wg4"])
def test_afc_hand_over_per_call(amd, afc_set, monkeypatch, shape):
    """the carry {fo, tf, mu, leftover, nsym} of every demodulate() call (check_stream: integers ==, floats 1e-7) and everything else"""
    items, exp = afc_set
    plain = [j for j, it in enumerate(items) if it[2] is None and it[0] != "migrated"]
    nmax = max(it[1].size // 2 for it in items) + 64
    d, ks, kernel = context(amd, monkeypatch, shape, len(plain) + 1, max_samples=nmax, streaming=True)
    d2, ks2, _ = context(amd, monkeypatch, shape, 1, max_samples=nmax, streaming=True)
    try:
        for j, k in zip(plain, ks):
            d.push(k, items[j][1])
            d.flush(k)
        # the migrated stream: CUT samples here, the rest in the other context
        jm, km = [it[0] for it in items].index("migrated"), ks[len(plain)]
        x, acc = items[jm][1], new_acc()
        d.push(km, x[: 2 * CUT])
        d.process()
        d.sync()
        assert d.frontend_kernel() == kernel
        drain(d, km, acc)
        d2.import_streams([ks2[0]], bytes(d.export_streams([km])))
        d2.push(ks2[0], x[2 * CUT:])
        d2.flush(ks2[0])
        d2.process()
        d2.sync()
        assert d2.frontend_kernel() == kernel
        held(amd, result(amd, d2, ks2[0], acc), exp[jm], f"{shape} migrated")
        for j, k in zip(plain, ks):
            held(amd, result(amd, d, k, new_acc()), exp[j], f"{shape} {items[j][0]}")
    finally:
        d.close()
        d2.close()
    jw = len(items) - 1
    d, ks, kernel = context(amd, monkeypatch, shape, 1, max_samples=nmax, streaming=True, init_offset=2500.0)
    try:
        d.push(ks[0], items[jw][1])
        d.flush(ks[0])
        d.process()
        d.sync()
        assert d.frontend_kernel() == kernel
        held(amd, result(amd, d, ks[0], new_acc()), exp[jw], f"{shape} -o 2500")
    finally:
        d.close()


# ------------------------------------------------------------------ 4. the fp64 ring's addressing
def attached_run(amd, monkeypatch, int16, ptr, n):
    d = make_demod(amd, monkeypatch, int16, 1, max_samples=n + 64, streaming=True)
    try:
        d.attach(0, ptr, n, eof=True)
        d.process()
        d.sync()
        assert d.frontend_kernel() == "k_msk_frontend_rb"
        fr, meta = d.pop_frames(0)
        st = d.state(0)
        assert st.stalled == 0
        return dict(frames=fr, meta=meta, events=d.pop_events(0), soft=d.soft(0), chunks=d.chunks(0), state=st)
    finally:
        d.close()


def identical(a, b, what):
    assert_same(dict(a, state=state_tuple(a["state"])), dict(b, state=state_tuple(b["state"])), what)


@pytest.fixture(scope="module")
def long_capture(oracle):
    x = impair(oracle.modulate(oracle.bert_frames(26, "LONG", first=2)), amp=3500.0, f0_hz=-900.0, ebn0_db=16.0, seed=47)
    assert x.size // 2 > (1 << 21) + 4000 + CHUNK
    return x


def test_fp64_ring_origin_past_2_16_and_2_21(amd, oracle, long_capture, monkeypatch):
    """one stream attached 4000 samples into a resident 26-frame capture: the chunk origin passes 2^16 and 2^21 samples, the 2048-sample
    ring wraps > 1000 times; against the oracle in full and identical to the int16 ring"""
    import torch
    off = 4000
    dev_iq = torch.from_numpy(long_capture).to(torch.device("cuda", 0))
    n = long_capture.size // 2 - off
    ptr = dev_iq.data_ptr() + 4 * off
    assert ptr % 16 == 0
    got = attached_run(amd, monkeypatch, False, ptr, n)
    assert got["state"].chunk_origin > (1 << 21)
    exp = oracle.receive(long_capture[2 * off:], streaming=True)
    check_stream(amd, got, exp, "origin past 2^21", edge_ties=0, offset_ties=None)
    identical(got, attached_run(amd, monkeypatch, True, ptr, n), "origin past 2^21: fp64 ring vs int16 ring")


def test_fp64_ring_origin_past_2_27_equals_int16_ring(amd, long_capture, monkeypatch):
    """the same capture repeated in HBM until the chunk origin passes 2^27 samples (32 x origin leaves 32 bits there): the two rings
    see the same operands, so every record must be identical"""
    import torch
    reps = (1 << 27) // (long_capture.size // 2) + 2
    dev_iq = torch.from_numpy(long_capture).to(torch.device("cuda", 0)).repeat(reps)
    n = dev_iq.numel() // 2
    got = attached_run(amd, monkeypatch, False, dev_iq.data_ptr(), n)
    assert got["state"].chunk_origin > (1 << 27) and len(got["frames"]) >= 10 * reps
    identical(got, attached_run(amd, monkeypatch, True, dev_iq.data_ptr(), n), "origin past 2^27: fp64 ring vs int16 ring")
