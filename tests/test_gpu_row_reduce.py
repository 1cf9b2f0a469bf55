"""GPU: the two places where the symbol loop of csrc/k_frontend.hip changed its INSTRUCTIONS and must not change a bit.

 A. the all-reduce over the four DPP rows: two v_mfma_f64_4x4x4 with 0/1 row selectors and an add where two permlane swaps stood.
    Inputs: full-scale captures (the largest row partials: constant +32767, constant -32768, alternating); silence gaps whose edges
    lie 15, 30 and 45 samples into a symbol's 60-sample span, so that one, two or three whole rows of a symbol carry exact zeros
    (the masked terms 0 * r, zero sums, signed-zero angles); a single non-zero sample in each row's sample range (one-tap windows,
    held as that class like tests/test_gpu_symbol_slots.py holds its `single_tap`).
 B. the soft log: in a trip of four, slots 1 and 3 store two values with one 16-byte store. Inputs: calls that start at an even and
    at an odd soft index (the store's address 0 and 8 mod 16), the 8192-symbol ring on four streams staggered by 0 .. 3 symbols with
    frames popped between rounds, last calls of 1 .. 9 symbols, runs of silent symbols that begin at every index mod 4 (a silent
    symbol in every slot of a trip, slots 0 and 1 among them).

Shapes: the fp64 ring, the int16 ring (OPV_FRONTEND_INT16_RING=1) and k_msk_frontend_rb_wg4 (516 streams): identical results.
Bounds: stream_checks.check_stream / stream_runs.check_capture as they stand. And the soft logs' SHA-256, recorded from the parent
commit's library (the permlane-swap tree, one store per symbol) on these inputs on an MI355X: DIGESTS below. No capture is longer
than five -s calls."""
import hashlib
from concurrent.futures import ProcessPoolExecutor
from functools import partial

import numpy as np
import pytest

from fixtures import amd  # noqa: F401
from hostile_inputs import ambiguous
from oracle_lib import impair
from soak_inputs import host_workers, oracle_receive_job
from stream_checks import check_stream
from stream_runs import (CAP_SOFT, CARRY_ATOL, CHUNK, SMALL_M, WRAP_PIECES, assert_same, check_capture, drain, make_demod, new_acc, result,
                         state_tuple)

pytestmark = pytest.mark.gpu
WHOLE = [1 << 30]
WG4_S = 516
WG4_SLOTS = [0, 1, 2, 3, 257, 258, 514, 515]
SHAPES = ["fp64", "int16", "wg4"]
MAX_SAMPLES = 5 * CHUNK

# SHA-256 (first 16 hex digits) of each stream's soft log (float64, little endian), from the parent commit's library
DIGESTS = {
    "full_scale": ["306c18d57c198834", "bb0b8c6a8dfe33a4", "09c8626e0d66899f"],
    "row_gaps": ["7c301a912c4aa374"],
    "row_taps": ["cd6a08bc9a8f5f8a", "5f02f581750629ad", "5f02f581750629ad", "cd6a08bc9a8f5f8a"],
    "ends": ["e9dce614111c3e80", "9375f8ec4b77e05f", "e101233630be080e", "e4f98ea8821f5359", "57762f845b8acd50", "830a12825863a29c",
             "b5ad6903aab5525c", "0b3551141fc4a96d", "8954a694bd981633", "30ce2f228f45cf78"],
    "ring": ["4546ab5189c6dde1", "f937156fceec85e1", "e02c7eae42a6cfe4", "7fb9bf1b140ab413"],
}


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


def oracle_all(caps):
    with ProcessPoolExecutor(host_workers()) as pool:
        exp = list(pool.map(partial(oracle_receive_job, want_soft=True), caps))
    for e in exp:
        e["amb"] = ambiguous(e["soft"])
    return exp


def run(amd, monkeypatch, shape, caps, pieces=WHOLE, first=None, **kw):
    """the captures through one context of the given launch shape ("fp64", "int16": one stream per capture; "wg4": 516 streams of
    which WG4_SLOTS carry them), every stream fed `first` samples (if given), then the pieces in turn, a round after every piece,
    frames popped every round; -> per-stream results"""
    n = [c.size // 2 for c in caps]
    assert max(n) <= MAX_SAMPLES
    kw.setdefault("max_samples", max(n) + 64)
    if shape == "wg4":
        assert len(caps) <= len(WG4_SLOTS)
        d, ks, kernel = amd.Demod(WG4_S, streaming=True, **kw), WG4_SLOTS[: len(caps)], "k_msk_frontend_rb_wg4"
    else:
        d, ks, kernel = make_demod(amd, monkeypatch, shape == "int16", len(caps), streaming=True, **kw), list(range(len(caps))), "k_msk_frontend_rb"
    try:
        at, accs, rounds = [0] * len(caps), [new_acc() for _ in caps], 0
        while rounds == 0 or min(a - m for a, m in zip(at, n)) < 0:
            piece = first if (first is not None and rounds == 0) else pieces[(rounds - (first is not None)) % len(pieces)]
            for j, (k, c) in enumerate(zip(ks, caps)):
                m = min(piece, n[j] - at[j])
                if m > 0:
                    d.push(k, c[2 * at[j]: 2 * (at[j] + m)])
                    at[j] += m
                    if at[j] == n[j]:
                        d.flush(k)
            d.process()
            d.sync()
            assert d.frontend_kernel() == kernel
            for j, k in enumerate(ks):
                assert drain(d, k, accs[j]).stalled == 0, (rounds, k)
            rounds += 1
        return [result(amd, d, k, accs[j]) for j, k in enumerate(ks)]
    finally:
        d.close()


def identical(a, b, what):
    assert_same(dict(a, state=state_tuple(a["state"])), dict(b, state=state_tuple(b["state"])), what)


def digest(soft):
    return hashlib.sha256(np.ascontiguousarray(soft, "<f8").tobytes()).hexdigest()[:16]


def same_as_parent(key, got, shape):
    have = [digest(g["soft"]) for g in got]
    print(f"{key} {shape}: {have}")
    assert have == DIGESTS[key], f"{key}, {shape}: soft logs differ from the parent commit's"


class Shared:
    """the fp64-ring results of a capture set, computed by whichever case runs first and compared with by the others"""

    def __init__(self):
        self.got = {}

    def fp64(self, amd, monkeypatch, key, caps, **kw):
        if key not in self.got:
            self.got[key] = run(amd, monkeypatch, "fp64", caps, **kw)
        return self.got[key]


@pytest.fixture(scope="module")
def shared():
    return Shared()


def runs_of_zeros(soft):
    z = np.concatenate([[0], (soft == 0.0).astype(np.int8), [0]])
    d = np.diff(z)
    a, b = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    return list(zip(a.tolist(), (b - a).tolist()))


def _zeroed(base, ranges):
    z = base.reshape(-1, 2).copy()
    for a, b in ranges:
        z[a:b] = 0
    return np.ascontiguousarray(z.reshape(-1))


# ------------------------------------------------------------------ A1. the largest row partials
FULL_NAMES = ["plus_full", "minus_full", "alternating"]


@pytest.fixture(scope="module")
def full_scale_set():
    n = CHUNK + 12345
    alt = np.where(np.arange(n) & 1, -32768, 32767).astype(np.int16)
    caps = [np.full(2 * n, 32767, np.int16), np.full(2 * n, -32768, np.int16), np.ascontiguousarray(np.repeat(alt, 2))]
    exp = oracle_all(caps)
    assert all(len(e["chunks"]) == 2 and e["amb"].size == 0 for e in exp)
    assert all(np.mean(np.abs(e["soft"])) > 1e9 for e in exp[:2])             # partials of ~32767 * 15 per row and component
    return caps, exp


@pytest.mark.parametrize("shape", SHAPES)
def test_full_scale_row_partials(amd, full_scale_set, shared, monkeypatch, shape):
    caps, exp = full_scale_set
    ref = shared.fp64(amd, monkeypatch, "full", caps)
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, caps)
    same_as_parent("full_scale", got, shape)
    for name, g, e, r in zip(FULL_NAMES, got, exp, ref):
        check_capture(amd, g, e, "patho", f"{shape} {name}")
        identical(g, r, f"{name}: {shape} vs fp64 ring")


# ------------------------------------------------------------------ A2 / B4. whole rows of exact zeros, silent symbols in every slot
ROW_EDGES = (5, 20, 35)                       # a symbol at pos = 40 k spans samples 40 k - 10 .. 40 k + 49: 15, 30, 45 samples into it


@pytest.fixture(scope="module")
def row_gap_set(oracle):
    """a clean capture on tune (the timing loop keeps pos within a sample of 40 k + mu) with gaps that begin and end on the row
    boundaries of a symbol's span, every pair of (begin, end) boundaries, silencing 1 .. 6 whole symbols between the partly
    silent ones; a gap is moved by whole symbols until the oracle shows no one-tap window"""
    base = impair(oracle.modulate(oracle.bert_frames(3, "ROWS", first=11)), amp=7000.0)
    lead = int(np.nonzero(base.reshape(-1, 2).any(axis=1))[0][0])
    gaps, k = [], 60
    for rep in range(3):
        for a in ROW_EDGES:
            for b in ROW_EDGES:
                nsil = 2 + (len(gaps) % 6)
                gaps.append([lead + 40 * k + a, lead + 40 * (k + nsil) + b])
                k += 70 + len(gaps) % 4                                       # the runs begin at every index mod 4
    for _ in range(200):
        x = _zeroed(base, gaps)
        e = oracle.receive(x, streaming=True)
        amb = ambiguous(e["soft"])
        if amb.size == 0:
            break
        at = lead + 40 * int(amb.min())
        j = int(np.argmin([min(abs(q - at), abs(r - at)) for q, r in gaps]))
        gaps[j][0] += 40; gaps[j][1] += 40
    else:
        raise AssertionError("could not remove the one-tap windows")
    assert x.size // 2 <= MAX_SAMPLES
    e["amb"] = amb
    runs = [r for r in runs_of_zeros(e["soft"]) if r[0] > 0]
    assert len(runs) >= 20 and {a % 4 for a, _ in runs} == {0, 1, 2, 3}, runs      # a silent symbol in every slot of a trip
    assert {a % 4 for a, n in runs if n >= 2} == {0, 1, 2, 3}
    return x, e


@pytest.mark.parametrize("shape", SHAPES)
def test_rows_of_exact_zeros(amd, row_gap_set, shared, monkeypatch, shape):
    x, exp = row_gap_set
    ref = shared.fp64(amd, monkeypatch, "rowgaps", [x])
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, [x])
    same_as_parent("row_gaps", got, shape)
    print(f"{shape}: edge_ties {got[0]['state'].edge_ties}")
    check_capture(amd, got[0], exp, "gap", f"row gaps, {shape}")
    assert np.array_equal(got[0]["soft"] == 0.0, exp["soft"] == 0.0)
    identical(got[0], ref[0], f"row gaps: {shape} vs fp64 ring")


# ------------------------------------------------------------------ A3. one-tap windows in each row's sample range
@pytest.fixture(scope="module")
def row_tap_set(oracle):
    """all zeros but one sample. On silence pos = 40 k exactly, symbol k spans samples 40 k - 10 .. 40 k + 49 and row r of it samples
    40 k - 10 + 15 r .. + 14: the sample stands in the middle of row r of symbol 2500 (and, 40 samples further into it, in a row of
    symbol 2499 where that exists). The oracle alone decides which amplitude serves: one at which its two energies round equal,
    soft = 0 throughout, as for tests/test_gpu_symbol_slots.py's single_tap"""
    n = CHUNK + 30000
    caps, exp = [], []
    for r in range(4):
        for amp in (12000, 9000, 15000, 5000, 20000, 7000):
            x = np.zeros(2 * n, np.int16)
            at = 40 * 2500 - 10 + 15 * r + 7
            x[2 * at], x[2 * at + 1] = amp, -(amp // 2)
            e = oracle.receive(x, streaming=True)
            if np.all(e["soft"] == 0.0):
                e["amb"] = ambiguous(e["soft"])
                caps.append(x); exp.append(e)
                break
        else:
            raise AssertionError(f"row {r}: no amplitude at which the oracle's energies round equal")
    return caps, exp


@pytest.mark.parametrize("shape", SHAPES)
def test_one_tap_window_in_each_row(amd, row_tap_set, shared, monkeypatch, shape):
    caps, exp = row_tap_set
    ref = shared.fp64(amd, monkeypatch, "rowtaps", caps)
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, caps)
    same_as_parent("row_taps", got, shape)
    for r, (g, e, f) in enumerate(zip(got, exp, ref)):
        st = g["state"]
        print(f"{shape} row {r}: edge_ties {st.edge_ties}, non-zero softs {g['soft'][g['soft'] != 0.0]}")
        assert st.stalled == 0 and st.edge_ties >= 1 and st.total_symbols == e["n_soft"] == len(g["soft"]), (shape, r, st.edge_ties)
        assert int(np.sum(g["soft"] != 0.0)) <= 2 and float(np.max(np.abs(g["soft"]))) <= 8 * 2.0 ** -25, (shape, r)
        assert np.array_equal(g["chunks"][:, 3:], e["chunks"][:, 3:]) and np.allclose(g["chunks"][:, :3], e["chunks"][:, :3], rtol=0, atol=CARRY_ATOL)
        assert len(g["frames"]) == 0 and len(g["events"]) == len(e["events"]) == 0
        identical(g, f, f"row {r}: {shape} vs fp64 ring")


# ------------------------------------------------------------------ B1 / B3. calls at even and odd soft indices, last calls of 1 .. 9 symbols
TAILS = list(range(5, 410, 10))


@pytest.fixture(scope="module")
def ends_set(oracle):
    base = oracle.modulate(oracle.bert_frames(2, "PAIR", first=23))
    plain = impair(base, amp=3300.0, f0_hz=380.0, ebn0_db=15.0, seed=2502)
    caps = [np.ascontiguousarray(plain[: 2 * (CHUNK + t)]) for t in TAILS]
    exp = oracle_all(caps)
    assert all(len(e["chunks"]) == 2 and e["chunks"][0, 4] == 2167 for e in exp)       # the second call starts at an odd soft index
    tail_syms = [int(e["chunks"][1, 4]) for e in exp]
    pick = [tail_syms.index(k) for k in (1, 2, 3, 4, 5, 6, 7, 9)]
    have = [tail_syms.index(8)]
    caps, exp = [caps[k] for k in pick + have], [exp[k] for k in pick + have]
    # ... and one of three calls, whose third call starts at an even index again
    three = np.ascontiguousarray(plain[: 2 * (2 * CHUNK + 2000)])
    e3 = oracle_all([three])[0]
    starts = np.concatenate([[0], np.cumsum(e3["chunks"][:, 4])[:-1]]).astype(int)
    assert len(starts) == 3 and starts[1] % 2 == 1 and starts[2] % 2 == 0, starts
    return caps + [three], exp + [e3]


@pytest.mark.parametrize("feed", ["whole", "tail_in_its_own_launch"])
def test_call_starts_and_last_calls(amd, ends_set, monkeypatch, feed):
    caps, exp = ends_set
    kw = {} if feed == "whole" else dict(first=CHUNK + 3)
    got = run(amd, monkeypatch, "fp64", caps, **kw)
    same_as_parent("ends", got, f"fp64 {feed}")
    for k, (g, e) in enumerate(zip(got, exp)):
        check_stream(amd, g, e, f"{feed} stream {k}", edge_ties=0, offset_ties=None)
        assert len(g["soft"]) == e["n_soft"]
    ref = run(amd, monkeypatch, "int16", caps[:8], **kw)
    wg4 = run(amd, monkeypatch, "wg4", caps[:8], **kw)
    for k, (g, r, w) in enumerate(zip(got, ref, wg4)):
        identical(g, r, f"{feed} stream {k}: fp64 ring vs int16 ring")
        identical(g, w, f"{feed} stream {k}: fp64 ring vs _rb_wg4")


# ------------------------------------------------------------------ B2. the smallest soft ring, wrapping on every slot
@pytest.fixture(scope="module")
def ring_set(oracle):
    base = impair(oracle.modulate(oracle.bert_frames(5, "RING5", first=35)), amp=2700.0, f0_hz=-510.0, ebn0_db=15.0, seed=2510)
    caps = [np.ascontiguousarray(base[2 * 40 * j: 2 * MAX_SAMPLES]) for j in range(4)]
    exp = oracle_all(caps)
    assert all(e["n_soft"] > CAP_SOFT + 2000 and len(e["frames"]) >= 3 for e in exp), [(e["n_soft"], len(e["frames"])) for e in exp]
    return caps, exp


@pytest.mark.parametrize("shape", SHAPES)
def test_smallest_soft_ring_with_paired_stores(amd, ring_set, shared, monkeypatch, shape):
    caps, exp = ring_set
    kw = dict(pieces=WRAP_PIECES, max_samples=SMALL_M)
    ref = shared.fp64(amd, monkeypatch, "ring", caps, **kw)
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, caps, **kw)
    same_as_parent("ring", got, shape)
    for k, (g, e, r) in enumerate(zip(got, exp, ref)):
        check_stream(amd, g, e, f"{shape} ring stream {k}", edge_ties=0, offset_ties=None)
        assert len(g["soft"]) == e["n_soft"]
        identical(g, r, f"ring stream {k}: {shape} vs fp64 ring")
