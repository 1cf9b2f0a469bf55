"""GPU: the path the stream's wave walks between two batches of symbols (csrc/k_frontend.hip, the loop nest at the end of
msk_frontend_body). A batch made of whole four-symbol trips goes from `housekeeping` straight back to `housekeeping`: the previous
sums are not copied, fo stays unsettled, the `while` test is not evaluated and the tap read of the batch's last symbol is kept; only
a batch with fewer than four provably clear symbols takes the remainder path (pairs, one last symbol, settle, copy, refetch).

Where a batch ends depends on when the fp64 ring's helper wave publishes, so no result may depend on it. The bit-for-bit digests of
test_gpu_symbol_body.py are the main proof; the tests here drive the places where the control flow between batches can go wrong.
Each runs on the fp64 ring, is held to the oracle and must be IDENTICAL to the int16 ring (another batch structure altogether: its
batches are cut by tile events at fixed sample positions):

 1. segmentation: one noisy capture of four whole demodulate() calls and a tail, fed whole and in odd pieces (pieces below one
    symbol; a launch that finds exactly one chunk and not a sample more; a launch that runs two calls; launches that find nothing
    to do). A -s call is a whole chunk or the tail at the end of the capture, so what the pieces move is which launch runs a call,
    where its samples lie in the stream's buffer and what the helper has ready when the call's first batches begin;
 2. call ends: tails behind one whole chunk sized so that the last call has 1, 2, .. 9 and more symbols (every residue of a trip
    behind the call's first symbol), pushed whole and with the tail in a launch of its own, with streams that end every call ON
    the +/-2000 Hz clamp of the AFC (the chunk log's fo is the settled value); per call {fo, tf, mu, leftover, nsym} against the oracle;
 3. the soft ring's bound: the smallest ring (8192 symbols), four streams staggered by 0 .. 3 symbols, frames popped between rounds;
 4. digital silence inside batches: ~90 gaps of one to five silent symbols each; the out-of-line routine is entered for each of
    them and for the symbol behind them, some 300 times, spread over the four slots of a trip by the gaps' random spacing;
 5. an out-of-range -o: the second-symbol instantiation followed directly by batches of whole trips.

Bounds: stream_checks.check_stream as it stands (soft symbols < 1e-9 of their mean, decisions and integer columns ==, the chunk
log's float columns 1e-7), for the gapped capture stream_runs.check_capture's "gap" class as it stands (soft 1e-8 of
the mean, edge_ties <= 12); against the int16 ring and between two segmentations: identity."""
from concurrent.futures import ProcessPoolExecutor
from functools import partial

import numpy as np
import pytest

from fixtures import amd  # noqa: F401
from hostile_inputs import ambiguous
from oracle_lib import impair
from soak_inputs import host_workers, oracle_receive_job
from stream_checks import _gapped_capture, check_stream
from stream_runs import (CAP_SOFT, CHUNK, SMALL_M, WRAP_PIECES, assert_same, check_capture, drain, make_demod, new_acc, result,
                         state_tuple)

pytestmark = pytest.mark.gpu
WHOLE = [1 << 30]


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


def oracle_all(caps):
    with ProcessPoolExecutor(host_workers()) as pool:
        return list(pool.map(partial(oracle_receive_job, want_soft=True), caps))


def run(amd, monkeypatch, int16, caps, pieces=WHOLE, first=None, **kw):
    """the captures through one context on the fp64 or (int16) the int16 ring, every stream fed `first` samples (if given), then
    the pieces in turn (cycled), a round after every piece, frames popped every round; -> (per-stream results, rounds)"""
    n = [c.size // 2 for c in caps]
    kw.setdefault("max_samples", max(n) + 64)
    d = make_demod(amd, monkeypatch, int16, len(caps), streaming=True, **kw)
    try:
        at, accs, rounds = [0] * len(caps), [new_acc() for _ in caps], 0
        while rounds == 0 or min(a - m for a, m in zip(at, n)) < 0:
            piece = first if (first is not None and rounds == 0) else pieces[(rounds - (first is not None)) % len(pieces)]
            for k, c in enumerate(caps):
                m = min(piece, n[k] - at[k])
                if m > 0:
                    d.push(k, c[2 * at[k]: 2 * (at[k] + m)])
                    at[k] += m
                    if at[k] == n[k]:
                        d.flush(k)
            d.process()
            d.sync()
            assert d.frontend_kernel() == "k_msk_frontend_rb"
            for k in range(len(caps)):
                assert drain(d, k, accs[k]).stalled == 0, (rounds, k)
            rounds += 1
        return [result(amd, d, k, accs[k]) for k in range(len(caps))], rounds
    finally:
        d.close()


def identical(a, b, what):
    assert_same(dict(a, state=state_tuple(a["state"])), dict(b, state=state_tuple(b["state"])), what)


# ------------------------------------------------------------------ 1. segmentation cannot matter
SEG_N = 4 * CHUNK + 2000
# 86 719 samples in three pieces (two of them shorter than a symbol): nothing to do; the chunk's last sample: call 0 with not a
# sample to spare; 45: nothing to do; one more chunk: call 1; two chunks and three samples: calls 2 and 3 in one launch; the rest
# in pieces of one to five symbols' worth, the last of them followed by the flush (the tail call)
SEG_PIECES = [13, 39, CHUNK - 53, 1, 45, CHUNK, 2 * CHUNK + 3, 57, 120, 200, 40, 80, 160, 7, 301, 1000]


@pytest.fixture(scope="module")
def seg_set(oracle):
    x = impair(oracle.modulate(oracle.bert_frames(5, "SEG", first=31)), amp=2800.0, f0_hz=830.0, ebn0_db=13.0, seed=1301)
    x = np.ascontiguousarray(x[: 2 * SEG_N])
    assert x.size // 2 == SEG_N <= 350000 and sum(SEG_PIECES[:4]) == CHUNK
    exp = oracle.receive(x, streaming=True)
    assert len(exp["chunks"]) == 5 and len(exp["frames"]) >= 2
    return x, exp


def test_segmentation_cannot_matter(amd, seg_set, monkeypatch):
    x, exp = seg_set
    whole, r0 = run(amd, monkeypatch, False, [x])
    cut, r1 = run(amd, monkeypatch, False, [x], pieces=SEG_PIECES)
    assert r0 == 1 and r1 >= 14
    check_stream(amd, whole[0], exp, "whole", edge_ties=0, offset_ties=None)
    check_stream(amd, cut[0], exp, "in pieces", edge_ties=0, offset_ties=None)
    identical(cut[0], whole[0], "fp64 ring: in pieces vs whole")
    identical(whole[0], run(amd, monkeypatch, True, [x])[0][0], "whole: fp64 ring vs int16 ring")
    identical(cut[0], run(amd, monkeypatch, True, [x], pieces=SEG_PIECES)[0][0], "in pieces: fp64 ring vs int16 ring")


# ------------------------------------------------------------------ 2. call ends
TAILS = list(range(5, 570, 10))               # samples behind the whole chunk: the tail call sees them + the chunk's leftover
CLAMP_F0 = (2300.0, -2300.0)                   # a carrier beyond the AFC's clamp: the loop leans on it
CLAMP_TAILS = list(range(205, 405, 20))        # 5 .. 10 symbols in the tail call


@pytest.fixture(scope="module")
def ends_set(oracle):
    base = oracle.modulate(oracle.bert_frames(2, "ENDS", first=12))
    plain = impair(base, amp=3300.0, f0_hz=-420.0, ebn0_db=15.0, seed=1302)
    caps = [np.ascontiguousarray(plain[: 2 * (CHUNK + t)]) for t in TAILS]
    for j, f0 in enumerate(CLAMP_F0):
        for ebn0, tails in ((None, CLAMP_TAILS), (16.0, CLAMP_TAILS[:4])):     # clean: ON the clamp at every call's end; noisy: around it
            y = impair(base, amp=3000.0, f0_hz=f0, ebn0_db=ebn0, seed=1303 + j)
            caps += [np.ascontiguousarray(y[: 2 * (CHUNK + t)]) for t in tails]
    exp = oracle_all(caps)
    # what the set is for, from the oracle alone: the tail call has 1 .. 9 symbols and more, and its symbols behind the first one
    # leave every residue of a four-symbol trip; the clamp streams end their calls on the clamp
    assert all(len(e["chunks"]) == 2 and e["chunks"][0, 4] == 2167 for e in exp)
    tail_syms = [int(e["chunks"][1, 4]) for e in exp[: len(TAILS)]]
    assert set(range(1, 10)) <= set(tail_syms) and max(tail_syms) >= 13, tail_syms
    assert {(s - 1) % 4 for s in tail_syms if s >= 6} == {0, 1, 2, 3}
    # (the oracle shows: the clean +2300 Hz streams end the chunk and most tails with fo ON the clamp; at -2300 Hz and under noise the
    # loop saw-tooths a few Hz inside it, clamped on many symbols but not on a call's last)
    clamp = exp[len(TAILS):]
    assert all(np.all(np.abs(e["chunks"][:, 0]) > 1970.0) and e["chunks"][1, 4] >= 5 for e in clamp)
    clean = clamp[: len(CLAMP_TAILS)]
    assert all(e["chunks"][0, 0] == 2000.0 for e in clean) and sum(e["chunks"][1, 0] == 2000.0 for e in clean) >= 6
    assert {int(e["chunks"][1, 4]) for e in clean} >= {5, 6, 7, 8, 9}
    return caps, exp


@pytest.mark.parametrize("feed", ["whole", "tail_in_its_own_launch"])
def test_call_ends(amd, ends_set, monkeypatch, feed):
    """per call {fo, tf, mu, leftover, nsym} (check_stream: integers ==, floats 1e-7) and everything else. tail_in_its_own_launch:
    the chunk and 17 samples first (one whole call, nothing left to do), then the rest and the flush: a launch whose only call is
    the tail's handful of symbols"""
    caps, exp = ends_set
    kw = {} if feed == "whole" else dict(first=CHUNK + 17)
    got, rounds = run(amd, monkeypatch, False, caps, **kw)
    assert rounds == (1 if feed == "whole" else 2)
    for k, (g, e) in enumerate(zip(got, exp)):
        check_stream(amd, g, e, f"{feed} stream {k} ({caps[k].size // 2 - CHUNK} samples behind the chunk)", edge_ties=0, offset_ties=None)
    ref, _ = run(amd, monkeypatch, True, caps, **kw)
    for k, (g, r) in enumerate(zip(got, ref)):
        identical(g, r, f"{feed} stream {k}: fp64 ring vs int16 ring")


# ------------------------------------------------------------------ 3. the soft ring's bound
@pytest.fixture(scope="module")
def ring_set(oracle):
    """four 12-frame captures whose starts are staggered by 0, 1, 2 and 3 symbols: the ring's wrap (a fixed symbol count) moves
    against the batches (cut at sample positions / by the helper's publications) by one symbol from stream to stream"""
    base = impair(oracle.modulate(oracle.bert_frames(12, "RING", first=91)), amp=2700.0, f0_hz=510.0, ebn0_db=15.0, seed=1310)
    caps = [np.ascontiguousarray(base[2 * 40 * j:]) for j in range(4)]
    exp = oracle_all(caps)
    assert all(e["n_soft"] > 3 * CAP_SOFT for e in exp)           # three wraps per stream
    return caps, exp


def test_soft_ring_bound_cuts_batches(amd, ring_set, monkeypatch):
    caps, exp = ring_set
    got, rounds = run(amd, monkeypatch, False, caps, pieces=WRAP_PIECES, max_samples=SMALL_M)
    assert rounds >= 30
    for k, (g, e) in enumerate(zip(got, exp)):
        check_stream(amd, g, e, f"ring stream {k}", edge_ties=0, offset_ties=None)
    ref, _ = run(amd, monkeypatch, True, caps, pieces=WRAP_PIECES, max_samples=SMALL_M)
    for k, (g, r) in enumerate(zip(got, ref)):
        identical(g, r, f"ring stream {k}: fp64 ring vs int16 ring")


# ------------------------------------------------------------------ 4. silence inside batches
@pytest.fixture(scope="module")
def gap_set(oracle):
    iq3 = oracle.modulate(oracle.bert_frames(3, "GAPS", first=5))
    x, starts = _gapped_capture(oracle, iq3)                      # 1.2 kHz off tune, gaps of 105 .. 259 zeros, no one-tap window
    exp = oracle.receive(x, streaming=True)
    exp["amb"] = ambiguous(exp["soft"])
    silent = int(np.sum(exp["soft"] == 0.0))
    assert len(starts) >= 60 and exp["amb"].size == 0 and silent >= 2 * len(starts), (len(starts), silent)
    return np.ascontiguousarray(x), exp


def test_silence_inside_batches(amd, gap_set, monkeypatch):
    x, exp = gap_set
    got = run(amd, monkeypatch, False, [x])[0][0]
    check_capture(amd, got, exp, "gap", "gaps, fp64 ring")
    identical(got, run(amd, monkeypatch, True, [x])[0][0], "gaps: fp64 ring vs int16 ring")
    cut = run(amd, monkeypatch, False, [x], pieces=[50021, 777, 100003])[0][0]
    identical(cut, got, "gaps: in pieces vs whole")


# ------------------------------------------------------------------ 5. an out-of-range -o
def test_out_of_range_initial_offset(amd, oracle, monkeypatch):
    x = impair(oracle.modulate(oracle.bert_frames(2, "WIDE", first=6)), amp=2500.0, f0_hz=1800.0, ebn0_db=16.0, seed=1320)
    exp = oracle.receive(x, streaming=True, init_offset=2500.0)
    assert len(exp["chunks"]) >= 2
    got = run(amd, monkeypatch, False, [x], init_offset=2500.0)[0][0]
    check_stream(amd, got, exp, "-o 2500", edge_ties=0, offset_ties=None)
    identical(got, run(amd, monkeypatch, True, [x], init_offset=2500.0)[0][0], "-o 2500: fp64 ring vs int16 ring")
