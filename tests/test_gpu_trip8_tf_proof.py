"""GPU: what csrc/k_frontend.hip's loop nest decides per demodulate() call.

 * Per call the stream's wave evaluates opv_tf_clamp_cannot_act (csrc/opv_tf_rule.h; tests/test_tf_clamp_rule_host.py holds the rule
   itself) and runs one of two instantiations of the call's symbols: the guarded nest keeps the timing loop's clamp, the free nest
   drops it. fmin(fmax(x, -0.1), 0.1) is x for every x inside the bounds, so WHICH nest ran must not show in any result.
   OPV_FRONTEND_TF_GUARD=1 forces the guarded nest, OPV_TEST_TIMING_FREQ0 starts every stream from a chosen timing_freq (nothing
   else brings one near the clamp), opv_tap_frontend_calls counts the calls by nest.
 * Both nests are the whole section of a call: first symbol, the second one under an out-of-range -o, batches of four-symbol
   trips with the fast boundary, the remainder path. The free nest is new code at every one of those places. (Eight-symbol trips,
   which this module was first written for, were measured worth 2.7 cycles per symbol and not kept: NOTEBOOK.md.)

 1. nest choice cannot matter: a noisy and a clean capture, by default and with the guard forced, on the fp64 ring, the int16
    ring and _rb_wg4: identical between the two runs, held to the oracle, the tap all free / all guarded;
 2. calls that must be guarded are, and are right: streams started ON the clamp, just inside it, one ulp either side of the rule's
    threshold and well inside, on captures whose clock error leans the loop outward, each held to the oracle's chunk chain started
    from the same timing_freq, identical to the same run with the guard forced, the tap as the rule says on the oracle's own
    per-call timing_freq;
 3. the free nest at the edges of calls and batches: last calls of 1 .. 17 symbols, the smallest soft ring on eight streams
    staggered by 0 .. 7 symbols, ~90 silence gaps, an out-of-range -o; fp64 ring, identical to the int16 ring (and, where the run is
    short, to the guarded nest), held to the oracle. Where a batch ends depends on the helper wave's timing and is not asserted.

Bounds: stream_checks.check_stream and stream_runs.check_capture as they stand; between runs of the product: identity."""
import math
from concurrent.futures import ProcessPoolExecutor
from functools import partial

import numpy as np
import pytest

from fixtures import amd  # noqa: F401
from hostile_inputs import ambiguous
from oracle_lib import impair, resample_clock
from soak_inputs import host_workers, oracle_receive_job
from stream_checks import _gapped_capture, check_stream
from stream_runs import (CAP_SOFT, CHUNK, SMALL_M, WRAP_PIECES, assert_same, check_capture, drain, make_demod, new_acc, result,
                         state_tuple)

pytestmark = pytest.mark.gpu
WHOLE = [1 << 30]
WG4_S = 516                                   # the first stream counts k_msk_frontend_rb_wg4 serves: 513 ..
WG4_SLOTS = [0, 1, 2, 3, 257, 258, 514, 515]  # every wave of a workgroup; the first, a middle and the last workgroup
BETA, TFMAX = 0.00001, 0.1


def rule(tf, n):
    """csrc/opv_tf_rule.h, operation for operation"""
    return abs(tf) + 2.0 * BETA * float(n // 39 + 2) < TFMAX


@pytest.fixture(scope="module")
def oracle():
    from oracle_lib import Oracle
    return Oracle()


def oracle_all(caps):
    with ProcessPoolExecutor(host_workers()) as pool:
        return list(pool.map(partial(oracle_receive_job, want_soft=True), caps))


def run(amd, monkeypatch, shape, caps, guard=False, tf0=None, pieces=WHOLE, first=None, flush=True, **kw):
    """the captures through one context of the given launch shape ("fp64", "int16": one stream per capture; "wg4": 516 streams of
    which WG4_SLOTS carry them), every stream fed `first` samples (if given), then the pieces in turn, a round after every piece,
    frames popped every round; -> (per-stream results, rounds, per-stream (free, guarded) calls)"""
    n = [c.size // 2 for c in caps]
    kw.setdefault("max_samples", max(n) + 64)
    if guard:
        monkeypatch.setenv("OPV_FRONTEND_TF_GUARD", "1")
    if tf0 is not None:
        monkeypatch.setenv("OPV_TEST_TIMING_FREQ0", float(tf0).hex())
    try:
        if shape == "wg4":
            assert len(caps) <= len(WG4_SLOTS)
            d, ks, kernel = amd.Demod(WG4_S, streaming=True, **kw), WG4_SLOTS[: len(caps)], "k_msk_frontend_rb_wg4"
        else:
            d, ks, kernel = make_demod(amd, monkeypatch, shape == "int16", len(caps), streaming=True, **kw), list(range(len(caps))), "k_msk_frontend_rb"
    finally:
        monkeypatch.delenv("OPV_FRONTEND_TF_GUARD", raising=False)
        monkeypatch.delenv("OPV_TEST_TIMING_FREQ0", raising=False)
    try:
        at, accs, rounds = [0] * len(caps), [new_acc() for _ in caps], 0
        while rounds == 0 or min(a - m for a, m in zip(at, n)) < 0:
            piece = first if (first is not None and rounds == 0) else pieces[(rounds - (first is not None)) % len(pieces)]
            for j, (k, c) in enumerate(zip(ks, caps)):
                m = min(piece, n[j] - at[j])
                if m > 0:
                    d.push(k, c[2 * at[j]: 2 * (at[j] + m)])
                    at[j] += m
                    if at[j] == n[j] and flush:
                        d.flush(k)
            d.process()
            d.sync()
            assert d.frontend_kernel() == kernel
            for j, k in enumerate(ks):
                assert drain(d, k, accs[j]).stalled == 0, (rounds, k)
            rounds += 1
        return [result(amd, d, k, accs[j]) for j, k in enumerate(ks)], rounds, [d.frontend_calls(k) for k in ks]
    finally:
        d.close()


def identical(a, b, what):
    assert_same(dict(a, state=state_tuple(a["state"])), dict(b, state=state_tuple(b["state"])), what)


# ------------------------------------------------------------------ 1. nest choice cannot matter
@pytest.fixture(scope="module")
def pair_set(oracle):
    noisy = impair(oracle.modulate(oracle.bert_frames(5, "NEST", first=31)), amp=2800.0, f0_hz=830.0, ebn0_db=13.0, seed=2301)
    noisy = np.ascontiguousarray(noisy[: 2 * (4 * CHUNK + 2000)])
    clean = np.ascontiguousarray(impair(oracle.modulate(oracle.bert_frames(3, "NEST", first=7)), amp=3100.0))
    caps = [noisy, clean]
    exp = oracle_all(caps)
    assert len(exp[0]["chunks"]) == 5 and len(exp[0]["frames"]) >= 2 and len(exp[1]["frames"]) == 3
    assert max(float(np.max(np.abs(e["chunks"][:, 1]))) for e in exp) < 0.01          # timing_freq nowhere near the rule's 0.055
    return caps, exp


@pytest.mark.parametrize("shape", ["fp64", "int16", "wg4"])
def test_nest_choice_cannot_matter(amd, pair_set, monkeypatch, shape):
    caps, exp = pair_set
    free, _, calls_f = run(amd, monkeypatch, shape, caps)
    forced, _, calls_g = run(amd, monkeypatch, shape, caps, guard=True)
    for j, e in enumerate(exp):
        check_stream(amd, free[j], e, f"{shape} capture {j}, by the rule", edge_ties=0, offset_ties=None)
        check_stream(amd, forced[j], e, f"{shape} capture {j}, guard forced", edge_ties=0, offset_ties=None)
        identical(free[j], forced[j], f"{shape} capture {j}: by the rule vs guard forced")
        assert calls_f[j] == (len(e["chunks"]), 0) and calls_g[j] == (0, len(e["chunks"])), (shape, j, calls_f[j], calls_g[j])


# ------------------------------------------------------------------ 2. calls that must be guarded are, and are right
def _threshold_pair(n):
    """adjacent doubles (free, guarded) either side of the rule's threshold for a call of n samples, by bisection on the rule"""
    lo, hi = 0.0, TFMAX
    while math.nextafter(lo, 1.0) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if rule(mid, n) else (lo, mid)
    return lo, hi


THR_BELOW, THR_ABOVE = _threshold_pair(CHUNK)
TF0 = {"on_the_clamp+": 0.1, "on_the_clamp-": -0.1, "inside+": 0.0999, "inside-": -0.0999, "threshold-1ulp": THR_BELOW,
       "threshold+1ulp": THR_ABOVE, "well_inside": 0.03}
N_CALLS = 5


def chain_job(args):
    """the oracle's -s chunk chain (oracle/opv_oracle.c: oro_receive, streaming) over whole chunks only, from a demodulator whose
    timing_freq starts at tf0; tracker and decoder over its soft log"""
    x, tf0 = args
    from oracle_lib import Oracle
    o = Oracle()
    d = o.new_demod()
    d.afc_alpha = 0.001
    d.timing_freq = tf0
    n, start, softs, chunks, est = x.size // 2, 0, [], [], float("nan")
    while n - start >= CHUNK:
        c = x[2 * start: 2 * (start + CHUNK)]
        if not chunks:
            est = o.estimate_offset(c)
            d.freq_offset = est
        s = o.demodulate(d, c)
        softs.append(s)
        chunks.append([d.freq_offset, d.timing_freq, d.mu, float(d.leftover), float(len(s))])
        lo = d.leftover
        start += CHUNK - lo if 0 < lo < CHUNK else CHUNK
    soft = np.concatenate(softs)
    e = o.track(soft)
    keep = e["metrics"] >= 0                                     # (a frame the decoder drops is not released to the caller)
    return dict(frames=e["frames"][keep], metrics=e["metrics"][keep], frame_sym=e["frame_sym"][keep], events=e["events"], n_soft=len(soft),
                soft=soft, est_offset=est, final_freq_offset=d.freq_offset, final_state=e["final_state"], chunks=np.array(chunks))


@pytest.fixture(scope="module")
def lean_set(oracle):
    """per tf0: a clean 6-frame capture whose sample clock is 4000 ppm off in the direction that leans the loop OUTWARD (a positive
    timing_freq is a symbol longer than 40 samples: resample_clock with a negative ppm), cut so that five whole calls run and no
    tail; the oracle's chain from that tf0"""
    base = impair(oracle.modulate(oracle.bert_frames(6, "LEAN", first=3)), amp=3000.0)
    caps = {}
    for name, tf0 in TF0.items():
        x = resample_clock(base, -4000.0 if tf0 > 0 else 4000.0)
        caps[name] = np.ascontiguousarray(x[: 2 * (N_CALLS * CHUNK + 40)])
        assert caps[name].size // 2 <= 440000
    with ProcessPoolExecutor(host_workers()) as pool:
        exps = dict(zip(caps, pool.map(chain_job, [(caps[k], TF0[k]) for k in caps])))
    for name, e in exps.items():
        ch, tf0 = e["chunks"], TF0[name]
        assert len(ch) == N_CALLS and np.all((ch[:, 4] >= 2150) & (ch[:, 4] <= 2185)), (name, ch[:, 4])
        assert np.all(np.abs(ch[:, 1] - tf0) < 1e-3), (name, ch[:, 1])           # a call moves timing_freq by a few 1e-4 at most
        starts = np.concatenate([[tf0], ch[:-1, 1]])
        e["guarded"] = [not rule(float(t), CHUNK) for t in starts]
        # (the device's timing_freq agrees with the oracle's to ~1e-12: no call start may sit that close to the threshold, the two
        # values chosen to sit ON it excepted - those are the first call's, handed over exactly)
        assert all(abs(abs(float(t)) - THR_BELOW) > 1e-9 for t in starts[1:]), (name, starts)
    # what the rule makes of the oracle's own trajectories
    assert all(all(exps[k]["guarded"]) for k in ("on_the_clamp+", "on_the_clamp-", "inside+", "inside-"))
    assert not any(exps["well_inside"]["guarded"])
    assert exps["threshold+1ulp"]["guarded"][0] and not exps["threshold-1ulp"]["guarded"][0]
    # (started ON the clamp, every symbol whose timing error points outward is clamped until the first inward one; the chunk log
    # shows call ENDS only, and those wander a few 1e-4 inside: 0.09974 .. 0.09992 here)
    return caps, exps


@pytest.mark.parametrize("name", list(TF0))
def test_guarded_calls_are_guarded_and_right(amd, lean_set, monkeypatch, name):
    """per call {fo, tf, mu, leftover, nsym} and the soft symbols by check_stream's bounds against the oracle's chain from the same
    timing_freq; identical to the run with the guard forced; the tap's counts are the rule's verdicts on the oracle's per-call
    timing_freq"""
    caps, exps = lean_set
    x, e, tf0 = caps[name], exps[name], TF0[name]
    got, _, calls = run(amd, monkeypatch, "fp64", [x], tf0=tf0, flush=False)
    forced, _, calls_g = run(amd, monkeypatch, "fp64", [x], tf0=tf0, flush=False, guard=True)
    print(f"{name}: tf0 {tf0!r}, calls (free, guarded) {calls[0]}, oracle per-call tf {e['chunks'][:, 1]}")
    check_stream(amd, got[0], e, f"tf0 {name}", edge_ties=0, offset_ties=None)
    identical(got[0], forced[0], f"tf0 {name}: by the rule vs guard forced")
    n_g = sum(e["guarded"])
    assert calls[0] == (N_CALLS - n_g, n_g) and calls_g[0] == (0, N_CALLS), (name, calls, calls_g, e["guarded"])
    ref, _, _ = run(amd, monkeypatch, "int16", [x], tf0=tf0, flush=False)
    identical(got[0], ref[0], f"tf0 {name}: fp64 ring vs int16 ring")


# ------------------------------------------------------------------ 3. the free nest at the edges of calls and batches
TAILS = list(range(5, 770, 10))                # samples behind the whole chunk: the tail call sees them + the chunk's leftover


@pytest.fixture(scope="module")
def ends_set(oracle):
    base = oracle.modulate(oracle.bert_frames(2, "OCT", first=12))
    plain = impair(base, amp=3300.0, f0_hz=-420.0, ebn0_db=15.0, seed=2302)
    caps = [np.ascontiguousarray(plain[: 2 * (CHUNK + t)]) for t in TAILS]
    exp = oracle_all(caps)
    assert all(len(e["chunks"]) == 2 and e["chunks"][0, 4] == 2167 for e in exp)
    tail_syms = [int(e["chunks"][1, 4]) for e in exp]
    # the last call has 1 .. 17 symbols: behind its first symbol every residue of a trip, up to four whole trips
    assert set(range(1, 18)) <= set(tail_syms), sorted(set(tail_syms))
    return caps, exp


@pytest.mark.parametrize("feed", ["whole", "tail_in_its_own_launch"])
def test_last_calls_of_1_to_17_symbols(amd, ends_set, monkeypatch, feed):
    caps, exp = ends_set
    kw = {} if feed == "whole" else dict(first=CHUNK + 17)
    got, rounds, calls = run(amd, monkeypatch, "fp64", caps, **kw)
    assert rounds == (1 if feed == "whole" else 2)
    for k, (g, e) in enumerate(zip(got, exp)):
        check_stream(amd, g, e, f"{feed} stream {k} ({caps[k].size // 2 - CHUNK} samples behind the chunk)", edge_ties=0, offset_ties=None)
        assert calls[k] == (2, 0), (k, calls[k])
    ref, _, _ = run(amd, monkeypatch, "int16", caps, **kw)
    for k, (g, r) in enumerate(zip(got, ref)):
        identical(g, r, f"{feed} stream {k}: fp64 ring vs int16 ring")


@pytest.fixture(scope="module")
def ring_set(oracle):
    """eight 12-frame captures whose starts are staggered by 0 .. 7 symbols: the ring's wrap (a fixed symbol count) moves against
    the batches by one symbol from stream to stream, twice through every slot of a trip"""
    base = impair(oracle.modulate(oracle.bert_frames(12, "RING8", first=91)), amp=2700.0, f0_hz=510.0, ebn0_db=15.0, seed=2310)
    caps = [np.ascontiguousarray(base[2 * 40 * j:]) for j in range(8)]
    exp = oracle_all(caps)
    assert all(e["n_soft"] > 3 * CAP_SOFT for e in exp)           # three wraps per stream
    return caps, exp


def test_soft_ring_bound_in_the_free_nest(amd, ring_set, monkeypatch):
    caps, exp = ring_set
    got, rounds, _ = run(amd, monkeypatch, "fp64", caps, pieces=WRAP_PIECES, max_samples=SMALL_M)
    assert rounds >= 30
    for k, (g, e) in enumerate(zip(got, exp)):
        check_stream(amd, g, e, f"ring stream {k}", edge_ties=0, offset_ties=None)
    ref, _, _ = run(amd, monkeypatch, "int16", caps, pieces=WRAP_PIECES, max_samples=SMALL_M)
    for k, (g, r) in enumerate(zip(got, ref)):
        identical(g, r, f"ring stream {k}: fp64 ring vs int16 ring")


@pytest.fixture(scope="module")
def gap_set(oracle):
    iq3 = oracle.modulate(oracle.bert_frames(3, "GAPS", first=5))
    x, starts = _gapped_capture(oracle, iq3)                      # 1.2 kHz off tune, gaps of 105 .. 259 zeros, no one-tap window
    exp = oracle.receive(x, streaming=True)
    exp["amb"] = ambiguous(exp["soft"])
    silent = int(np.sum(exp["soft"] == 0.0))
    assert len(starts) >= 60 and exp["amb"].size == 0 and silent >= 2 * len(starts), (len(starts), silent)
    return np.ascontiguousarray(x), exp


def test_silence_in_the_free_nest(amd, gap_set, monkeypatch):
    x, exp = gap_set
    got, _, _ = run(amd, monkeypatch, "fp64", [x])
    check_capture(amd, got[0], exp, "gap", "gaps, fp64 ring")
    identical(got[0], run(amd, monkeypatch, "int16", [x])[0][0], "gaps: fp64 ring vs int16 ring")
    identical(got[0], run(amd, monkeypatch, "fp64", [x], guard=True)[0][0], "gaps: by the rule vs guard forced")
    identical(run(amd, monkeypatch, "fp64", [x], pieces=[50021, 777, 100003])[0][0], got[0], "gaps: in pieces vs whole")


def test_out_of_range_initial_offset_then_the_free_nest(amd, oracle, monkeypatch):
    x = impair(oracle.modulate(oracle.bert_frames(2, "WIDE8", first=6)), amp=2500.0, f0_hz=1800.0, ebn0_db=16.0, seed=2320)
    exp = oracle.receive(x, streaming=True, init_offset=2500.0)
    assert len(exp["chunks"]) >= 2
    got, _, _ = run(amd, monkeypatch, "fp64", [x], init_offset=2500.0)
    check_stream(amd, got[0], exp, "-o 2500", edge_ties=0, offset_ties=None)
    identical(got[0], run(amd, monkeypatch, "int16", [x], init_offset=2500.0)[0][0], "-o 2500: fp64 ring vs int16 ring")
    identical(got[0], run(amd, monkeypatch, "fp64", [x], init_offset=2500.0, guard=True)[0][0], "-o 2500: by the rule vs guard forced")
