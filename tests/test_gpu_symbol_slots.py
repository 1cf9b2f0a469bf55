"""GPU: the places where the symbol loop of csrc/k_frontend.hip gave up issue slots, held to the oracle and to each other.

The loop's arithmetic is frozen bit for bit by tests/test_gpu_symbol_body.py. This module feeds the inputs on which a change of
its INSTRUCTIONS (not of its arithmetic) would show first:

 1. the soft value, now `|S_2|^2` handed out by a DPP move and `|S_1|^2 * -1.0` added by one v_fmac_f64_dpp: equal and zero
    energies. DC, a bare carrier on either tone, real-only and imaginary-only signals, an all-zero capture, a capture with a single
    non-zero sample. The decision "a tie is tone 2" and the sign handed to the phase detector show in the soft log and in the
    AFC state of every call;
 2. the silence test, whose mask now lives in vcc from the compare to the branch: ~90 silence gaps of a few symbols each behind
    symbols of either soft sign (the tone select of the same symbol writes vcc in front of the compare), silence as the first and
    as the second symbol of a call, a whole silent call followed by signal;
 3. the soft log's stores at the edges of calls and batches (the store was moved in front of the phase detector, measured slower
    and put back: the cases stay, the log is written by every symbol): last calls of 1 .. 9 symbols whole and with the tail in a
    launch of its own, the smallest soft ring on four streams staggered by 0 .. 3 symbols with frames popped between rounds, a
    silent symbol as the last symbol of a call.

Shapes: the fp64 ring (k_msk_frontend_rb, 128 threads), the int16 ring (OPV_FRONTEND_INT16_RING=1) and k_msk_frontend_rb_wg4
(516 streams, the eight slots tests/test_gpu_symbol_body.py uses); where the nest matters also with OPV_FRONTEND_TF_GUARD=1.
Bounds: stream_checks.check_stream and stream_runs.check_capture as they stand; between shapes: identity (assert_same).
The helpers cannot pre-fill a stream's soft log, so "nothing beyond n_soft was written" is held the other way the log allows:
length and values against the oracle, and identity with the int16-ring run, whose symbols leave by the same path."""
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
WG4_S = 516                                   # the first stream counts k_msk_frontend_rb_wg4 serves: 513 ..
WG4_SLOTS = [0, 1, 2, 3, 257, 258, 514, 515]  # every wave of a workgroup; the first, a middle and the last workgroup
SHAPES = ["fp64", "int16", "wg4"]
MAX_SAMPLES = 5 * CHUNK                       # no capture of this module is longer than five -s calls


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


def run(amd, monkeypatch, shape, caps, guard=False, pieces=WHOLE, first=None, **kw):
    """the captures through one context of the given launch shape ("fp64", "int16": one stream per capture; "wg4": 516 streams of
    which WG4_SLOTS carry them), every stream fed `first` samples (if given), then the pieces in turn, a round after every piece,
    frames popped every round; -> (per-stream results, rounds)"""
    n = [c.size // 2 for c in caps]
    assert max(n) <= MAX_SAMPLES
    kw.setdefault("max_samples", max(n) + 64)
    if guard:
        monkeypatch.setenv("OPV_FRONTEND_TF_GUARD", "1")
    try:
        if shape == "wg4":
            assert len(caps) <= len(WG4_SLOTS)
            d, ks, kernel = amd.Demod(WG4_S, streaming=True, **kw), WG4_SLOTS[: len(caps)], "k_msk_frontend_rb_wg4"
        else:
            d, ks, kernel = make_demod(amd, monkeypatch, shape == "int16", len(caps), streaming=True, **kw), list(range(len(caps))), "k_msk_frontend_rb"
    finally:
        monkeypatch.delenv("OPV_FRONTEND_TF_GUARD", raising=False)
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
        return [result(amd, d, k, accs[j]) for j, k in enumerate(ks)], rounds
    finally:
        d.close()


def identical(a, b, what):
    assert_same(dict(a, state=state_tuple(a["state"])), dict(b, state=state_tuple(b["state"])), what)


class Shared:
    """the fp64-ring results of a capture set, computed by whichever case runs first and compared with by the others"""

    def __init__(self):
        self.got = {}

    def fp64(self, amd, monkeypatch, key, caps, **kw):
        if key not in self.got:
            self.got[key] = run(amd, monkeypatch, "fp64", caps, **kw)[0]
        return self.got[key]


@pytest.fixture(scope="module")
def shared():
    return Shared()


def runs_of_zeros(soft):
    """[(first, length)] of the runs of exactly-zero soft symbols"""
    z = np.concatenate([[0], (soft == 0.0).astype(np.int8), [0]])
    d = np.diff(z)
    a, b = np.nonzero(d == 1)[0], np.nonzero(d == -1)[0]
    return list(zip(a.tolist(), (b - a).tolist()))


# ------------------------------------------------------------------ 1. equal and zero energies
TIE_NAMES = ["dc", "carrier_tone1", "carrier_tone2", "real_only", "imag_only", "all_zero", "single_tap"]


@pytest.fixture(scope="module")
def tie_set(oracle):
    n = 2 * CHUNK + 12345
    t = np.arange(n)
    sig = impair(oracle.modulate(oracle.bert_frames(3, "TIES", first=17)), amp=9000.0)[: 2 * n].copy()

    def iq(re, im):
        x = np.empty(2 * n, np.int16)
        x[0::2], x[1::2] = re, im
        return x
    tone = 16383.0 * np.exp(2j * np.pi * 13550.0 * t / 2168000.0)
    tap = np.zeros(n, np.int16)
    tap[100003] = 12000
    caps = [np.full(2 * n, 12345, np.int16),
            iq(np.rint(tone.real), np.rint(tone.imag)), iq(np.rint(tone.real), -np.rint(tone.imag)),
            iq(sig[0::2], 0), iq(0, sig[1::2]),
            np.zeros(2 * n, np.int16), iq(tap, -(tap // 2))]
    exp = oracle_all(caps)
    assert len(caps) == len(TIE_NAMES)
    # what the oracle itself says of these inputs: exact ties (soft = +0 between energies of 1e8 and more) while the AFC has not
    # yet turned a one-component input, nothing but zeros on silence and around a lone sample (its two energies round equal)
    for name in ("dc", "real_only", "imag_only"):
        s = exp[TIE_NAMES.index(name)]["soft"]
        assert 2 <= int(np.sum(s == 0.0)) < 10 and s[0] == 0.0 and np.mean(np.abs(s)) > 1e8, name
    for name in ("all_zero", "single_tap"):
        assert np.all(exp[TIE_NAMES.index(name)]["soft"] == 0.0), name
    for name in ("carrier_tone1", "carrier_tone2"):
        s = exp[TIE_NAMES.index(name)]["soft"]
        assert np.all(s != 0.0) and abs(int(np.sum(np.sign(s)))) == s.size, name           # one tone throughout
    assert np.sign(exp[1]["soft"][0]) == -np.sign(exp[2]["soft"][0])
    assert all(e["amb"].size == 0 for e in exp)
    return caps, exp


@pytest.mark.parametrize("shape", SHAPES)
def test_equal_and_zero_energies(amd, tie_set, shared, monkeypatch, shape):
    """held to the oracle as tests/test_gpu_parity.py::test_pathological_inputs_match_the_oracle holds its inputs (frames, metrics,
    events, symbol counts, softs to 1e-8, the offset estimate, the chunk log), the single sample as the one-tap window it is;
    every shape identical to the fp64 ring, and the fp64 ring to itself with the guard forced"""
    caps, exp = tie_set
    ref = shared.fp64(amd, monkeypatch, "ties", caps)
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, caps)[0]
    for name, g, e in zip(TIE_NAMES, got, exp):
        print(f"{shape} {name}: edge_ties {g['state'].edge_ties}, symbols {g['state'].total_symbols}, fo per call {g['chunks'][:, 0]}")
        if name == "single_tap":
            # a one-tap window: both tone energies are |s|^2, the reference's choice is the rounding of its own LO (here it
            # rounds equal: soft = 0 throughout) and no other implementation can follow it. What can be held: the window is
            # REPORTED (edge_ties), the two energies (1.8e8: a square of a sum of a few products, each rounded) part by a few
            # units in their last place (2^-25) at most, in the one or two symbols whose on-time window holds the sample,
            # and nothing else of the stream moves.
            st = g["state"]
            assert st.stalled == 0 and st.edge_ties >= 1 and st.total_symbols == e["n_soft"] == len(g["soft"]), (shape, st.edge_ties)
            assert int(np.sum(g["soft"] != 0.0)) <= 2 and float(np.max(np.abs(g["soft"]))) <= 8 * 2.0 ** -25, (shape, g["soft"][g["soft"] != 0.0])
            assert np.array_equal(g["chunks"][:, 3:], e["chunks"][:, 3:]) and np.allclose(g["chunks"][:, :3], e["chunks"][:, :3], rtol=0, atol=CARRY_ATOL)
            assert len(g["frames"]) == 0 and len(g["events"]) == len(e["events"]) == 0
            continue
        check_capture(amd, g, e, "patho", f"{shape} {name}")
        # a tie is tone 2 and is logged as +0; the tone of every symbol that is clear of the 1e-8 bound
        clear = (e["soft"] == 0.0) | (np.abs(e["soft"]) > 1e-6 * np.mean(np.abs(e["soft"])))
        assert np.array_equal(g["soft"][clear] == 0.0, e["soft"][clear] == 0.0), f"{shape} {name}: where the tones tie"
        assert np.array_equal(np.signbit(g["soft"][clear]), np.signbit(e["soft"][clear])), f"{shape} {name}: signs of the soft symbols"
    for name, g, r in zip(TIE_NAMES, got, ref):
        identical(g, r, f"{name}: {shape} vs fp64 ring")
    if shape == "fp64":
        for name, g, r in zip(TIE_NAMES, run(amd, monkeypatch, "fp64", caps, guard=True)[0], ref):
            identical(g, r, f"{name}: guard forced vs by the rule")


# ------------------------------------------------------------------ 2. the silence test's mask
GAP_AMPS = (6000.0, 4700.0, 7900.0, 3100.0)


def gapped_at_every_amplitude(oracle, iq):
    """hostile_inputs.gapped_capture's recipe (1.2 kHz off tune, gaps of 105 .. 259 exact zeros, an edge moved by three samples
    where the oracle shows a one-tap window: soft = -/+2^-31), with one more demand. A one-tap window whose two energies happen to
    ROUND equal in the reference shows soft = 0 and is invisible to that nudging; the product counts it in edge_ties all the same
    (tests/test_gpu_parity.py::test_many_silence_gaps_signed_zero_rule says why, and allows a handful). Where a window's taps fall
    is decided by the timing loop, which does not see the amplitude; how |s|^2 rounds is. So the same gaps are cut into the
    capture at four amplitudes and nudged until the oracle shows no one-tap window at any of them: one that rounds equal at all
    four is not to be expected, and edge_ties can be asserted 0. -> the capture at the first amplitude, the gaps' starts"""
    bases = [impair(iq, amp=a, f0_hz=1200.0).reshape(-1, 2) for a in GAP_AMPS]
    rng = np.random.default_rng(5)
    pos, gaps = 3000, []
    while pos + 400 < bases[0].shape[0]:
        glen = int(rng.integers(105, 260))
        gaps.append([pos, glen])
        pos += glen + int(rng.integers(1500, 4000))
    for _ in range(400):
        xs = [_zeroed(b.reshape(-1), [(q, q + n) for q, n in gaps]) for b in bases]
        amb = [ambiguous(oracle.receive(x, streaming=True)["soft"]) for x in xs]
        amb = np.concatenate(amb)
        if amb.size == 0:
            return xs[0], [g[0] for g in gaps]
        at = 40 * int(amb.min())
        j = int(np.argmin([min(abs(q - at), abs(q + n - at)) for q, n in gaps]))
        if abs(gaps[j][0] - at) < abs(gaps[j][0] + gaps[j][1] - at):
            gaps[j][0] -= 3; gaps[j][1] += 3
        else:
            gaps[j][1] += 3
    raise AssertionError("could not remove the one-tap windows")


@pytest.fixture(scope="module")
def gap_set(oracle):
    """~90 gaps of a few silent symbols each in a capture 1.2 kHz off tune, no one-tap window at any of four amplitudes"""
    x, starts = gapped_at_every_amplitude(oracle, oracle.modulate(oracle.bert_frames(3, "GAPS", first=5)))
    assert x.size // 2 <= MAX_SAMPLES
    exp = oracle.receive(x, streaming=True)
    exp["amb"] = ambiguous(exp["soft"])
    runs = [r for r in runs_of_zeros(exp["soft"]) if r[0] > 0]
    assert len(starts) >= 60 and len(runs) >= 60 and exp["amb"].size == 0, (len(starts), len(runs))
    short = [n for _, n in runs if n <= 6]                                   # (a gap of 105 .. 259 zeros silences two to six symbols)
    assert len(short) >= 60 and len(set(short)) >= 4, sorted({n for _, n in runs})
    before = np.array([exp["soft"][a - 1] for a, _ in runs])
    assert min(int(np.sum(before < 0)), int(np.sum(before > 0))) >= 15       # gaps behind symbols of either tone
    return x, exp


@pytest.mark.parametrize("shape", SHAPES)
def test_silence_gaps_behind_either_tone(amd, gap_set, shared, monkeypatch, shape):
    x, exp = gap_set
    ref = shared.fp64(amd, monkeypatch, "gaps", [x])[0]
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, [x])[0][0]
    print(f"{shape}: edge_ties {got['state'].edge_ties}")
    check_capture(amd, got, exp, "gap", f"gaps, {shape}")
    assert got["state"].edge_ties == 0, (shape, got["state"].edge_ties)
    assert np.array_equal(got["soft"] == 0.0, exp["soft"] == 0.0)
    identical(got, ref, f"gaps: {shape} vs fp64 ring")
    if shape != "wg4":
        identical(run(amd, monkeypatch, shape, [x], guard=True)[0][0], ref, f"gaps: {shape} with the guard forced vs fp64 ring")


def _zeroed(base, ranges):
    z = base.reshape(-1, 2).copy()
    for a, b in ranges:
        z[a:b] = 0
    return np.ascontiguousarray(z.reshape(-1))


@pytest.fixture(scope="module")
def call_edge_set(oracle):
    """silence where a call begins and ends, each found by moving the zeros' edges until the oracle shows the wanted symbols silent
    and no one-tap window:
      first:  the first symbol of the stream's first call silent, the second one not (it meets a silent predecessor);
      second: the second symbol silent, the first one not;
      call:   a whole silent call, then signal;
      last:   the last symbol of the first call silent (and the first one of the next)"""
    base = impair(oracle.modulate(oracle.bert_frames(2, "EDGES", first=9)), amp=5000.0, f0_hz=-700.0)
    lead = int(np.nonzero(base.reshape(-1, 2).any(axis=1))[0][0]) + 40        # (the modulator's output starts with a few zeros)
    two = base[2 * lead: 2 * (lead + 2 * CHUNK + 4000)]

    def search(make, wanted, span):
        for k in span:
            x = make(k)
            e = oracle.receive(x, streaming=True)
            e["amb"] = ambiguous(e["soft"])
            if e["amb"].size == 0 and wanted(e):
                return x, e
        raise AssertionError("no edge position gives the wanted silent symbols")

    caps, exp = {}, {}
    caps["first"], exp["first"] = search(lambda k: _zeroed(two, [(0, 60 + k)]),
                                         lambda e: e["soft"][0] == 0.0 and np.all(e["soft"][1:20] != 0.0), range(0, 40, 3))
    caps["second"], exp["second"] = search(lambda k: _zeroed(two, [(34 + k, 125 + k)]),
                                           lambda e: e["soft"][0] != 0.0 and e["soft"][1] == 0.0 and np.all(e["soft"][3:20] != 0.0), range(0, 16))
    caps["call"], exp["call"] = search(lambda k: np.ascontiguousarray(np.concatenate([np.zeros(2 * (CHUNK + 3000 + k), np.int16), two])),
                                       lambda e: np.all(e["soft"][: int(e["chunks"][0, 4])] == 0.0) and np.any(e["soft"] != 0.0), range(0, 40, 3))

    def last_silent(e):
        n0 = int(e["chunks"][0, 4])
        return e["soft"][n0 - 1] == 0.0 and e["soft"][n0 - 6] != 0.0
    caps["last"], exp["last"] = search(lambda k: _zeroed(two, [(CHUNK - 150 - k, CHUNK + 80)]), last_silent, range(0, 60, 3))
    assert all(c.size // 2 <= MAX_SAMPLES for c in caps.values())
    assert all(len(e["chunks"]) >= 3 for e in exp.values())
    names = list(caps)
    return names, [caps[k] for k in names], [exp[k] for k in names]


@pytest.mark.parametrize("shape", SHAPES)
def test_silence_at_the_edges_of_calls(amd, call_edge_set, shared, monkeypatch, shape):
    names, caps, exp = call_edge_set
    ref = shared.fp64(amd, monkeypatch, "edges", caps)
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, caps)[0]
    for name, g, e, r in zip(names, got, exp, ref):
        print(f"{shape} {name}: edge_ties {g['state'].edge_ties}, symbols per call {g['chunks'][:, 4]}")
        check_capture(amd, g, e, "gap", f"{name}, {shape}")
        assert len(g["soft"]) == e["n_soft"] and np.array_equal(g["soft"] == 0.0, e["soft"] == 0.0), (shape, name)
        assert np.array_equal(np.signbit(g["chunks"][:, 0]), np.signbit(e["chunks"][:, 0]))
        identical(g, r, f"{name}: {shape} vs fp64 ring")
    if shape != "wg4":
        for name, g, r in zip(names, run(amd, monkeypatch, shape, caps, guard=True)[0], ref):
            identical(g, r, f"{name}: {shape} with the guard forced vs fp64 ring")


# ------------------------------------------------------------------ 3. the soft log at the edges of calls and batches
TAILS = list(range(5, 410, 10))               # samples behind the whole chunk: the tail call sees them + the chunk's leftover


@pytest.fixture(scope="module")
def ends_set(oracle):
    base = oracle.modulate(oracle.bert_frames(2, "NINE", first=21))
    plain = impair(base, amp=3300.0, f0_hz=380.0, ebn0_db=15.0, seed=2402)
    caps = [np.ascontiguousarray(plain[: 2 * (CHUNK + t)]) for t in TAILS]
    exp = oracle_all(caps)
    assert all(len(e["chunks"]) == 2 and e["chunks"][0, 4] == 2167 for e in exp)
    tail_syms = [int(e["chunks"][1, 4]) for e in exp]
    assert set(range(1, 10)) <= set(tail_syms), sorted(set(tail_syms))      # last calls of 1 .. 9 symbols, every slot of two trips
    return caps, exp, tail_syms


@pytest.mark.parametrize("feed", ["whole", "tail_in_its_own_launch"])
def test_last_calls_of_1_to_9_symbols(amd, ends_set, monkeypatch, feed):
    caps, exp, tail_syms = ends_set
    kw = {} if feed == "whole" else dict(first=CHUNK + 3)
    got, rounds = run(amd, monkeypatch, "fp64", caps, **kw)
    assert rounds == (1 if feed == "whole" else 2)
    for k, (g, e) in enumerate(zip(got, exp)):
        check_stream(amd, g, e, f"{feed} stream {k} (last call of {tail_syms[k]} symbols)", edge_ties=0, offset_ties=None)
        assert len(g["soft"]) == e["n_soft"] == 2167 + tail_syms[k]
    ref, _ = run(amd, monkeypatch, "int16", caps, **kw)
    forced, _ = run(amd, monkeypatch, "fp64", caps, guard=True, **kw)
    for k, (g, r, f) in enumerate(zip(got, ref, forced)):
        identical(g, r, f"{feed} stream {k}: fp64 ring vs int16 ring")
        identical(g, f, f"{feed} stream {k}: by the rule vs guard forced")
    pick = [tail_syms.index(n) for n in (1, 2, 3, 4, 5, 6, 7, 9)]           # eight slots: one, a whole trip, two trips and the rest
    wg4, _ = run(amd, monkeypatch, "wg4", [caps[k] for k in pick], **kw)
    for k, g in zip(pick, wg4):
        identical(g, got[k], f"{feed} stream {k}: _rb_wg4 vs fp64 ring")


@pytest.fixture(scope="module")
def ring_set(oracle):
    """four five-frame captures (five calls) whose starts are staggered by 0 .. 3 symbols: the ring's wrap, a fixed symbol count,
    falls on each slot of a trip in turn"""
    base = impair(oracle.modulate(oracle.bert_frames(5, "RING4", first=33)), amp=2700.0, f0_hz=-510.0, ebn0_db=15.0, seed=2410)
    caps = [np.ascontiguousarray(base[2 * 40 * j: 2 * MAX_SAMPLES]) for j in range(4)]
    exp = oracle_all(caps)
    assert all(e["n_soft"] > CAP_SOFT + 2000 and len(e["frames"]) >= 3 for e in exp), [(e["n_soft"], len(e["frames"])) for e in exp]   # a wrap per stream
    return caps, exp


@pytest.mark.parametrize("shape", SHAPES)
def test_smallest_soft_ring_wraps_on_every_slot(amd, ring_set, shared, monkeypatch, shape):
    caps, exp = ring_set
    kw = dict(pieces=WRAP_PIECES, max_samples=SMALL_M)
    ref = shared.fp64(amd, monkeypatch, "ring", caps, **kw)
    got = ref if shape == "fp64" else run(amd, monkeypatch, shape, caps, **kw)[0]
    for k, (g, e, r) in enumerate(zip(got, exp, ref)):
        check_stream(amd, g, e, f"{shape} ring stream {k}", edge_ties=0, offset_ties=None)
        assert len(g["soft"]) == e["n_soft"]
        identical(g, r, f"ring stream {k}: {shape} vs fp64 ring")
    if shape == "fp64":
        for k, (g, r) in enumerate(zip(run(amd, monkeypatch, "fp64", caps, guard=True, **kw)[0], ref)):
            identical(g, r, f"ring stream {k}: guard forced vs by the rule")
