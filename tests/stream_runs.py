"""How the GPU modules RUN streams and gather what they produced, one definition each: making a context on either sample ring,
reading a stream's results in the three shapes the suite uses, the per-stream accumulator of the tests that pop in rounds, the
push sizes that several modules share, and the check of one hostile capture by its class. Bounds are those of
tests/stream_checks.py. Needs no device to import."""
import re
import struct

import numpy as np

from stream_checks import SOFT_TIGHT, check_stream, events_match, soft_err

CHUNK = 86720          # OPV_CHUNK_SAMPLES
HUNTING, VERIFYING, LOCKED = 0, 1, 2
# samples per push and round: one below a symbol (40 samples), odd ones, one chunk -1 / +0 / +1, primes above 100 000,
# multiples of 256 (what the helper wave publishes at a time)
PIECES = [104729, 39, 86719, 262144, 86720, 7919, 86721, 1000003, 256, 20011, 524288, 3]
# the soft ring's wrap (tests/test_gpu_symbol_body.py, tests/test_gpu_batch_boundary.py)
SMALL_M = 150000                              # cap_soft = the power of two >= M / 38 + 4096 = 8192 symbols, the smallest there is
CAP_SOFT = 8192
WRAP_PIECES = [39999, 20011, 7919, 49999, 257, 33333, 40, 45001]
SOFT_HOSTILE = 1e-8     # pathological / gapped captures (the bound their own tests carry)
CARRY_ATOL = 1e-7       # float columns of the chunk log (fo, tf, mu), as everywhere in the suite


# ------------------------------------------------------------------ error codes
def code_of(err):
    """the code an OpvError carries"""
    return int(str(err).split("opv error ")[1].split(":")[0])


def code_raised_by(amd, fn):
    """the code of the OpvError fn() raises, 0 if it raises none"""
    try:
        fn()
    except amd.OpvError as e:
        return int(re.match(r"opv error (-?\d+):", str(e)).group(1))
    return 0


# ------------------------------------------------------------------ contexts and captures
def make_demod(amd, monkeypatch, int16, S, **kw):
    if int16:
        monkeypatch.setenv("OPV_FRONTEND_INT16_RING", "1")
    else:
        monkeypatch.delenv("OPV_FRONTEND_INT16_RING", raising=False)
    try:
        return amd.Demod(S, **kw)
    finally:
        monkeypatch.delenv("OPV_FRONTEND_INT16_RING", raising=False)


def base_capture(amd, frames=3, seed=0, sigma=300.0):
    iq = amd.modulate(amd.bert_frames(frames)).astype(np.float64)
    rng = np.random.default_rng(seed)
    return np.clip(np.rint(iq + sigma * rng.standard_normal(iq.shape)), -32768, 32767).astype(np.int16)


# ------------------------------------------------------------------ one stream's results
def state_tuple(st):
    # floats by their bits: est_offset_hz is NaN where no offset search ran, and NaN != NaN
    return tuple(struct.pack("<d", v) if isinstance(v, float) else v for v in (getattr(st, f) for f, _ in st._fields_))


def collect(d, k):
    """for check_stream: the state as the binding's object"""
    fr, meta = d.pop_frames(k)
    return dict(frames=fr, meta=meta, events=d.pop_events(k), soft=d.soft(k), state=d.state(k), chunks=d.chunks(k))


def collect_bits(d, s):
    """for assert_same: the state as state_tuple"""
    fr, meta = d.pop_frames(s)
    return dict(frames=fr, meta=meta, events=d.pop_events(s), soft=d.soft(s), state=state_tuple(d.state(s)), chunks=d.chunks(s))


def collect_unstalled(d, s):
    """collect_bits of a stream that must not be stalled, with the symbol count and the state's fields as a list (picklable)"""
    fr, meta = d.pop_frames(s)               # (fails on a stream in an error state: overflow != 0)
    st = d.state(s)
    assert st.stalled == 0, (s, st.stalled)
    return dict(frames=fr, meta=meta, events=d.pop_events(s), soft=d.soft(s), state=state_tuple(st), chunks=d.chunks(s),
                total_symbols=int(st.total_symbols), st=[getattr(st, f) for f, _ in st._fields_])


def assert_same(a, b, what):
    assert a["state"] == b["state"], what
    for k in ("soft", "chunks", "frames", "meta", "events"):
        x, y = a[k], b[k]
        assert x.shape == y.shape, (what, k)
        assert x.tobytes() == y.tobytes(), (what, k)      # bit for bit (NaN-safe, -0.0 distinct)


def explain(d, k, got, exp, tag):
    """what a mismatch is diagnosed from: where the soft symbols part, in which demodulate() call, on which wave"""
    a, b = got["soft"], exp["soft"]
    m = min(len(a), len(b))
    bad = np.nonzero(np.abs(a[:m] - b[:m]) > SOFT_TIGHT * (np.mean(np.abs(b)) + 1e-300))[0]
    first = int(bad[0]) if bad.size else None
    call = None if first is None else int(np.searchsorted(np.cumsum(exp["chunks"][:, 4]), first, side="right"))
    st = got["state"]
    hw_id, xcc_id, _cycles, _ticks = d.wave_info(k)
    print(f"{tag}: MISMATCH. symbols {len(a)} (oracle {len(b)}), {bad.size} soft symbols off, first at {first} (demodulate() call {call} of "
          f"{len(exp['chunks'])}); frames {len(got['frames'])} (oracle {len(exp['frames'])}); stalled 0x{st.stalled:x}, chunk_origin "
          f"{st.chunk_origin}, n_chunks {st.n_chunks}; dbg_hw_id 0x{hw_id:x}, dbg_xcc_id {xcc_id}")


# ------------------------------------------------------------------ what a test keeps per stream over many rounds
def new_acc():
    return dict(frames=[], meta=[], events=[], soft=[], chunks=[], n_soft=0, n_chunks=0)


def drain(d, k, acc, pop=True, soft=True):
    """append what stream k of context d has produced since the last drain (the taps are absolute: nothing is read twice)"""
    if pop:
        f, m = d.pop_frames(k)
        acc["frames"].append(f)
        acc["meta"].append(m)
        acc["events"].append(d.pop_events(k))
    st = d.state(k)
    if soft and st.total_symbols > acc["n_soft"]:
        s = d.soft(k, first=acc["n_soft"])
        assert len(s) == st.total_symbols - acc["n_soft"]
        acc["soft"].append(s)
        acc["n_soft"] = st.total_symbols
    if st.n_chunks > acc["n_chunks"]:
        c = d.chunks(k, first=acc["n_chunks"])
        assert len(c) == st.n_chunks - acc["n_chunks"]
        acc["chunks"].append(c)
        acc["n_chunks"] = st.n_chunks
    return st


def result(amd, d, k, acc):
    st = drain(d, k, acc)
    cat = lambda xs, empty: np.concatenate(xs) if xs else empty
    return dict(frames=cat(acc["frames"], np.zeros((0, 134), np.uint8)), meta=cat(acc["meta"], np.zeros(0, amd.META_DTYPE)),
                events=cat(acc["events"], np.zeros(0, amd.EVENT_DTYPE)), soft=cat(acc["soft"], np.zeros(0)),
                chunks=cat(acc["chunks"], np.zeros((0, 5))), state=st)


def held_to_the_oracle(amd, d, k, acc, exp, tag, offset_ties=0):
    got = result(amd, d, k, acc)
    assert got["state"].stalled == 0, tag
    check_stream(amd, got, exp, tag, edge_ties=0, offset_ties=offset_ties)
    assert got["state"].frames_decoded == len(exp["frames"]) and got["state"].frames_perfect == int(np.sum(exp["metrics"] == 0)), tag
    return got


def feed(d, k, x, lo, hi, acc, pop=True, piece=40000):
    """samples [lo, hi) of capture x into stream k in pieces, a round after each"""
    for o in range(lo, hi, piece):
        d.push(k, x[2 * o: 2 * min(o + piece, hi)])
        d.process()
        drain(d, k, acc, pop=pop)


def tracker_at(exp, n_sym):
    """where the ORACLE's tracker stands once it has consumed n_sym symbols: 'hunting', 'verifying', 'collecting' (LOCKED, a payload
    pending release), 'miss-collecting' (the same behind a sync MISS: the pending frame is a flywheel frame) or 'between' (LOCKED,
    the last payload released, the next sync check not made yet)"""
    ev = [e for e in exp["events"] if e["sym_idx"] < n_sym]
    if not ev or ev[-1]["kind"] == 5:
        return "hunting"
    if ev[-1]["kind"] == 1:
        return "verifying"
    last = ev[-1]
    if last["kind"] == 2:                                   # VERIFYING -> LOCKED is printed AT the first release
        return "between"
    released = int(last["sym_idx"]) + 2144 in [int(r) for r in exp["frame_sym"] if r < n_sym]
    if released:
        return "between"
    return "miss-collecting" if last["kind"] == 4 else "collecting"


# ------------------------------------------------------------------ the check of one hostile capture
def check_capture(amd, got, exp, cls, tag, streaming=True):
    """One stream against the oracle's result for its capture, by the capture's class (tests/test_gpu_mapping_matrix.py's
    docstring); -> its soft error."""
    st = got["state"]
    assert st.stalled == 0, f"{tag}: stalled 0x{st.stalled:x}"
    if cls == "full":
        check_stream(amd, got, exp, tag, edge_ties=0, offset_ties=None)
        return soft_err(got["soft"], exp["soft"])[0]
    n_soft = exp["n_soft"]
    # up to the oracle's first one-tap window. In -s mode only the un-nudged capture is cut short by that: the nudged one has none,
    # and the pathological ones are compared in full, as test_pathological_inputs_match_the_oracle compares them (its capture 5,
    # the signal that stops and resumes, has one such window at symbol 4249, after which that test holds the product to 1e-8 too)
    cut = exp["amb"].size and not (cls == "patho" and streaming)
    k_end = int(exp["amb"][0]) if cut else n_soft
    assert st.total_symbols == n_soft and len(got["soft"]) == n_soft, f"{tag}: {st.total_symbols} symbols, oracle {n_soft}"
    scale = np.mean(np.abs(exp["soft"])) + 1e-300
    a = float(np.max(np.abs(got["soft"][:k_end] - exp["soft"][:k_end]))) / scale if k_end else 0.0
    assert a < SOFT_HOSTILE, f"{tag}: soft error {a:.3e} before symbol {k_end}"
    e0, e1 = st.est_offset_hz, exp["est_offset"]
    assert (np.isnan(e0) and np.isnan(e1)) or e0 == e1, f"{tag}: offset estimate {e0} vs {e1}"
    ch, ech = got["chunks"], exp["chunks"]
    done = np.nonzero(np.cumsum(ech[:, 4]) <= k_end)[0]                    # demodulate() calls that ended before k_end
    assert len(ch) >= done.size, f"{tag}: {len(ch)} chunk rows"
    for c in done:
        assert np.array_equal(ch[c, 3:], ech[c, 3:]), f"{tag}: call {c}: leftover / symbols {ch[c, 3:]} vs {ech[c, 3:]}"
        assert np.allclose(ch[c, :3], ech[c, :3], rtol=0, atol=CARRY_ATOL), f"{tag}: call {c}: {ch[c]} vs {ech[c]}"
    if cls == "tie" and exp["amb"].size:
        assert st.edge_ties >= 1, f"{tag}: the oracle shows {exp['amb'].size} one-tap windows, edge_ties {st.edge_ties}"
    if cls == "gap":
        assert st.edge_ties <= 12, f"{tag}: edge_ties {st.edge_ties} on the nudged capture"
    if k_end == n_soft:                                                    # nothing ambiguous: every decision too
        assert ch.shape == ech.shape, f"{tag}: chunk log {ch.shape} vs {ech.shape}"
        assert np.array_equal(got["frames"], exp["frames"]), f"{tag}: decoded bytes differ"
        assert np.array_equal(got["meta"]["viterbi_metric"], exp["metrics"]), f"{tag}: Viterbi metrics differ"
        assert np.array_equal(got["meta"]["release_symbol"], exp["frame_sym"]), f"{tag}: sync positions differ"
        events_match(amd, got["events"], exp["events"])
        assert abs(st.freq_offset_hz - exp["final_freq_offset"]) < 1e-6 and st.sync_state == exp["final_state"], tag
    return a
