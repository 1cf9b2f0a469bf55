"""GPU: a receive stream at far positions - absolute symbol and sample indices across 2^31, 2^32 and beyond 2^40 - held to the
oracle. At 2 168 000 S/s a stream's sample count passes 2^31 after 16.5 minutes and 2^32 after 33, its symbol count after 11 and 22
hours; the suite reaches those positions in milliseconds through the migration blob: a stream exported from an ordinary short run
has every absolute index of its carry moved forward by a constant (tests/stream_rules_probe.cpp: probe_blob_shift, compiled against
csrc/opv_stream_rules.h) and is imported again. The reference's behaviour does not depend on the absolute counts except through the
index it prints and through ksym & 3 in the signed-zero rule, and the shifts are multiples of 4: so the oracle's result for the
UNSHIFTED capture, with the shift added to every index reported after the import, is the exact expectation.

Run shape of every case: the first `cut` samples go into a 1-stream source context in 40 000-sample pieces, a round after each, and
what they produced is kept; export, shift, import into slot 5 of a fresh 20-stream destination whose slots 4 and 6 serve two
ordinary streams from their first sample on (they must not notice: both are held to the oracle too); the rest in 40 000-sample
pieces, a round after each; everything drained with absolute indices. Held with check_stream's own bounds (frames, metrics, release
symbols, event lines ==; soft symbols < SOFT_TIGHT; estimate ==; chunk log) plus stalled == 0 and edge_ties == 0; the silence-gap
capture with its own class (1e-8, chunk log 1e-7, edge_ties <= 12). After EVERY round the stream's total_symbols, total_samples and
chunk_origin must be what the oracle's own call schedule (its leftovers) says, plus the shift.

Control: the same schedule with both shifts 0 into the same kind of destination. A stream's arithmetic depends on ring positions
only through where results are stored, so soft symbols, chunk log, AFC / timing state, frames and metrics of the shifted run must
be the SAME BITS, and every reported index must differ by exactly the shift.

Every placement ("symbol 2^32 in the middle of the second call after the import") is asserted from the oracle's numbers before the
product sees a sample. Two cases deviate from a 40 000-sample schedule because what they are about cannot happen in one:
payload_2p32 feeds the rest in 300 000-sample pieces (three frames decoded in one round: the decoder pairs two of them in a wave),
and hunting_window_2p32 is cut at 100 000 samples of the capture whose first sync word lies at symbol 2177 - a stream cut at
50 000 samples has produced no symbol yet, which the shift refuses (test_refusals)."""
import struct

import numpy as np
import pytest

from far_probe import probe, shifted_blob  # noqa: F401
from fixtures import amd  # noqa: F401
from link_model import CODED, check_record, link_model
from oracle_lib import accidents, impair
from stream_checks import _gapped_capture, events_match, soft_err
from stream_runs import (CHUNK, HUNTING, LOCKED, drain, feed, held_to_the_oracle, make_demod, new_acc, result, state_tuple,
                         tracker_at)

pytestmark = pytest.mark.gpu
EINVAL = -1
SLOT = 5
NEIGHBOURS = (("shifted", 4), ("noisy", 6))
CUT = 2 * CHUNK + 20000
# (id, int16 ring forced, opv_set_frontend, the kernel a round must have launched)
DESTS = [("rb_f64", False, 1, "k_msk_frontend_rb"), ("rb_i16", True, 1, "k_msk_frontend_rb"), ("x4", False, 4, "k_msk_frontend_x4_wg4"),
         ("x16", False, 16, "k_msk_frontend_x16_wg4")]


@pytest.fixture(scope="module")
def caps(oracle, iq10):
    """the captures of this file and the oracle's result for each, with its call schedule (computed once, never changed)"""
    iq8 = oracle.modulate(oracle.bert_frames(8))
    c = {"noisy": impair(iq8, amp=2000.0, f0_hz=1200.0, ebn0_db=14.0, seed=5), "shifted": iq8[2 * 560:]}
    rng = np.random.default_rng(7009)
    c["accident"], _ = accidents(impair(iq10, amp=3000.0, f0_hz=-700.0, ebn0_db=15.0, seed=79), rng, 3000.0, n_max=2)
    c["gapped"] = _gapped_capture(oracle, iq10)[0]
    exp = {}
    for k, x in c.items():
        e = oracle.receive(x, streaming=True)
        e["amb"] = np.nonzero((e["soft"] != 0) & (np.abs(e["soft"]) < 1.0))[0]
        e["n"] = x.size // 2
        # the reference's chunker (src/opv-demod.cpp:1070-1076): call c reads samples [starts[c], starts[c] + 86720), the next
        # one starts `leftover` samples in front of its end; the last call is the tail behind the last full chunk
        starts = [0]
        for row in e["chunks"][:-1]:
            lo = int(row[3])
            starts.append(starts[-1] + (CHUNK - lo if 0 < lo < CHUNK else CHUNK))
        e["starts"] = np.array(starts, np.int64)
        e["cum"] = np.cumsum(e["chunks"][:, 4]).astype(np.int64)
        e["n_full"] = len(starts) - 1
        assert e["starts"][e["n_full"] - 1] + CHUNK <= e["n"] < e["starts"][e["n_full"]] + CHUNK and e["n"] > e["starts"][-1]
        exp[k] = e
    assert exp["gapped"]["amb"].size == 0
    return c, exp


def calls_done(e, avail):
    """full demodulate() calls the oracle has made once `avail` samples have arrived"""
    return int(np.sum(e["starts"][:e["n_full"]] + CHUNK <= avail))


def symbols_done(e, calls):
    return int(e["cum"][calls - 1]) if calls else 0


def call_of(e, sym):
    """the demodulate() call that produces symbol `sym`"""
    return int(np.searchsorted(e["cum"], sym, side="right"))


def shift_to(power, target):
    """the multiple of 4 that moves index B to 2^power, for the B in [target, target + 3] that allows one"""
    return ((1 << power) - target) & ~3


def sample_shift(e, c, power):
    """sample 2^power into the middle of call c's span: total_samples steps across it when call c ends, and so does chunk_origin"""
    d = shift_to(power, int(e["starts"][c]) + CHUNK // 2)
    p = (1 << power) - d
    assert c * CHUNK < p <= (c + 1) * CHUNK and e["starts"][c] <= p < e["starts"][c + 1], (c, p)
    return d


# ---- the cases: (run options, d_sym, d_samp), every placement asserted from the oracle's numbers ------------------------------
def plan(case, exps):
    noisy = exps["noisy"]
    k0 = calls_done(noisy, CUT)                               # calls made at the source
    assert k0 == 2 and noisy["n_full"] >= k0 + 4
    if case in ("call_2p32", "call_2p31", "moved_again", "compaction_2p32"):
        power = 31 if case == "call_2p31" else 32
        c = k0 + 1                                              # the second call after the import
        d_sym = shift_to(power, symbols_done(noisy, c) + int(noisy["chunks"][c, 4]) // 2)
        b = (1 << power) - d_sym
        assert symbols_done(noisy, c) + 1000 < b < symbols_done(noisy, c + 1) - 1000
        opt = dict(cap="noisy", cut=CUT)
        if case == "moved_again":
            opt.update(again=c + 1)                             # moved on once call c has been made
        if case == "compaction_2p32":
            opt.update(max_samples=3 * CHUNK + 40000, iq=True)
        return opt, d_sym, sample_shift(noisy, c, power)
    if case == "beyond_2p40":
        return dict(cap="noisy", cut=CUT, pop_src=False), (1 << 40) + 8, (1 << 40) + 4
    if case == "payload_2p32":
        piece = 300000
        n_cut, n_round = symbols_done(noisy, k0), symbols_done(noisy, calls_done(noisy, CUT + piece))
        fs = noisy["frame_sym"].astype(np.int64)
        j0 = int(np.sum(fs < n_cut))                            # first frame decoded at the destination: the wave's frame A
        in_round = int(np.sum((fs >= n_cut) & (fs < n_round)))
        assert j0 >= 1 and in_round >= 3 and in_round % 2 == 1, (j0, in_round)
        d_sym = shift_to(32, int(fs[j0 + 1]) - 2143 + 1000)
        b = (1 << 32) - d_sym
        assert fs[j0] < b and fs[j0 + 1] - 2143 + 999 < b < fs[j0 + 1] - 1000      # A's payload in front of it, B's across it
        assert b > n_cut
        return dict(cap="noisy", cut=CUT, link=True, piece=piece), d_sym, sample_shift(noisy, call_of(noisy, b), 32)
    if case == "locked_window_2p32":
        ev = noisy["events"]
        s = int(ev["sym_idx"][(ev["kind"] == 3) & (ev["sym_idx"] > symbols_done(noisy, k0 + 1))][0])
        d_sym = shift_to(32, s - 12)
        b = (1 << 32) - d_sym
        assert s - 23 < b < s and tracker_at(noisy, s) != "hunting"
        return dict(cap="noisy", cut=CUT), d_sym, sample_shift(noisy, call_of(noisy, b), 32)
    if case == "hunting_window_2p32":
        e = exps["shifted"]
        cut = 100000
        n_cut = symbols_done(e, calls_done(e, cut))
        first = e["events"][0]
        s = int(first["sym_idx"])
        assert n_cut >= 24 and first["kind"] == 1 and tracker_at(e, n_cut) == "hunting" and n_cut <= s - 9
        d_sym = shift_to(32, s - 12)
        b = (1 << 32) - d_sym
        assert s - 23 < b < s and b >= n_cut                    # (the count crosses after the import, inside the 24-symbol window)
        return dict(cap="shifted", cut=cut, state=HUNTING), d_sym, sample_shift(e, call_of(e, b), 32)
    if case == "flywheel_2p32":
        e = exps["accident"]
        cut = 4 * CHUNK + 20000
        n_cut = symbols_done(e, calls_done(e, cut))
        ev = e["events"]
        s = int(ev["sym_idx"][ev["kind"] == 4][0])
        assert s > n_cut and s + 2144 in e["frame_sym"].astype(np.int64)            # the MISS, and the flywheel frame it leads to
        d_sym = shift_to(32, s + 1072)
        b = (1 << 32) - d_sym
        assert s < b < s + 2144 and tracker_at(e, b) == "miss-collecting"
        return dict(cap="accident", cut=cut), d_sym, sample_shift(e, call_of(e, b), 32)
    if case == "gap_edge_2p32":
        e = exps["gapped"]
        n_cut = symbols_done(e, calls_done(e, CUT))
        z = e["soft"] == 0
        lead = np.nonzero(z[1:] & ~z[:-1])[0] + 1               # first silent symbol of every gap
        k = int(lead[lead > n_cut + 2168][0])
        d_sym = shift_to(32, k)
        b = (1 << 32) - d_sym
        assert e["soft"][k - 1] != 0 and e["soft"][k] == 0 and k <= b < k + 40
        return dict(cap="gapped", cut=CUT, cls="gap"), d_sym, sample_shift(e, call_of(e, b), 32)
    raise KeyError(case)


CASES = ["call_2p32", "call_2p31", "payload_2p32", "locked_window_2p32", "hunting_window_2p32", "flywheel_2p32", "gap_edge_2p32",
         "compaction_2p32", "beyond_2p40", "moved_again"]


# ---- one run --------------------------------------------------------------------------------------------------------------------
def make_dest(amd, monkeypatch, dest, max_samples):
    _, int16, per_wave, _ = dest
    d = make_demod(amd, monkeypatch, int16, 20, max_samples=max_samples, streaming=True)
    d.set_frontend(per_wave)
    return d


def drain_main(d, k, acc, pop, links):
    if pop and links is not None:
        f, m, r = d.pop_frames(k, link=True)
        acc["frames"].append(f)
        acc["meta"].append(m)
        acc["events"].append(d.pop_events(k))
        links.append(r)
        pop = False
    return drain(d, k, acc, pop=pop)


def check_round(e, st, pushed, d_sym, d_samp, tag):
    """the stream's counters after a round against the oracle's call schedule"""
    k = st.n_chunks
    if st.flushed:
        total = e["n_full"] * CHUNK + (e["n"] - int(e["starts"][-1]))
        assert k == len(e["chunks"]) and st.total_symbols == e["n_soft"] + d_sym and st.total_samples == total + d_samp, (tag, k)
        return
    assert k == calls_done(e, pushed), (tag, k, pushed)
    assert st.total_symbols == symbols_done(e, k) + d_sym, (tag, k, st.total_symbols)
    assert st.total_samples == k * CHUNK + d_samp, (tag, k, st.total_samples)
    assert st.chunk_origin == int(e["starts"][k]) + d_samp, (tag, k, st.chunk_origin)


def run(amd, monkeypatch, probe, caps, opt, dest, d_sym, d_samp, tag):
    """-> dict(main, trace, neighbours, links, n_src): what the moved stream and its two neighbours produced"""
    xs, exps = caps
    x, e = xs[opt["cap"]], exps[opt["cap"]]
    n, cut, piece = e["n"], opt["cut"], opt.get("piece", 40000)
    acc = new_acc()
    src = amd.Demod(1, max_samples=n + 64, streaming=True)
    feed(src, 0, x, 0, cut, acc, pop=opt.get("pop_src", True))
    st = src.state(0)
    n_cut = symbols_done(e, calls_done(e, cut))
    assert st.total_symbols == n_cut and st.stalled == 0 and st.sync_state == opt.get("state", LOCKED), (tag, st.total_symbols)
    check_round(e, st, cut, 0, 0, tag)
    n_src = dict(frames=sum(len(f) for f in acc["frames"]), events=sum(len(v) for v in acc["events"]), symbols=n_cut)
    rc, blob = shifted_blob(probe, src.export_streams([0]), d_sym, d_samp)
    src.close()
    assert rc == 0, (tag, rc)
    M = opt.get("max_samples") or max(v["n"] for v in exps.values()) + 64
    dst = make_dest(amd, monkeypatch, dest, M)
    others = []
    try:
        links = [] if opt.get("link") else None
        if links is not None:
            dst.enable_link_report()
        dst.import_streams([SLOT], blob)
        acc["n_soft"] += d_sym
        st2 = dst.state(SLOT)
        check_round(e, st2, cut, d_sym, d_samp, tag)
        assert st2.sync_state == st.sync_state and st2.n_chunks == st.n_chunks and st2.frames_released == st.frames_released
        cur, pop, pos, flushed, trace, edge = dst, "again" not in opt, cut, False, [], []
        origin = st2.chunk_origin
        naccs = [new_acc() for _ in NEIGHBOURS]
        npos = [0 for _ in NEIGHBOURS]
        ndone = [False for _ in NEIGHBOURS]
        rounds = 0
        while not (flushed and all(ndone)):
            if pos < n:
                hi = min(pos + piece, n)
                cur.push(SLOT, x[2 * pos: 2 * hi])
                pos = hi
                if opt.get("iq"):
                    # what the device buffer holds, by ABSOLUTE sample index: from 16 samples in front of the chunk origin (what
                    # compaction always keeps) to the last sample pushed; and the eight samples around sample 2^32
                    first = origin - 16
                    got = cur.iq(SLOT, first=first)
                    assert got.size and np.array_equal(got, x[2 * (first - d_samp): 2 * pos]), (tag, first, got.size)
                    at = (1 << 32) - 4
                    got = cur.iq(SLOT, first=at, cap=8)
                    assert np.array_equal(got, x[2 * (at - d_samp): 2 * min(at - d_samp + 8, pos)][:got.size]), (tag, rounds)
                    edge.append((got.size // 2, origin))
            elif not flushed:
                cur.flush(SLOT)
                flushed = True
            for i, (name, s) in enumerate(NEIGHBOURS):
                if npos[i] < exps[name]["n"]:
                    hi = min(npos[i] + 40000, exps[name]["n"])
                    dst.push(s, xs[name][2 * npos[i]: 2 * hi])
                    npos[i] = hi
                elif not ndone[i]:
                    dst.flush(s)
                    ndone[i] = True
            dst.process()
            if cur is not dst:
                cur.process()
            if rounds == 0:
                assert dst.frontend_kernel() == dest[3], (tag, dst.frontend_kernel())
            st = drain_main(cur, SLOT, acc, pop, links)
            check_round(e, st, pos, d_sym, d_samp, tag)
            trace.append((st.n_chunks, st.total_symbols, st.total_samples, st.chunk_origin, st.frames_released))
            origin = st.chunk_origin
            for (name, s), na in zip(NEIGHBOURS, naccs):
                drain(dst, s, na)
            if "again" in opt and cur is dst and st.n_chunks >= opt["again"]:
                # far indices inside SEG_FREC / SEG_EVENTS and in soft_first: frames and events unpopped since the import
                assert st.frames_released > n_src["frames"] and (d_sym == 0 or (st.total_symbols > 1 << 32 and st.total_samples > 1 << 32)), (tag, trace[-1])
                nxt = DESTS[(DESTS.index(dest) + 1) % len(DESTS)]
                cur = make_dest(amd, monkeypatch, nxt, M)
                others.append((cur, nxt))
                cur.import_streams([SLOT], dst.export_streams([SLOT]))
                dst.reset(SLOT)
                pop = True
            rounds += 1
        for cur2, nxt in others:
            assert cur2.frontend_kernel() == nxt[3], (tag, cur2.frontend_kernel())
        if opt.get("iq") and d_samp:
            # iq_base itself stepped across sample 2^32 in a compaction: the samples around it were there, and then were dropped
            held = [i for i, (got, _) in enumerate(edge) if got]
            assert held and edge[held[0]][0] == 8 and any(got == 0 and o > 1 << 32 for got, o in edge[held[-1] + 1:]), (tag, edge)
        out = dict(trace=trace, links=links, n_src=n_src, acc=acc, ctx=cur, dst=dst, naccs=naccs)
        return out
    except BaseException:
        for c, _ in others:
            c.close()
        dst.close()
        raise


def close(out):
    if out["ctx"] is not out["dst"]:
        out["ctx"].close()
    out["dst"].close()


def far_expectation(e, n_src, d_sym, all_late):
    """the oracle's result with every index reported after the import moved forward (all_late: nothing was popped at the source, so
    every frame record and event travelled in the blob and was moved with it)"""
    f = dict(e)
    lo = 0 if all_late else n_src["symbols"]
    f["events"] = e["events"].copy()
    late = f["events"]["sym_idx"] >= lo
    f["events"]["sym_idx"][late] += np.uint64(d_sym)
    f["frame_sym"] = e["frame_sym"].copy()
    f["frame_sym"][f["frame_sym"] >= lo] += np.uint64(d_sym)
    f["n_soft"] = e["n_soft"] + d_sym
    if not all_late:
        assert int(np.sum(e["frame_sym"] < lo)) == n_src["frames"] and int(np.sum(e["events"]["sym_idx"] < lo)) == n_src["events"]
    return f


def check_gapped(amd, got, e, tag):
    """the silence-gap capture's own class, as test_many_silence_gaps_signed_zero_rule and the mapping matrix hold it: soft symbols
    within 1e-8 of their mean, the carry of every demodulate() call within 1e-7, at most 12 windows counted as edge ties; the nudged
    capture holds no one-tap window, so every decision is compared too; -> the soft error"""
    st = got["state"]
    assert st.stalled == 0 and st.edge_ties <= 12, (tag, st.stalled, st.edge_ties)
    assert st.total_symbols == e["n_soft"] and got["soft"].shape == e["soft"].shape, tag
    a = float(np.max(np.abs(got["soft"] - e["soft"]))) / (np.mean(np.abs(e["soft"])) + 1e-300)
    assert a < 1e-8, f"{tag}: soft error {a:.3e}"
    assert st.est_offset_hz == e["est_offset"], tag
    assert got["chunks"].shape == e["chunks"].shape and np.array_equal(got["chunks"][:, 3:], e["chunks"][:, 3:]), tag
    for c in range(len(e["chunks"])):
        assert np.allclose(got["chunks"][c, :3], e["chunks"][c, :3], rtol=0, atol=1e-7), (tag, c, got["chunks"][c], e["chunks"][c])
    assert np.array_equal(got["frames"], e["frames"]) and np.array_equal(got["meta"]["viterbi_metric"], e["metrics"]), tag
    assert np.array_equal(got["meta"]["release_symbol"], e["frame_sym"]), tag
    events_match(amd, got["events"], e["events"])
    assert abs(st.freq_offset_hz - e["final_freq_offset"]) < 1e-6 and st.sync_state == e["final_state"], tag
    return a


def held(amd, out, caps, opt, d_sym, tag):
    """the moved stream and both neighbours against the oracle; -> their results"""
    xs, exps = caps
    e = far_expectation(exps[opt["cap"]], out["n_src"], d_sym, not opt.get("pop_src", True))
    if opt.get("cls") == "gap":
        got = result(amd, out["ctx"], SLOT, out["acc"])
        a = check_gapped(amd, got, e, tag)
    else:
        got = held_to_the_oracle(amd, out["ctx"], SLOT, out["acc"], e, tag, offset_ties=None)
        a = soft_err(got["soft"], e["soft"])[0]
    print(f"FAR {tag}: soft max|d|/mean|soft| = {a:.3e}")
    assert np.array_equal(got["meta"]["payload_symbol"], e["frame_sym"] - np.uint64(2143)), tag
    neigh = [held_to_the_oracle(amd, out["dst"], s, na, exps[name], f"{tag} neighbour {name}", offset_ties=None)
             for (name, s), na in zip(NEIGHBOURS, out["naccs"])]
    return got, neigh


_CONTROL = {}


def control(amd, monkeypatch, probe, caps, opt, dest):
    """the same schedule with both shifts 0 (computed once per schedule and destination, shared, never changed)"""
    key = (tuple(sorted(opt.items())), dest[0])
    if key not in _CONTROL:
        tag = f"control {sorted(opt.items())} {dest[0]}"
        out = run(amd, monkeypatch, probe, caps, opt, dest, 0, 0, tag)
        try:
            got, neigh = held(amd, out, caps, opt, 0, tag)
        finally:
            close(out)
        _CONTROL[key] = (got, neigh, out["trace"], out["links"])
    return _CONTROL[key]


def bits(v):
    return struct.pack("<d", v)


def same_but_shifted(far, ctl, n_src, d_sym, d_samp, all_late, tag):
    (got, neigh, trace, links), (got0, neigh0, trace0, links0) = far, ctl
    for k in ("soft", "chunks", "frames"):
        assert got[k].shape == got0[k].shape and got[k].tobytes() == got0[k].tobytes(), (tag, k)
    nf, ne = (0, 0) if all_late else (n_src["frames"], n_src["events"])
    for k in ("viterbi_metric", "sync_ok", "sync_quality"):
        assert got["meta"][k].tobytes() == got0["meta"][k].tobytes(), (tag, k)
    for k in ("release_symbol", "payload_symbol"):
        a, b = got["meta"][k].astype(object), got0["meta"][k].astype(object)
        assert list(a[:nf]) == list(b[:nf]) and list(a[nf:]) == [v + d_sym for v in b[nf:]], (tag, k)
    for k in ("kind", "count", "corr", "raw"):
        assert got["events"][k].tobytes() == got0["events"][k].tobytes(), (tag, k)
    a, b = got["events"]["sym_idx"].astype(object), got0["events"]["sym_idx"].astype(object)
    assert list(a[:ne]) == list(b[:ne]) and list(a[ne:]) == [v + d_sym for v in b[ne:]], tag
    s, s0 = got["state"], got0["state"]
    for k in ("freq_offset_hz", "timing_freq", "mu", "est_offset_hz"):
        assert bits(getattr(s, k)) == bits(getattr(s0, k)), (tag, k)
    for k in ("sync_state", "frames_released", "frames_decoded", "frames_perfect", "n_chunks", "flushed", "events_dropped", "edge_ties", "stalled", "offset_ties"):
        assert getattr(s, k) == getattr(s0, k), (tag, k)
    assert (s.total_symbols, s.total_samples, s.chunk_origin) == (s0.total_symbols + d_sym, s0.total_samples + d_samp, s0.chunk_origin + d_samp), tag
    assert trace == [(c, sym + d_sym, tot + d_samp, org + d_samp, fr) for c, sym, tot, org, fr in trace0], tag
    if links is not None:
        assert np.concatenate(links).tobytes() == np.concatenate(links0).tobytes(), tag
    for g, g0 in zip(neigh, neigh0):                            # the neighbours: the same bits, indices included
        assert state_tuple(g["state"]) == state_tuple(g0["state"]), tag
        for k in ("soft", "chunks", "frames", "meta", "events"):
            assert g[k].tobytes() == g0[k].tobytes(), (tag, "neighbour", k)


@pytest.mark.parametrize("dest", DESTS, ids=[d[0] for d in DESTS])
@pytest.mark.parametrize("case", CASES)
def test_far_positions(amd, oracle, probe, caps, monkeypatch, case, dest):
    opt, d_sym, d_samp = plan(case, caps[1])
    assert d_sym % 4 == 0 and d_samp % 4 == 0 and d_sym >= 1 << 30 and d_samp >= 1 << 30
    tag = f"{case} {dest[0]}"
    ctl = control(amd, monkeypatch, probe, caps, opt, dest)
    out = run(amd, monkeypatch, probe, caps, opt, dest, d_sym, d_samp, tag)
    try:
        got, neigh = held(amd, out, caps, opt, d_sym, tag)
        if opt.get("link"):
            # the records of the frames decoded at the destination: the integers against the model over the ORACLE's payloads, and
            # the whole record (m1 ==, m2 / ma within their bound) as test_from_iq_three_streams holds it - against the model over
            # the device's own soft symbols, read back here by their far indices (m1 is a sum in index order: == needs the same terms)
            e = caps[1][opt["cap"]]
            rec = np.concatenate(out["links"])
            nf = out["n_src"]["frames"]
            assert len(rec) == len(got["frames"]) - nf == len(e["frames"]) - nf and rec["valid"].all(), tag
            for j in range(len(rec)):
                ps = int(got["meta"]["payload_symbol"][nf + j])
                assert ps == int(e["frame_sym"][nf + j]) - 2143 + d_sym
                m = link_model(oracle, e["soft"][ps - d_sym: ps - d_sym + CODED])
                for k in ("valid", "bit_errors", "weak", "nonfinite"):
                    assert int(rec[j][k]) == m[k], (tag, j, k)
                assert np.array_equal(m["frame"], got["frames"][nf + j]) and m["metric"] == got["meta"]["viterbi_metric"][nf + j], (tag, j)
                own = out["ctx"].soft(SLOT, first=ps, cap=CODED)
                assert own.tobytes() == got["soft"][ps - d_sym: ps - d_sym + CODED].tobytes(), (tag, j)
                check_record(rec[j], link_model(oracle, own), (tag, j))
    finally:
        close(out)
    same_but_shifted((got, neigh, out["trace"], out["links"]), ctl, out["n_src"], d_sym, d_samp, not opt.get("pop_src", True), tag)


def test_refusals(amd, probe, caps):
    """opv_tap_soft with `first` older than what the stream holds, at far indices, answers OPV_EINVAL and the stream stays usable;
    a blob with an entry below the 24-symbol rule is refused by the shift, its bytes untouched, and still imports as it is."""
    xs, exps = caps
    x, e = xs["noisy"], exps["noisy"]
    n = e["n"]
    _, d_sym, d_samp = plan("call_2p32", exps)
    acc = new_acc()
    src = amd.Demod(1, max_samples=n + 64, streaming=True)
    feed(src, 0, x, 0, CUT, acc)
    blob = bytes(src.export_streams([0]))
    floor = struct.unpack_from("<Q", blob, probe.probe_offset(b"sizeof.header") + probe.probe_offset(b"e.soft_first"))[0]
    n_cut = src.state(0).total_symbols
    n_src = dict(symbols=n_cut, frames=sum(len(f) for f in acc["frames"]), events=sum(len(v) for v in acc["events"]))
    assert 0 < floor < n_cut - 24
    tail = src.soft(0, first=floor)
    src.close()
    rc, far = shifted_blob(probe, blob, d_sym, d_samp)
    assert rc == 0
    d = amd.Demod(1, max_samples=n + 64, streaming=True)
    d.import_streams([0], far)
    for first in (0, 1, floor, n_cut - 1, d_sym, floor + d_sym - 2, floor + d_sym - 1, (floor + d_sym) & 0x7FFFFFFF):
        with pytest.raises(amd.OpvError) as err:
            d.soft(0, first=first)
        assert int(str(err.value).split("opv error ")[1].split(":")[0]) == EINVAL, first
    assert d.soft(0, first=floor + d_sym).tobytes() == tail.tobytes()          # what travelled, by its far index
    assert d.soft(0, first=n_cut + d_sym).size == 0 and d.soft(0, first=n_cut + d_sym + (1 << 32)).size == 0
    acc["n_soft"] += d_sym
    feed(d, 0, x, CUT, n, acc)
    d.flush(0)
    d.process()
    held_to_the_oracle(amd, d, 0, acc, far_expectation(e, n_src, d_sym, False), "after eight refused taps", offset_ties=None)
    d.close()
    # below the 24-symbol rule: cut at 50 000 samples no demodulate() call has been made (n_soft = 0)
    src = amd.Demod(1, max_samples=n + 64, streaming=True)
    acc = new_acc()
    feed(src, 0, x, 0, 50000, acc)
    assert src.state(0).total_symbols == 0 and src.state(0).sync_state == HUNTING
    blob = bytes(src.export_streams([0]))
    src.close()
    rc, same = shifted_blob(probe, blob, d_sym, d_samp)
    assert rc != 0 and same == blob
    d = amd.Demod(1, max_samples=n + 64, streaming=True)
    d.import_streams([0], same)
    feed(d, 0, x, 50000, n, acc)
    d.flush(0)
    d.process()
    held_to_the_oracle(amd, d, 0, acc, e, "after a refused shift", offset_ties=None)
    d.close()
