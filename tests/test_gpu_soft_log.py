"""The back half of the receive chain - k_sync_track, k_frame_scale / k_frame_scale_wave and k_frame_decode as opv_process
launches them - held to the oracle on MADE soft logs (tests/soft_log_inputs.py), handed to the device through the parity tap
opv_tap_push_soft: thresholds met with equality, hits in lane 63 / lane 0 of a scan step, windows and check / release symbols
on call boundaries, sync words the tracker must ignore, NaN / Inf / denormals / overflowing sums in sync windows and payloads.

Everything is compared with `==` (NaN with equal_nan): given the same doubles the back half is specified to be bit-identical
to the reference. tests/test_soft_log_host.py shows on the CPU that every pair of logs sits on both sides of its edge and that
the oracle equals the compiled reference on all of them.

The contexts are the smallest that can still go wrong: max_samples = 32 gives a soft ring of 4096 symbols (every second
payload and many sync windows wrap it), 4 frame slots and 80 event slots."""
import numpy as np
import pytest

import soft_log_inputs as S
from fixtures import amd  # noqa: F401
from oracle_lib import format_events
from stream_runs import HUNTING, LOCKED, code_of

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY, ESTATE = -1, -4, -6
SMALL = 32                                     # max_samples: cap_soft 4096, cap_frames 4, cap_events 80
MID = 330000                                   # cap_soft 16384, cap_frames 8, cap_events 96


def caps_of(max_samples):
    """opv_create's capacities"""
    cap_soft = 1
    while cap_soft < max_samples // 38 + 4096:
        cap_soft <<= 1
    cap_frames = max_samples // (2168 * 38) + 4
    return cap_soft, cap_frames, 4 * cap_frames + 64


@pytest.fixture(scope="module")
def logs(oracle):
    d = S.all_logs(oracle)
    d["g.edge"] = S.decoder_edge_log(oracle)[1]
    return d


@pytest.fixture(scope="module")
def tracked(oracle, logs):
    """Oracle.track of every log: computed once, shared, never changed"""
    return {name: oracle.track(log.soft) for name, log in logs.items()}


class Run:
    """what one stream has handed out so far"""

    def __init__(self, amd):
        self.frames, self.meta, self.events = [], [], []
        self.amd = amd

    def pop(self, d, s, events=True):
        f, m = d.pop_frames(s)
        self.frames.append(f)
        self.meta.append(m)
        if events:
            self.events.append(d.pop_events(s))
        return len(f)

    def result(self):
        return (np.concatenate(self.frames), np.concatenate(self.meta),
                np.concatenate(self.events) if self.events else np.zeros(0, self.amd.EVENT_DTYPE))


def feed(amd, d, s, soft, cuts=(), run=None, events=True):
    """`soft` to stream s in calls that end at the symbol counts `cuts` (and at the log's end); a call the ring has no room for
    (OPV_ECAPACITY) is halved. One opv_process per call, frames and events popped between rounds."""
    run = run or Run(amd)
    edges = sorted(set(c for c in cuts if 0 < c < soft.size) | {soft.size})
    todo = [soft[a:b] for a, b in zip([0] + edges[:-1], edges)]
    while todo:
        p = todo.pop(0)
        try:
            d.push_soft(s, p)
        except amd.OpvError as e:
            assert code_of(e) == ECAPACITY and p.size > 1, e
            todo[:0] = [p[:p.size // 2], p[p.size // 2:]]
            continue
        d.process()
        run.pop(d, s, events)
    return run


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))


def check_events(amd, got, exp, tag):
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for k in ("kind", "count", "sym_idx", "corr", "raw"):
        assert same(got[k], exp[k]), (tag, k, got[k], exp[k])
    assert amd.format_events(got) == format_events(exp), tag


def check(amd, d, s, run, exp, tag, events=True):
    """frames, metrics, release and payload symbols, qualities, sync_ok, events and their lines, total_symbols, final state"""
    fr, meta, ev = run.result()
    keep = exp["metrics"] >= 0                             # (opv_pop_frames skips what the decoder dropped, as the reference's writer does)
    assert same(meta["viterbi_metric"], exp["metrics"][keep]), (tag, meta["viterbi_metric"], exp["metrics"])
    assert same(fr, exp["frames"][keep]), tag
    assert same(meta["release_symbol"], exp["frame_sym"][keep]), tag
    assert same(meta["payload_symbol"], exp["frame_sym"][keep] - 2143), tag
    assert same(meta["sync_quality"], exp["quality"][keep]), (tag, meta["sync_quality"], exp["quality"])
    assert same(meta["sync_ok"], exp["sync_ok"][keep]), (tag, meta["sync_ok"], exp["sync_ok"])
    if events:
        check_events(amd, ev, exp["events"], tag)
    st = d.state(s)
    assert st.total_symbols == exp["n_soft"] and st.sync_state == exp["final_state"], (tag, st.total_symbols, st.sync_state)
    assert st.frames_released == len(exp["metrics"]) and st.frames_decoded == int(keep.sum()), (tag, st.frames_released)
    assert st.frames_perfect == int((exp["metrics"] == 0).sum()) and st.stalled == 0, tag
    assert st.total_samples == 0 and st.n_chunks == 0, tag  # (no front-end ever ran for this stream)
    if events:
        assert st.events_dropped == 0, tag


def special_cuts(log, exp):
    """the alignments of (d), and a call that ends one symbol before, on and one symbol after every check symbol
    (anchor + 2168: kinds 3 / 4, and the HUNTING hits) and every release symbol (anchor + 2144)"""
    cuts = set(log.cuts)
    syms = [int(e["sym_idx"]) for e in exp["events"] if int(e["kind"]) in (1, 3, 4)] + [int(v) for v in exp["frame_sym"]]
    for c in syms:
        cuts.update((c, c + 1, c + 2))                     # symbol c is the call's first missing symbol / its last / its last but one
    return cuts


@pytest.mark.parametrize("mode", ["whole", "odd_pieces", "special_cuts"])
def test_every_made_log_through_one_stream(amd, logs, tracked, mode):
    """Every log of (a)-(h) and the decoder edge values as a log, through one stream of the smallest context (reset in between):
    in one call where the ring takes it, in calls of 997 symbols, and cut at the listed alignments."""
    d = amd.Demod(1, max_samples=SMALL, streaming=True)
    try:
        for name, log in logs.items():
            exp = tracked[name]
            if mode == "whole":
                cuts = ()
            elif mode == "odd_pieces":
                cuts = range(997, log.soft.size, 997)
            else:
                cuts = special_cuts(log, exp)
            run = feed(amd, d, 0, log.soft, cuts)
            check(amd, d, 0, run, exp, (name, mode))
            tail = min(log.soft.size, 4096)
            assert same(d.soft(0, first=log.soft.size - tail, cap=tail), log.soft[-tail:]), name   # opv_tap_soft reads a tapped stream like any other
            d.reset(0)
    finally:
        d.close()


def test_decoder_edge_values_reach_every_branch_in_context(amd, logs, tracked):
    """The decoder edge values as payloads of a tapped log, through the in-context path (ring positions, fscale[], two frames
    per wave): equal to the oracle, and the DEVICE's results sit on different branches - a dropped payload, a perfect one
    and one with a metric above 5000."""
    d = amd.Demod(1, max_samples=SMALL, streaming=True)
    try:
        run = feed(amd, d, 0, logs["g.edge"].soft, range(2711, logs["g.edge"].soft.size, 2711))
        check(amd, d, 0, run, tracked["g.edge"], "g.edge")
        _, meta, _ = run.result()
        st = d.state(0)
        assert st.frames_released - st.frames_decoded >= 1
        assert (meta["viterbi_metric"] == 0).any() and (meta["viterbi_metric"] > 5000).any()
    finally:
        d.close()


def test_decoder_edge_values_isolated(amd, oracle):
    """k_decode_payloads on NaN, +/-Inf, sums that overflow, denormals, -0.0, a single non-zero value (|soft / scale| = 2144),
    equal values and values on every quantiser boundary: metric, quantised values, deinterleaved values, hard decisions and
    bytes against oracle.frame_decode. An odd number of payloads: the last wave's second half is idle."""
    names, pl = S.decoder_edge_payloads(oracle)
    if len(names) % 2 == 0:
        names, pl = names[:-1], pl[:-1]
    d = amd.Demod(1, max_samples=SMALL, streaming=True)
    try:
        got = d.decode_payloads(pl, taps=True)
    finally:
        d.close()
    mets = []
    for k, (name, p) in enumerate(zip(names, pl)):
        e = oracle.frame_decode(p)
        mets.append(e["metric"])
        assert got["metrics"][k] == e["metric"], (name, got["metrics"][k], e["metric"])
        if e["metric"] >= 0:
            assert np.array_equal(got["q"][k], e["q"]), (name, np.flatnonzero(got["q"][k] != e["q"])[:8])
            assert np.array_equal(got["deint"][k], e["deint"]), name
            assert np.array_equal(got["bits"][k], e["bits"]), name
            assert np.array_equal(got["frames"][k], e["frame"]), name
    mets = np.array(mets)
    assert (mets == -1).any() and (mets == 0).any() and (mets > 5000).any()


def test_five_streams_release_0_1_2_3_5_frames_in_one_round(amd, oracle):
    """S = 5, one opv_process: odd counts (an idle second half of a decoder wave), a stream with nothing, the stream-major grid.
    Every log ends on its last frame's release symbol: a release on the last symbol of a call."""
    counts = [0, 1, 2, 3, 5]
    lg = [S.counted_log(oracle, n, seed=40 + n) for n in counts]
    exp = [oracle.track(l.soft) for l in lg]
    assert [len(e["metrics"]) for e in exp] == counts
    d = amd.Demod(5, max_samples=MID, streaming=True)
    try:
        for s, l in enumerate(lg):
            d.push_soft(s, l.soft)
        d.process()
        runs = []
        for s in range(5):
            assert d.state(s).frames_released == counts[s]
            r = Run(amd)
            r.pop(d, s)
            runs.append(r)
        for s in range(5):
            check(amd, d, s, runs[s], exp[s], ("five", s))
    finally:
        d.close()


def test_many_streams_take_the_frame_per_lane_scale_kernel(amd, oracle, logs, tracked):
    """1100 streams x the 4 frame slots of the smallest context exceed what opv_process gives the wave-per-frame scale pre-pass:
    k_frame_scale (one frame per lane) runs instead. Tapped logs on streams 0, 1, 63, 64 and 1099, the others idle."""
    S_, names = 1100, ["b.norm070.yes", "f.nan", "c.four_five.no", "g.edge", "d.two_in_step.yes"]
    where = [0, 1, 63, 64, 1099]
    d = amd.Demod(S_, max_samples=SMALL, streaming=True)
    try:
        runs = {s: Run(amd) for s in where}
        longest = max(logs[n].soft.size for n in names)
        for at in range(0, longest, 1900):                  # 1900 symbols always fit behind a frame in flight (4096 - 2168)
            for s, n in zip(where, names):
                p = logs[n].soft[at:at + 1900]
                if p.size:
                    d.push_soft(s, p)
            d.process()
            for s in where:
                runs[s].pop(d, s)
        for s, n in zip(where, names):
            check(amd, d, s, runs[s], tracked[n], ("many", n))
        assert d.state(500).total_symbols == 0 and d.state(500).frames_released == 0
    finally:
        d.close()


def test_released_backlog_and_the_lossy_event_ring(amd, oracle):
    """A consumer that stops popping: the tracker stalls in front of the ninth release (8 frame slots), the soft ring takes
    symbols until it is full, and after the pops ONE round - entered with a 100-symbol push, i.e. an estimate of 4 frames -
    releases and decodes the whole backlog (the scale and decode grids stride on). Then the rest of a 130-frame log with the
    frames popped and the events never: the ring's retained tail is the oracle's last lines."""
    cap_soft, cap_frames, cap_events = caps_of(MID)
    assert (cap_soft, cap_frames, cap_events) == (16384, 8, 96)
    log = S.long_log(oracle)
    exp = oracle.track(log.soft)
    rel = exp["frame_sym"].astype(np.int64)
    assert (exp["metrics"] >= 0).all() and len(exp["events"]) > cap_events + 20
    d = amd.Demod(1, max_samples=MID, streaming=True)
    try:
        run = Run(amd)
        pushed = 0
        while True:                                         # no pops: until the ring refuses a push
            try:
                d.push_soft(0, log.soft[pushed:pushed + 2000])
            except amd.OpvError as e:
                assert code_of(e) == ECAPACITY
                break
            pushed += 2000
            d.process()
            assert pushed < 40000
        st = d.state(0)
        # the stall, through the state and the events: stopped in front of release number cap_frames + 1, nothing lost
        assert st.stalled == 2 and st.frames_released == cap_frames and st.sync_state == LOCKED and st.total_symbols == pushed
        stall_at = int(rel[cap_frames])
        assert pushed > stall_at
        ev0 = d.pop_events(0)
        n0 = int((exp["events"]["sym_idx"] < stall_at).sum())
        check_events(amd, ev0, exp["events"][:n0], "stall")
        assert run.pop(d, 0, events=False) == cap_frames
        d.push_soft(0, log.soft[pushed:pushed + 100])
        pushed += 100
        backlog = int((rel < pushed).sum()) - cap_frames
        assert backlog > 4, backlog                         # more than the 100 / 2168 + 4 frames this round is sized for
        d.process()
        assert run.pop(d, 0, events=False) == backlog       # all of it, in that one round
        assert d.state(0).stalled == 0
        feed(amd, d, 0, log.soft[pushed:], range(9001, log.soft.size, 9001), run=run, events=False)
        n_ev = len(exp["events"]) - n0
        assert n_ev > cap_events
        assert d.state(0).events_dropped == n_ev - cap_events
        tail = d.pop_events(0)
        check_events(amd, tail, exp["events"][-cap_events:], "tail")
        run.events = []
        exp_all = dict(exp, n_soft=log.soft.size)
        check(amd, d, 0, run, exp_all, "backlog", events=False)
        assert d.state(0).events_dropped == n_ev - cap_events
    finally:
        d.close()


def test_tap_contract_and_an_iq_neighbour(amd, oracle, iq10, logs, tracked):
    """opv_tap_push_soft's own rules: OPV_ECAPACITY at exactly one symbol over the front-end's ring rule and acceptance at the
    limit (nothing staged by a refused call), OPV_ESTATE both ways for mixing with IQ, opv_reset_stream clears it - and a
    neighbour stream that receives ordinary IQ in the same rounds still equals oracle.receive."""
    n = iq10.size // 2
    M = n + 64
    cap_soft = caps_of(M)[0]
    d = amd.Demod(3, max_samples=M, streaming=True)
    quiet = 0.5 * np.ones(cap_soft + 1)                     # (energy 12 per window: never a sync word)

    def refused(call, *a):
        with pytest.raises(amd.OpvError) as e:
            call(*a)
        return code_of(e.value)
    try:
        # ---- the ring rule: (n_soft - soft_keep) + n <= cap_soft, soft_keep = 0 before the tracker has run ...
        assert refused(d.push_soft, 0, quiet) == ECAPACITY
        assert d.state(0).total_symbols == 0
        d.push_soft(0, quiet[:cap_soft - 5])
        assert refused(d.push_soft, 0, quiet[:6]) == ECAPACITY
        d.push_soft(0, quiet[:5])
        assert refused(d.push_soft, 0, quiet[:1]) == ECAPACITY
        d.process()
        st = d.state(0)
        assert st.total_symbols == cap_soft and st.sync_state == HUNTING and st.stalled == 0
        # ... and the tracker's next window (23 symbols back) after a hunt over everything: soft_keep = trk_next - 24
        assert refused(d.push_soft, 0, quiet[:cap_soft - 23]) == ECAPACITY
        assert d.state(0).total_symbols == cap_soft
        d.push_soft(0, quiet[:cap_soft - 24])
        d.process()
        assert d.state(0).total_symbols == 2 * cap_soft - 24 and len(d.pop_events(0)) == 0
        # ---- bad arguments
        L = amd.lib()
        for args in ((None, 0, quiet.ctypes.data, 10), (d.h, 3, quiet.ctypes.data, 10), (d.h, -1, quiet.ctypes.data, 10),
                     (d.h, 0, None, 10), (d.h, 0, quiet.ctypes.data, 0)):
            assert L.opv_tap_push_soft(*args) == EINVAL, args
        import ctypes as C
        blob = np.zeros(1 << 16, np.uint8)
        assert L.opv_export_streams(d.h, 1, (C.c_int * 1)(0), blob.ctypes.data, blob.size) == ESTATE
        # ---- no mixing: a tapped stream takes no IQ ...
        few = iq10[:2000]
        assert refused(d.push, 0, few) == ESTATE
        assert refused(d.push_batch, [0], [few]) == ESTATE
        assert refused(d.flush, 0) == ESTATE
        import torch
        dev_iq = torch.zeros(4096, dtype=torch.int16, device="cuda:0")
        assert refused(d.attach, 0, dev_iq.data_ptr(), 1000, True) == ESTATE
        wb = amd.Wideband(d, 1, [0], [0.0], np.array([1], np.int16), 0)
        try:
            assert refused(wb.push, few) == ESTATE
        finally:
            wb.close()
        # ... and a stream that has received IQ takes no staged symbols; the context stays usable either way
        d.push(1, few)
        assert refused(d.push_soft, 1, quiet[:10]) == ESTATE
        d.attach(2, dev_iq.data_ptr(), 1000, False)
        assert refused(d.push_soft, 2, quiet[:10]) == ESTATE
        d.process()
        d.sync()
        # ---- opv_reset_stream clears it, both ways
        d.reset(-1)
        assert refused(d.push_soft, 0, quiet) == ECAPACITY  # (a fresh ring again: soft_keep = 0)
        name = "c.four_five.no"
        log, exp = logs[name], tracked[name]
        run0 = Run(amd)
        # stream 1 (IQ before the reset) now takes the log, stream 0 (tapped before) the IQ, in the same rounds
        pieces = [log.soft[a:a + 1777] for a in range(0, log.soft.size, 1777)]
        step = (-(-n // len(pieces)) + 1) & ~1
        got1 = Run(amd)
        for k, p in enumerate(pieces):
            d.push_soft(1, p)
            d.push(0, iq10[2 * k * step: 2 * (k + 1) * step])
            if k == len(pieces) - 1:
                d.flush(0)
            d.process()
            got1.pop(d, 1)
            run0.pop(d, 0)
        check(amd, d, 1, got1, exp, "neighbour of IQ")
        ref = oracle.receive(iq10, streaming=True)
        fr, meta, ev = run0.result()
        assert np.array_equal(fr, ref["frames"]) and len(fr) == 10
        assert np.array_equal(meta["viterbi_metric"], ref["metrics"]) and np.array_equal(meta["release_symbol"], ref["frame_sym"])
        assert amd.format_events(ev) == format_events(ref["events"])
        st = d.state(0)
        assert st.total_symbols == ref["n_soft"] and st.sync_state == ref["final_state"] and st.flushed == 1
    finally:
        d.close()
