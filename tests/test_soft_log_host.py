"""The made soft logs of tests/soft_log_inputs.py, on the CPU: every edge pair really sits on two sides of its edge (in the
oracle), and the oracle's back half (oro_tracker_process + oro_frame_decode) equals the compiled reference's on all of them -
inputs neither had been compared on before: thresholds met with equality, non-finite values, denormals, overflowing sums.
tests/test_gpu_soft_log.py then holds the device's tracker and in-context decoder to the oracle on the same logs."""
import numpy as np
import pytest

import soft_log_inputs as S
from oracle_lib import Reference, format_events


@pytest.fixture(scope="module")
def logs(oracle):
    d = S.all_logs(oracle)
    d["g.edge"] = S.decoder_edge_log(oracle)[1]
    return d


@pytest.fixture(scope="module")
def tracked(oracle, logs):
    """Oracle.track of every log, once"""
    return {name: oracle.track(log.soft) for name, log in logs.items()}


def kinds(t):
    return [(int(e["kind"]), int(e["sym_idx"])) for e in t["events"]]


def ev_at(t, kind, sym):
    hit = [e for e in t["events"] if int(e["kind"]) == kind and int(e["sym_idx"]) == sym]
    assert len(hit) == 1, (kind, sym, kinds(t))
    return hit[0]


def test_hunting_pairs_sit_on_both_sides_of_the_thresholds(tracked):
    """(a): raw == 5000 / 4999 at norm 1, norm 6800/8000 / 6798/8000 and the same ten times larger. The word ends at symbol 63."""
    for name, raw, corr in (("a.raw5000", 5000.0, 1.0), ("a.norm085", 6800.0, 0.85), ("a.rawhigh", 68000.0, 0.85)):
        yes, no = tracked[name + ".yes"], tracked[name + ".no"]
        e = ev_at(yes, 1, 63)
        assert e["raw"] == raw and e["corr"] == corr, (name, e)
        assert (1, 63) not in kinds(no), name
        assert len(no["metrics"]) < len(yes["metrics"]), name               # the refused word costs its frame
    assert len(tracked["a.raw5000.no"]["events"]) == 0 and tracked["a.raw5000.no"]["final_state"] == 0
    lone = ev_at(tracked["a.lone_symbol"], 1, 40)
    assert lone["raw"] == 6000.0 and lone["corr"] == 1.0


def test_locked_pairs_sit_on_both_sides_of_the_check(tracked):
    """(b): the second sync slot (ends at symbol 30 + 2168) at 7000/10000 / 6998/10000, energy 100 / 99 and energy 0."""
    c = 30 + 2168
    for name, corr_yes, corr_no, raw_no in (("b.norm070", 0.70, 6998.0 / 10000.0, 6998.0), ("b.energy100", 1.0, 0.0, 99.0),
                                            ("b.silent", 1.0, 0.0, 0.0)):
        yes, no = tracked[name + ".yes"], tracked[name + ".no"]
        assert ev_at(yes, 3, c)["corr"] == corr_yes, name
        miss = ev_at(no, 4, c)
        assert miss["corr"] == corr_no and miss["raw"] == raw_no and miss["count"] == 1, (name, miss)
        assert (3, c) not in kinds(no) and (4, c) not in kinds(yes)
        # the miss costs no frame: the flywheel releases it with sync_ok = 0 and the miss's norm as quality
        assert np.array_equal(yes["frame_sym"], no["frame_sym"]) and np.array_equal(yes["frames"], no["frames"])
        assert yes["sync_ok"].tolist() == [1, 1, 1, 1] and no["sync_ok"].tolist() == [1, 0, 1, 1]
        assert no["quality"][1] == corr_no and yes["quality"][1] == corr_yes


def test_miss_counter_pairs(tracked):
    """(c): four misses and a recovery against five and LOST_LOCK; a clean word right behind LOST_LOCK."""
    yes, no = tracked["c.four_five.yes"], tracked["c.four_five.no"]
    first = 26
    checks = [first + 2168 * k for k in range(1, 8)]
    assert [ev_at(yes, 4, c)["count"] for c in checks[:4]] == [1, 2, 3, 4]
    assert ev_at(yes, 3, checks[4])["corr"] == 1.0 and 5 not in [k for k, _ in kinds(yes)]
    assert yes["sync_ok"].tolist() == [1, 0, 0, 0, 0, 1, 1]
    assert yes["quality"].tolist() == [1.0, 0.0, -1.0, 0.5, 0.0, 1.0, 1.0]               # zero and negative norms as quality
    assert ev_at(yes, 4, checks[6])["count"] == 1                                        # (the log's end) the counter started again
    assert ev_at(no, 4, checks[4])["count"] == 5 and (5, checks[4]) in kinds(no)
    # nothing is released for the slot that lost lock: the next release belongs to the word found by the new hunt
    assert no["frame_sym"].tolist()[:5] == yes["frame_sym"].tolist()[:5]
    relock = ev_at(no, 1, checks[5])
    assert no["frame_sym"][5] == int(relock["sym_idx"]) + 2144
    lost = checks[4]
    for name, at in (("c.relock_next", lost + 1), ("c.relock_23", lost + 23)):
        y, n = tracked[name + ".yes"], tracked[name + ".no"]
        assert (5, lost) in kinds(y) and (5, lost) in kinds(n), name
        assert ev_at(y, 1, at)["corr"] == 1.0 and y["final_state"] == 2, name
        assert kinds(n)[-1] == (5, lost) and n["final_state"] == 0, name


def test_first_sync_positions(tracked, logs):
    """(d): a word ending at symbol 22 is never seen, from 23 on it is; lanes 63 / 0 of the first two scan steps; two words in
    one 64-symbol span."""
    assert kinds(tracked["d.first22"])[0] == (1, 22 + 2168)
    for end in (23, 24, 86, 87):
        assert kinds(tracked["d.first%d" % end])[0] == (1, end)
    assert kinds(tracked["d.lane63_64.yes"])[0] == (1, 23 + 63) and kinds(tracked["d.lane63_64.no"])[0] == (1, 23 + 64)
    yes, no = tracked["d.two_in_step.yes"], tracked["d.two_in_step.no"]
    assert kinds(yes)[0] == (1, 40) and (1, 70) not in kinds(yes)
    assert kinds(no)[0] == (1, 70)
    assert (40 - 23) // 64 == (70 - 23) // 64 == 0                                       # both in the first scan step


def test_embedded_sync_words_are_ignored(oracle, tracked, logs):
    """(e): a HUNTING tracker takes the embedded words (tracked from a cut behind the frame's own word); in their place, in
    VERIFYING and in LOCKED, they change no event. A word embedded 2168 symbols after a false anchor passes the check there."""
    yes, no = tracked["e.embedded.yes"], tracked["e.embedded.no"]
    log = logs["e.embedded.yes"]
    m = log.marks
    for which in ("verifying", "locked"):
        cut = m[which + "_from"]
        assert kinds(oracle.track(log.soft[cut:]))[0] == (1, m[which + "_end"] - cut), which
    assert not np.array_equal(log.soft, logs["e.embedded.no"].soft)
    assert format_events(yes["events"]) == format_events(no["events"]) and np.array_equal(yes["frame_sym"], no["frame_sym"])
    assert yes["metrics"][0] > 0 and yes["metrics"][1] > 0 and no["metrics"].tolist() == [0, 0, 0]   # (the word costs the payload bits)
    fy, fn = tracked["e.false_anchor.yes"], tracked["e.false_anchor.no"]
    assert kinds(fy)[0] == (1, 50) and kinds(fn)[0] == (1, 50)
    assert ev_at(fy, 3, 50 + 2168)["corr"] == 1.0 and ev_at(fn, 4, 50 + 2168)["count"] == 1


def test_walk_shows_every_event_kind(tracked):
    """(h)"""
    t = tracked["h.walk"]
    assert sorted(set(k for k, _ in kinds(t))) == [1, 2, 3, 4, 5]
    assert len(t["metrics"]) >= 35 and (t["metrics"] == 0).any() and (t["metrics"] > 0).any()


def test_nonfinite_logs_do_what_the_tests_need(tracked):
    """(f): the spoilt word is passed over in HUNTING, is a miss with a NaN corr in LOCKED; (g) as a log: a dropped payload, a
    perfect one and one above 5000 all occur."""
    for name in ("f.nan", "f.pinf", "f.ninf"):
        t = tracked[name]
        assert kinds(t)[0] == (1, 9 + 23 + 2168), name                   # frame 0's word (ends at 32) is not taken
        miss = [e for e in t["events"] if int(e["kind"]) == 4][0]
        assert np.isnan(miss["corr"]) and int(miss["count"]) == 1, name
    m = tracked["g.edge"]["metrics"]
    assert (m == -1).any() and (m == 0).any() and (m > 5000).any()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref/libopv_ref.so not built")
def test_oracle_equals_the_compiled_reference_on_every_made_log(tracked, logs):
    """Oracle.track == Reference.track, field for field, on every log of (a)-(h) and on the decoder edge values as a log:
    frames, metrics (dropped frames included), release symbols, qualities (the exact doubles of every HUNTING hit and LOCKED
    check, NaN included), the tracker's lines and final state. The reference tells its events on stderr only: kind, count and
    symbol are compared exactly, corr / raw as the printed text (glibc prints the x86 default NaN as `-nan`, Python as `nan`;
    the sign of a NaN is not compared)."""
    ref = Reference()
    for name, log in logs.items():
        a, b = tracked[name], ref.track(log.soft)
        for k in ("frames", "metrics", "frame_sym", "quality", "sync_ok"):
            assert same(a[k], b[k]), (name, k)
        assert a["final_state"] == b["final_state"], name
        assert format_events(a["events"]) == b["log"], name
        for k in ("kind", "count", "sym_idx"):
            assert np.array_equal(a["events"][k], b["events"][k]), (name, k)


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref/libopv_ref.so not built")
def test_decoder_edge_payloads_and_the_undefined_cast(oracle):
    """FrameDecoder::decode on NaN, +/-Inf, sums that overflow, denormals, -0.0, one non-zero value, equal values and values on
    every quantiser boundary: oracle == compiled reference (metric and bytes).

    The reference's `int(n + 0.5)` of a NaN is undefined behaviour in C++. PINNED here: what the compiled reference does on this
    toolchain (g++ -O3, x86-64: cvttsd2si / cvttpd2dq return INT_MIN, std::clamp makes it 0). So a NaN, and every value of a
    payload whose scale is NaN, quantises to 0 ("confident bit 0"): a payload holding one NaN decodes to the all-zero code word
    with metric 0 and is written out as a perfect frame. An infinite scale (an Inf in the payload, or a sum that overflows)
    quantises every finite value to 4 and +/-Inf (Inf / Inf = NaN) to 0. The oracle (gcc, same casts) and the device
    (v_cvt_i32_f64: NaN -> 0, then the clamp) must both give this."""
    ref = Reference()
    names, pl = S.decoder_edge_payloads(oracle)
    zero_frame = oracle.frame_decode(np.full(2144, 1.0))["frame"]         # all coded bits 0
    for name, p in zip(names, pl):
        d = oracle.frame_decode(p)
        m, fr = ref.frame_decode(p)
        assert m == d["metric"], name
        if m >= 0:
            assert np.array_equal(fr, d["frame"]), name
        if name.endswith("+nan"):
            assert (d["q"] == 0).all() and m == 0 and np.array_equal(fr, zero_frame), name
        if name.endswith("inf"):
            assert sorted(set(d["q"].tolist())) == [0, 4] and (d["q"] == 0).sum() == 9, name
        if name.endswith("1.7e308"):
            assert (d["q"] == 4).all(), name
        if name.endswith("denormal") or name in ("zeros", "single@2143"):
            assert m == -1, name
        if name in ("single@0", "single@1071"):
            assert np.abs(p).max() / (np.abs(p).sum() / 2144) == 2144.0                  # the stated bound, met
    assert len(set(names)) == len(names)
