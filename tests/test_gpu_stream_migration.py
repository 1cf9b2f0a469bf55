"""GPU: stream migration (opv_export_streams / opv_import_streams; csrc/k_stream_pack.hip) - a live stream taken out of one
context and put into another decodes as if it had never moved.

What that means here: per stream a test keeps what it popped and tapped from the SOURCE before the export (frames, meta, events,
soft symbols [0, n_soft), chunk log) and what it reads at the DESTINATION afterwards, concatenates the two, and holds the result to
the oracle's output for the WHOLE capture with check_stream's own bounds (bytes, metrics, release symbols, event lines ==; every
soft symbol under SOFT_TIGHT = 1e-9 of their mean; estimate ==; chunk log), plus stalled == 0 and edge_ties == 0.

The cuts are placed from the oracle's own events: before the offset search has run, in VERIFYING (the pending payload then lives
only in the soft tail), in LOCKED while a payload is collecting, in LOCKED between a release and the next sync check, between a
sync MISS and its flywheel frame, and with the flush still pending. (A clean capture demodulates to 2167 symbols per 86 720-sample
chunk while frames are 2168 symbols apart, so none of its chunk-boundary cuts within ten frames falls into the 24 symbols between a
release and the next sync check: that state is reached on a capture whose first 560 samples are cut off, which moves the first
acquired sync word to symbol 2177.)"""
import ctypes as C

import numpy as np
import pytest

from fixtures import amd  # noqa: F401
from oracle_lib import accidents, impair
from stream_checks import SOFT_TIGHT, _visible_gpus, check_stream, events_match, soft_err
from stream_runs import (CHUNK, HUNTING, LOCKED, VERIFYING, drain, feed, held_to_the_oracle, make_demod, new_acc, result, state_tuple,
                         tracker_at)

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY = -1, -4


@pytest.fixture(scope="module")
def caps(oracle, iq10):
    """the captures of this file and the oracle's result for each (computed once, never changed)"""
    c = {"clean": iq10,
         "noisy": impair(iq10, amp=2000.0, f0_hz=1200.0, ebn0_db=14.0, seed=5),
         "shifted": oracle.modulate(oracle.bert_frames(11))[2 * 560:]}
    rng = np.random.default_rng(7009)
    c["accident"], note = accidents(impair(iq10, amp=3000.0, f0_hz=-700.0, ebn0_db=15.0, seed=79), rng, 3000.0, n_max=2)
    exp = {k: oracle.receive(v, streaming=True) for k, v in c.items()}
    return c, exp


# ---- what a test keeps per stream: the accumulator of tests/stream_runs.py (new_acc, drain, result, held_to_the_oracle, feed) ------
def symbols_after(exp, n_chunks):
    return int(np.sum(exp["chunks"][:n_chunks, 4]))


def move(src, ks, dst, slots, via_bytes=True):
    blob = src.export_streams(ks)
    if via_bytes:
        blob = bytes(blob)                                  # (what a file or a socket would carry)
    dst.import_streams(slots, blob)
    return len(blob)


# ---- 1. cut points on one capture, -s ----------------------------------------------------------------------------------------
CUTS = [("clean", 50000, "hunting"), ("clean", CHUNK, "verifying"), ("clean", 3 * CHUNK + 12345, "collecting"),
        ("clean", 5 * CHUNK, "collecting"), ("clean", None, "collecting"), ("shifted", 4 * CHUNK, "between")]


@pytest.mark.parametrize("popped", [False, True], ids=["frames_left_unpopped", "everything_popped"])
@pytest.mark.parametrize("name,cut,where", CUTS, ids=[f"{n}-{c}-{w}" for n, c, w in CUTS])
def test_cut_points_source_destroyed_blob_through_bytes(amd, caps, name, cut, where, popped):
    """Pushed in pieces, exported after `cut` samples (None: all of them, the flush still pending), the source DESTROYED, the blob
    passed through bytes(), imported into a fresh context, the rest pushed, flushed."""
    x, exp = caps[0][name], caps[1][name]
    n = x.size // 2
    cut = n if cut is None else cut
    acc = new_acc()
    src = amd.Demod(1, max_samples=n + 64, streaming=True)
    feed(src, 0, x, 0, cut, acc, pop=popped)
    st = src.state(0)
    # the cut is where this case says it is - by the oracle's events and by the product's own state
    n_sym = symbols_after(exp, st.n_chunks)
    assert st.total_symbols == n_sym and tracker_at(exp, n_sym) == where, (st.n_chunks, n_sym, tracker_at(exp, n_sym))
    assert st.sync_state == {"hunting": HUNTING, "verifying": VERIFYING}.get(where, LOCKED)
    if (name, cut) == ("clean", CHUNK):
        early = exp["events"][exp["events"]["sym_idx"] < n_sym]
        assert n_sym == 2167 and [(int(e["kind"]), int(e["sym_idx"])) for e in early] == [(1, 23)] and exp["frame_sym"][0] >= n_sym
    if cut == 50000:
        assert st.n_chunks == 0 and np.isnan(st.est_offset_hz)          # the offset search has not run yet
    released = st.frames_released
    blob = bytes(src.export_streams([0]))
    assert amd.blob_streams(blob) == 1
    src.close()
    dst = amd.Demod(1, max_samples=n + 64, streaming=True)
    dst.import_streams([0], blob)
    st2 = dst.state(0)
    assert state_tuple(st2) == state_tuple(st)                            # counters, cursors and carry as exported
    if not popped:
        assert st2.frames_released == released and not acc["frames"]
        assert st2.frames_decoded == released                             # (counted from the unpopped metrics that travelled)
    feed(dst, 0, x, cut, n, acc)
    dst.flush(0)
    dst.process()
    held_to_the_oracle(amd, dst, 0, acc, exp, f"{name} cut at {cut} ({where}) popped={popped}", offset_ties=0 if name == "clean" else None)
    dst.close()


# ---- 2. across mappings and positions ----------------------------------------------------------------------------------------
def run_legs(amd, caps, monkeypatch, first_device=0):
    """three streams from a 3-stream context (k_msk_frontend_rb) into slots {5, 1, 14} of a 20-stream context forced to four streams
    per wave, on into one forced to sixteen, and back into 1-stream contexts; the accident capture's first cut lies between a sync
    MISS and the flywheel frame that follows it"""
    names = ["clean", "noisy", "accident"]
    xs, exps = [caps[0][k] for k in names], [caps[1][k] for k in names]
    ns = [x.size // 2 for x in xs]
    cuts = [[3 * CHUNK + 4000, 5 * CHUNK + 777, 8 * CHUNK], [2 * CHUNK + 99, 6 * CHUNK, 7 * CHUNK + 31111], [6 * CHUNK + 5000, 7 * CHUNK, 9 * CHUNK + 1]]
    accs = [new_acc() for _ in names]
    M = max(ns) + 64
    slots = [5, 1, 14]

    def leg(d, where, i):
        for k in range(3):
            feed(d, where[k], xs[k], 0 if i == 0 else cuts[k][i - 1], cuts[k][i], accs[k])

    a = make_demod(amd, monkeypatch, False, 3, max_samples=M, streaming=True)
    leg(a, [0, 1, 2], 0)
    assert a.frontend_kernel() == "k_msk_frontend_rb"
    st = a.state(2)
    n_sym = symbols_after(exps[2], st.n_chunks)
    assert st.total_symbols == n_sym and tracker_at(exps[2], n_sym) == "miss-collecting" and st.sync_state == LOCKED
    b = amd.Demod(20, max_samples=M, streaming=True, device=first_device)
    b.set_frontend(4)
    move(a, [0, 1, 2], b, slots)
    a.close()
    leg(b, slots, 1)
    assert b.frontend_kernel() == "k_msk_frontend_x4_wg4"
    c = amd.Demod(20, max_samples=M, streaming=True)
    c.set_frontend(16)
    move(b, slots, c, slots)
    b.close()
    leg(c, slots, 2)
    assert c.frontend_kernel() == "k_msk_frontend_x16_wg4"
    for k in range(3):
        one = make_demod(amd, monkeypatch, False, 1, max_samples=M, streaming=True)
        move(c, [slots[k]], one, [0])
        feed(one, 0, xs[k], cuts[k][2], ns[k], accs[k])
        one.flush(0)
        one.process()
        assert one.frontend_kernel() == "k_msk_frontend_rb"
        held_to_the_oracle(amd, one, 0, accs[k], exps[k], f"{names[k]} through rb -> x4 -> x16 -> rb", offset_ties=None)
        one.close()
    c.close()


def test_across_mappings_and_positions(amd, caps, monkeypatch):
    run_legs(amd, caps, monkeypatch)


@pytest.mark.skipif(_visible_gpus() < 2, reason="needs >= 2 GPUs (armed for an N-GPU box): the first leg's destination on device 1")
def test_across_mappings_with_the_first_destination_on_device_1(amd, caps, monkeypatch):
    """ARMED FOR AN N-GPU BOX (skipped on the 1-GPU pool): the blob is host memory, so the destination may be another device"""
    run_legs(amd, caps, monkeypatch, first_device=1)


# ---- 3. neighbours undisturbed -----------------------------------------------------------------------------------------------
def test_import_into_a_busy_context_leaves_the_neighbours_alone(amd, caps):
    """A destination of 8 streams, mid-capture with 6 of them live and a round in flight, imports 2: all 8 equal the oracle."""
    names = ["noisy", "clean", "accident", "clean", "noisy", "accident", "accident", "noisy"]
    xs, exps = [caps[0][k] for k in names], [caps[1][k] for k in names]
    ns = [x.size // 2 for x in xs]
    at = [2 * CHUNK + 500 * k for k in range(6)] + [4 * CHUNK + 17, 6 * CHUNK + 40000]
    accs = [new_acc() for _ in names]
    M = max(ns) + 64
    d = amd.Demod(8, max_samples=M, streaming=True)
    src = amd.Demod(2, max_samples=M, streaming=True)
    src_of = {6: 1, 7: 0}                                   # (source order need not be slot order)
    for k in range(6):
        feed(d, k, xs[k], 0, at[k], accs[k])
    for k in (6, 7):
        feed(src, src_of[k], xs[k], 0, at[k], accs[k], pop=(k == 6))
    for k in range(6):                                      # a round in flight when the import arrives: ordered, not lost
        d.push(k, xs[k][2 * at[k]: 2 * (at[k] + 30000)])
        at[k] += 30000
    d.process()
    move(src, [src_of[6], src_of[7]], d, [6, 7])
    src.close()
    for k in range(8):
        drain(d, k, accs[k])
    for k in range(8):
        feed(d, k, xs[k], at[k], ns[k], accs[k], piece=200000)
        d.flush(k)
    d.process()
    for k in range(8):
        held_to_the_oracle(amd, d, k, accs[k], exps[k], f"busy context stream {k}", offset_ties=None)
    d.close()


# ---- 4. wrapped rings, different capacities ----------------------------------------------------------------------------------
def test_wrapped_rings_into_a_context_of_other_capacities(amd, oracle, iq100):
    """100 frames at 13 dB and -900 Hz through a 3-chunk device buffer in pushes of a chunk and an odd remainder: at the export near
    frame 50 every ring of the source has wrapped; the destination's rings are more than twice as long. Held as
    test_long_stream_through_a_small_device_buffer holds its stream."""
    x = impair(iq100, amp=2500.0, f0_hz=-900.0, ebn0_db=13.0, seed=21)
    exp = oracle.receive(x, streaming=True)
    n, step = x.size // 2, CHUNK + 1237
    acc = new_acc()
    d = amd.Demod(1, max_samples=3 * CHUNK + 8192, streaming=True)
    o = 0
    while sum(len(f) for f in acc["frames"]) < 50:
        d.push(0, x[2 * o: 2 * (o + step)])
        o += step
        d.process()
        drain(d, 0, acc, soft=False)
    st = d.state(0)
    assert st.chunk_origin != 0 and st.sync_state == LOCKED
    with pytest.raises(amd.OpvError):
        d.soft(0, first=0)                                  # n_soft > cap_soft: the soft ring has wrapped
    tail_src = d.soft(0, first=st.total_symbols - 24)        # (the tracker's own window: the least a carried tail holds)
    d2 = amd.Demod(1, max_samples=8 * CHUNK, streaming=True)
    size = move(d, [0], d2, [0])
    print(f"blob of a wrapped 3-chunk stream: {size} bytes")
    d.close()
    assert state_tuple(d2.state(0)) == state_tuple(st)
    assert np.array_equal(d2.soft(0, first=st.total_symbols - 24), tail_src)
    with pytest.raises(amd.OpvError):
        d2.soft(0, first=0)                                 # history older than the carried tail did not travel
    while o < n:
        d2.push(0, x[2 * o: 2 * min(o + step, n)])
        o += step
        d2.process()
        drain(d2, 0, acc, soft=False)
    d2.flush(0)
    d2.process()
    drain(d2, 0, acc, soft=False)
    frames, metas, events = np.concatenate(acc["frames"]), np.concatenate(acc["meta"]), np.concatenate(acc["events"])
    assert len(frames) == len(exp["frames"]) > 90
    assert np.array_equal(frames, exp["frames"])
    assert np.array_equal(metas["viterbi_metric"], exp["metrics"])
    assert np.array_equal(metas["release_symbol"], exp["frame_sym"])
    events_match(amd, events, exp["events"])
    st = d2.state(0)
    assert st.total_symbols == exp["n_soft"] and st.n_chunks == len(exp["chunks"]) and st.stalled == 0 and st.edge_ties == 0
    assert st.frames_decoded == len(exp["frames"])
    assert abs(st.freq_offset_hz - exp["final_freq_offset"]) < 1e-6
    chunks = np.concatenate(acc["chunks"])
    assert np.array_equal(chunks[:, 3:], exp["chunks"][:, 3:]) and np.allclose(chunks[:, :3], exp["chunks"][:, :3], rtol=0, atol=1e-7)
    a, _ = soft_err(d2.soft(0, first=exp["n_soft"] - 1000), exp["soft"][-1000:])
    assert a < SOFT_TIGHT
    d2.close()


# ---- 5. same kernel, same schedule -> same bits ------------------------------------------------------------------------------
def test_moved_stream_is_bit_identical_to_the_unmoved_one(amd, caps):
    """One capture (a) straight through and (b) exported and imported at 3 x 86 720 + 12 345 samples into a context of the same
    shape, the same pushes and rounds either way: frames, metas, events, chunk log, final state and ALL soft symbols ==."""
    x = caps[0]["noisy"]
    n, cut = x.size // 2, 3 * CHUNK + 12345
    out = []
    for moved in (False, True):
        acc = new_acc()
        d = amd.Demod(1, max_samples=n + 64, streaming=True)
        feed(d, 0, x, 0, cut, acc, piece=150000)
        if moved:
            d2 = amd.Demod(1, max_samples=n + 64, streaming=True)
            move(d, [0], d2, [0])
            d.close()
            d = d2
        feed(d, 0, x, cut, n, acc, piece=150000)
        d.flush(0)
        d.process()
        got = result(amd, d, 0, acc)
        got["state"] = state_tuple(got["state"])
        out.append(got)
        d.close()
    a, b = out
    assert a["state"] == b["state"]
    for k in ("frames", "meta", "events", "chunks", "soft"):
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


# ---- 6. batch mode -----------------------------------------------------------------------------------------------------------
def test_batch_mode_export_before_flush(amd, oracle, caps):
    x = caps[0]["noisy"]
    exp = oracle.receive(x, streaming=False)
    n = x.size // 2
    acc = new_acc()
    d = amd.Demod(1, max_samples=n + 64, streaming=False)
    d.push(0, x[: 2 * 300001])
    d.process()
    d.push(0, x[2 * 300001:])
    assert d.state(0).total_symbols == 0
    d2 = amd.Demod(1, max_samples=n + 64, streaming=False)
    move(d, [0], d2, [0])
    d.close()
    d2.flush(0)
    d2.process()
    held_to_the_oracle(amd, d2, 0, acc, exp, "batch mode, exported before the flush", offset_ties=None)
    d2.close()


# ---- 7. refusals, all decided on the host ------------------------------------------------------------------------------------
def import_rc(amd, d, slots, blob):
    b = np.frombuffer(bytes(blob), np.uint8)
    ids = (C.c_int * len(slots))(*slots)
    return amd.lib().opv_import_streams(d.h, len(slots), ids, b.ctypes.data if b.size else None, b.size)


def test_refusals_leave_the_destination_usable(amd, oracle, caps):
    x, exp = caps[0]["clean"], caps[1]["clean"]
    n = x.size // 2
    src = amd.Demod(2, max_samples=n + 64, streaming=True)
    for k in range(2):
        feed(src, k, x, 0, n, new_acc(), pop=False, piece=300000)     # nine frames released (the tenth waits for the flush), none popped
    good = bytes(src.export_streams([0, 1]))
    one = bytes(src.export_streams([1]))
    assert src.state(1).frames_released == 9
    src.pop_frames(0)
    src.push(0, x[: 2 * 150000])                                      # 150 000 samples behind the processed ones, nothing unpopped
    big_tail = bytes(src.export_streams([0]))
    src.close()
    assert amd.blob_streams(good) == 2 and amd.blob_streams(one) == 1

    def poked(blob, at, width):
        b = bytearray(blob)
        for i in range(at, at + width):
            b[i] ^= 0x5A
        return bytes(b)

    d = amd.Demod(4, max_samples=n + 64, streaming=True)
    before = [state_tuple(d.state(k)) for k in range(4)]
    assert import_rc(amd, d, [0, 1], good[:-100]) == EINVAL           # truncated in the payload
    assert import_rc(amd, d, [0, 1], good[:40]) == EINVAL             # ... in the header
    assert import_rc(amd, d, [0, 1], good[:3000]) == EINVAL           # ... in the directory
    assert import_rc(amd, d, [0, 1], b"") == EINVAL
    assert import_rc(amd, d, [0, 1], poked(good, 0, 8)) == EINVAL     # magic
    assert import_rc(amd, d, [0, 1], poked(good, 8, 4)) == EINVAL     # format version
    assert import_rc(amd, d, [0, 1], poked(good, 12, 4)) == EINVAL    # sizeof(OpvStream)
    assert import_rc(amd, d, [0, 4], good) == EINVAL                  # destination out of range
    assert import_rc(amd, d, [0, -1], good) == EINVAL
    assert import_rc(amd, d, [2, 2], good) == EINVAL                  # named twice
    assert import_rc(amd, d, [0], good) == EINVAL                     # count other than the blob's
    assert [state_tuple(d.state(k)) for k in range(4)] == before
    batch = amd.Demod(2, max_samples=n + 64, streaming=False)
    assert import_rc(amd, batch, [0, 1], good) == EINVAL              # a streaming blob into a batch context
    batch.close()
    small = amd.Demod(1, max_samples=100000, streaming=True)
    assert import_rc(amd, small, [0], big_tail) == ECAPACITY          # IQ tail larger than the destination's max_samples
    assert import_rc(amd, small, [0], one) == ECAPACITY               # nine unpopped frames, frame_capacity 5
    assert small.device_frames()[3] == 5
    short = x[: 2 * 95000]
    check_stream(amd, small.receive([short])[0], oracle.receive(short, streaming=True), "small context after two refusals")
    small.close()
    # after eleven refusals: the context decodes a capture in every slot, and then takes the good blob
    got = d.receive([x] * 4)
    for k in range(4):
        check_stream(amd, got[k], exp, f"context after refusals, stream {k}")
    assert import_rc(amd, d, [3, 0], good) == 0
    for k in (3, 0):
        f, m = d.pop_frames(k)
        assert len(f) == 9 and np.array_equal(f, exp["frames"][:9]) and np.array_equal(m["release_symbol"], exp["frame_sym"][:9])
    d.close()
