"""GPU: the per-frame link report (include/opv_demod.h: opv_link; csrc/k_frame_link.hip, csrc/opv_link.hip) held to the CPU model
tests/link_model.py: the four integers with ==, m1 with ==, m2 and ma within the derived bound 2146 x 2^-53 x (m2, m1) wherever
the payload is finite. Stand-alone (opv_link_payloads) and in context (opv_enable_link_report + opv_pop_frames_link) on made
soft logs handed over through opv_tap_push_soft, from IQ, across ring reuse, on / off, reset and import; and the chain's own
results (frames, meta, events) are the same bits with the report on and off.

tests/test_link_report_host.py pins the model to the oracle on the CPU."""
import ctypes as C

import numpy as np
import pytest

import soft_log_inputs as S
from fixtures import amd  # noqa: F401
from link_model import CODED, check_record, link_model
from oracle_lib import impair
from stream_runs import code_of

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY, ESTATE = -1, -4, -6
SMALL = 32                                     # max_samples: cap_soft 4096, cap_frames 4
MID = 330000                                   # cap_soft 16384, cap_frames 8


class DevPtr:
    """torch view of library-owned device memory (CUDA array interface v2)"""

    def __init__(self, ptr, shape, typestr):
        self.__cuda_array_interface__ = {"data": (ptr, False), "shape": shape, "typestr": typestr, "version": 2}


def device_ring(amd, d, cap_frames):
    """the whole record ring copied back: [n_streams][cap_frames] of LINK_DTYPE"""
    import torch
    d.sync()
    n = d.n_streams * cap_frames * amd.LINK_DTYPE.itemsize
    raw = torch.as_tensor(DevPtr(d.device_link(), (n,), "|u1"), device="cuda:0").cpu().numpy()
    return raw.view(amd.LINK_DTYPE).reshape(d.n_streams, cap_frames)


def all_zero(rec):
    return not np.asarray(rec).tobytes().strip(b"\0")


def noisy_log(oracle, n_frames, sigma, seed, lead=10):
    """n_frames frames back to back: clean sync words (the tracker releases every frame), noise on the payloads"""
    rng = np.random.default_rng(seed)
    return S.cat(S.zeros(lead), *[S.cat(S.sync(S.A), S.payload(oracle, k, sigma=sigma, rng=rng)) for k in range(n_frames)], S.zeros(30))


# ------------------------------------------------------------------------------------------------ 1. stand-alone
@pytest.fixture(scope="module")
def mix(oracle):
    """65 payloads - one more than a wave of lanes of k_payload_scale, an odd count for the two-frames-per-wave decoder - and their
    model records: computed once, shared, never changed"""
    names, rows = [], []

    def add(name, p):
        names.append(name)
        rows.append(np.asarray(p, np.float64))
    rng = np.random.default_rng(65)
    for k in range(4):
        add("clean%d" % k, S.payload(oracle, k))
    for sigma in (125.0, 250.0, 354.0):
        for k in range(8):
            add("sigma%d/%d" % (sigma, 5 + 3 * k), S.payload(oracle, 5 + 3 * k, sigma=sigma, rng=rng))
    flips = {}
    for k in (30, 31):
        at = rng.choice(CODED, 7, replace=False)
        p = S.payload(oracle, k).copy()
        p[at] = -p[at]
        add("flip7/%d" % k, p)
        p = S.payload(oracle, k).copy()
        p[at] = 0.0
        add("zero7/%d" % k, p)
        flips[k] = at
    add("all_zero", S.zeros(CODED))
    en, ep = S.decoder_edge_payloads(oracle)
    for n, p in zip(en, ep):
        add("edge:" + n, p)
    assert len(rows) == 65
    pl = np.ascontiguousarray(np.stack(rows))
    return names, pl, [link_model(oracle, p) for p in pl], flips


def test_stand_alone_65_payloads(amd, oracle, mix):
    names, pl, model, flips = mix
    d = amd.Demod(1, max_samples=SMALL, streaming=True)
    try:
        before = d.decode_payloads(pl)
        rec = d.link_payloads(pl)
        again = d.link_payloads(pl)
        after = d.decode_payloads(pl)
    finally:
        d.close()
    assert rec.tobytes() == again.tobytes()                 # a fixed order of additions: the same bits in every run
    seen = dict(dropped=0, nonfinite=0, errors=0, weak=0)
    for k, (name, m) in enumerate(zip(names, model)):
        print(name, "dev", rec[k], "model", {f: m[f] for f in ("valid", "bit_errors", "weak", "nonfinite", "m1", "m2", "ma")})
        check_record(rec[k], m, name)
        assert int(rec[k]["nonfinite"]) == (int((~np.isfinite(pl[k])).sum()) if m["valid"] else 0), name
        for got in (before, after):                         # the decoder's own answers are what they were
            assert got["metrics"][k] == m["metric"], name
            if m["metric"] >= 0:
                assert np.array_equal(got["frames"][k], m["frame"]), name
        seen["dropped"] += m["valid"] == 0
        seen["nonfinite"] += m["nonfinite"] > 0
        seen["errors"] += m["bit_errors"] > 0
        seen["weak"] += m["weak"] > 0
    assert all_zero(rec[names.index("all_zero")])
    # the known answers, on the device's records
    enc31 = oracle.encode_frame(oracle.bert_frames(1, first=31)[0])
    assert rec[names.index("flip7/31")]["bit_errors"] == 7 and rec[names.index("zero7/31")]["weak"] == 7
    assert rec[names.index("zero7/31")]["bit_errors"] == int((enc31[flips[31]] == 0).sum())
    assert all(rec[names.index("clean%d" % k)]["bit_errors"] == 0 for k in range(4))
    assert seen["dropped"] >= 3 and seen["nonfinite"] >= 9 and seen["errors"] >= 16 and seen["weak"] >= 16, seen
    db = amd.link_esn0_db(rec)
    assert np.isnan(db[names.index("all_zero")]) and np.isnan(db[names.index("edge:clean+nan")])
    assert abs(db[names.index("sigma250/5")] - 3.01) < 0.8  # (A^2 / 2 sigma^2; spread 0.16 dB on 2144 symbols: tests/test_link_report_host.py)


# ------------------------------------------------------------------------------------------------ 2. in context, made soft logs
def check_stream_records(oracle, got_link, got_frames, got_meta, exp, tag, first=0):
    """popped records against the model over the oracle's released payloads, in frame order (dropped frames skipped alike)"""
    keep = [k for k in range(first, len(exp["metrics"])) if exp["metrics"][k] >= 0]
    assert len(got_link) == len(keep) == len(got_frames), (tag, len(got_link), len(keep))
    for j, k in enumerate(keep):
        m = link_model(oracle, exp["payloads"][k])
        assert m["metric"] == exp["metrics"][k] == got_meta["viterbi_metric"][j], (tag, k)
        assert np.array_equal(got_frames[j], m["frame"]), (tag, k)
        check_record(got_link[j], m, (tag, k))
    return keep


def run_three(amd, logs, link):
    """three streams of one context fed in pieces of 997 / 1777 / 2000 symbols, one opv_process per round. Streams 0 and 1 are
    popped every round; stream 2's consumer stays away until its soft ring refuses a push, then pops, and the next round - entered
    with pushes of less than a frame, i.e. sized for 4 frames per stream - releases and decodes the backlog."""
    d = amd.Demod(3, max_samples=MID, streaming=True)
    out = [dict(frames=[], meta=[], events=[], link=[]) for _ in range(3)]
    over = {}
    try:
        if link:
            d.enable_link_report()
        pieces, pos, away = [997, 1777, 2000], [0, 0, 0], True

        def pop(s):
            if link:
                f, m, r = d.pop_frames(s, link=True)
                out[s]["link"].append(r)
            else:
                f, m = d.pop_frames(s)
            out[s]["frames"].append(f)
            out[s]["meta"].append(m)
            out[s]["events"].append(d.pop_events(s))
            return len(f)
        while any(pos[s] < logs[s].size for s in range(3)):
            for s in range(3):
                if pos[s] >= logs[s].size:
                    continue
                p = logs[s][pos[s]:pos[s] + pieces[s]]
                try:
                    d.push_soft(s, p)
                    pos[s] += p.size
                except amd.OpvError as e:
                    assert code_of(e) == ECAPACITY and s == 2 and away, (e, s)
                    over["before"] = d.state(2).frames_released
                    over["popped"] = pop(2)
                    away = False
                    d.push_soft(2, logs[2][pos[2]:pos[2] + 100])
                    pos[2] += 100
            d.process()
            if "before" in over and "after" not in over:
                over["after"] = d.state(2).frames_released
            for s in range(3):
                if s != 2 or not away:
                    pop(s)
        assert not away
        states = [d.state(s) for s in range(3)]
        res = []
        for s in range(3):
            o = out[s]
            res.append(dict(frames=np.concatenate(o["frames"]), meta=np.concatenate(o["meta"]), events=np.concatenate(o["events"]),
                            link=np.concatenate(o["link"]) if link else None, released=states[s].frames_released,
                            symbols=states[s].total_symbols))
        return res, over
    finally:
        d.close()


def test_in_context_on_made_soft_logs(amd, oracle):
    logs = [noisy_log(oracle, 12, 125.0, 1, lead=10), noisy_log(oracle, 12, 250.0, 2, lead=77), noisy_log(oracle, 18, 354.0, 3, lead=10)]
    exp = [oracle.track(l) for l in logs]
    on, over = run_three(amd, logs, True)
    off, over_off = run_three(amd, logs, False)
    assert over == over_off
    # one round carried more released frames than it was sized for (pushes below 2168 symbols: 0 + 4 frames per stream)
    assert over["before"] == 8 and over["after"] - over["before"] > 4, over
    wraps = 0
    for s in range(3):
        keep = check_stream_records(oracle, on[s]["link"], on[s]["frames"], on[s]["meta"], exp[s], ("made", s))
        assert on[s]["released"] == len(exp[s]["metrics"]) and on[s]["symbols"] == logs[s].size
        assert np.array_equal(on[s]["meta"]["release_symbol"], exp[s]["frame_sym"][keep])
        wraps += int(((on[s]["meta"]["payload_symbol"] % 16384) + CODED > 16384).sum())
        # the chain's own results are the same bits with the report on and off
        for k in ("frames", "meta", "events"):
            assert on[s][k].tobytes() == off[s][k].tobytes(), (s, k)
        assert on[s]["released"] == off[s]["released"]
    assert wraps >= 1                                       # at least one payload wraps the soft ring
    assert sum(int(on[s]["link"]["bit_errors"].sum()) for s in range(3)) > 100 and on[0]["link"]["valid"].all()
    assert len(on[0]["link"]) == 12 and len(on[2]["link"]) >= 16


# ------------------------------------------------------------------------------------------------ 3. ring reuse, on / off
def test_ring_reuse_and_on_off(amd, oracle):
    log = S.long_log(oracle, n_frames=30).soft
    exp = oracle.track(log)
    rel = exp["frame_sym"].astype(np.int64)
    assert len(rel) == 30 and (exp["metrics"] >= 0).all()
    L = amd.lib()
    d = amd.Demod(1, max_samples=MID, streaming=True)      # 8 frame slots
    pos = [0]
    frames, link = [], []

    def advance(n_released, pop=None):
        """symbols up to the release of frame n_released - 1, in pieces the ring always takes"""
        upto = int(rel[n_released - 1]) + 1
        while pos[0] < upto:
            p = log[pos[0]:min(upto, pos[0] + 1900)]
            d.push_soft(0, p)
            pos[0] += p.size
            d.process()
            if pop:
                pop()

    def pop_link():
        f, _, r = d.pop_frames(0, link=True)
        frames.append(f)
        link.append(r)

    def pop_plain(cap=None):
        f, _ = d.pop_frames(0, cap)
        frames.append(f)
        link.append(None if not len(f) else np.zeros(len(f), amd.LINK_DTYPE))
        return len(f)
    try:
        # ---- before the first enable: OPV_ESTATE, and the context goes on processing
        ptr = C.c_void_p()
        out, meta, rec = np.zeros((8, 134), np.uint8), np.zeros(8, amd.META_DTYPE), np.zeros(8, amd.LINK_DTYPE)
        assert L.opv_device_link(d.h, C.byref(ptr)) == ESTATE
        assert L.opv_pop_frames_link(d.h, 0, out.ctypes.data, 8, meta.ctypes.data, rec.ctypes.data) == ESTATE
        advance(2, pop_plain)
        assert sum(len(f) for f in frames) == 2
        # ---- on: 14 frames through 8 slots, every record is its own frame's
        d.enable_link_report()
        advance(16, pop_link)
        # ---- off: two frames decoded, opv_pop_frames_link refuses, opv_pop_frames works
        d.enable_link_report(False)
        advance(18)
        assert L.opv_pop_frames_link(d.h, 0, out.ctypes.data, 8, meta.ctypes.data, rec.ctypes.data) == ESTATE
        assert d.state(0).frames_released == 18
        assert pop_plain(cap=1) == 1                        # frame 16; frame 17 stays unpopped
        # ---- on again: what was decoded meanwhile reads valid = 0, the next frames are reported
        d.enable_link_report()
        advance(19)
        pop_link()
        assert len(link[-1]) == 2 and all_zero(link[-1][0]) and link[-1][1]["valid"] == 1
        advance(30, pop_link)
        fr = np.concatenate(frames)
        lk = [r for part in link if part is not None for r in part]
        assert len(fr) == 30 == len(lk) and np.array_equal(fr, exp["frames"])
        for k in range(30):
            if k < 2 or k in (16, 17):
                assert all_zero(lk[k]), k
            else:
                check_record(lk[k], link_model(oracle, exp["payloads"][k]), ("reuse", k))
    finally:
        d.close()


def test_enable_then_pop_with_no_round_in_between(amd, oracle):
    """opv_enable_link_report is complete when it returns: frames decoded with the report off, one popped (the host's view of the
    stream stays valid), enable, opv_pop_frames_link AT ONCE - no opv_process in between - reads all-zero records. On the first
    enable (the zero-fill is the fresh ring's only initialisation) and on a later off -> on transition, where the slots hold
    the valid records of earlier frames."""
    log = noisy_log(oracle, 12, 125.0, 4)
    exp = oracle.track(log)
    rel = exp["frame_sym"].astype(np.int64)
    assert len(rel) == 12 and (exp["metrics"] >= 0).all()
    d = amd.Demod(2, max_samples=SMALL, streaming=True)    # 4 frame slots
    pos = [0]

    def advance(n_released):
        upto = int(rel[n_released - 1]) + 1
        while pos[0] < upto:
            p = log[pos[0]:min(upto, pos[0] + 1900)]
            d.push_soft(1, p)
            pos[0] += p.size
            d.process()
    try:
        advance(1)
        d.pop_frames(1)
        advance(3)                                          # frames 1, 2 decoded with the report off
        f, _ = d.pop_frames(1, cap=1)
        assert np.array_equal(f, exp["frames"][1:2])
        d.enable_link_report()                              # first enable: allocates
        f, _, r = d.pop_frames(1, link=True)
        assert np.array_equal(f, exp["frames"][2:3]) and len(r) == 1 and all_zero(r)
        assert all_zero(device_ring(amd, d, 4))
        for k in (4, 5, 6, 7):                              # every slot now holds a valid record
            advance(k)
            f, _, r = d.pop_frames(1, link=True)
            assert len(r) == 1 and r[0]["valid"] == 1
            check_record(r[0], link_model(oracle, exp["payloads"][k - 1]), ("enable", k - 1))
        d.enable_link_report(False)
        advance(9)                                          # frames 7, 8 with the report off: slots 3, 0
        f, _ = d.pop_frames(1, cap=1)
        assert np.array_equal(f, exp["frames"][7:8])
        d.enable_link_report()                              # off -> on: zero-fills again
        f, _, r = d.pop_frames(1, link=True)
        assert np.array_equal(f, exp["frames"][8:9]) and len(r) == 1 and all_zero(r)
        advance(10)
        f, _, r = d.pop_frames(1, link=True)
        assert len(r) == 1
        check_record(r[0], link_model(oracle, exp["payloads"][9]), ("enable", 9))
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 4. from IQ
def test_from_iq_three_streams(amd, oracle):
    tx = oracle.bert_frames(4)
    clean = oracle.modulate(tx)
    caps = [clean, impair(clean, ebn0_db=12.0, seed=12), impair(clean, ebn0_db=6.0, seed=6)]
    M = clean.size // 2 + 64
    cap_frames = M // (2168 * 38) + 4
    d = amd.Demod(3, max_samples=M, streaming=True)
    try:
        d.enable_link_report()
        for s, iq in enumerate(caps):
            d.push(s, iq)
            d.flush(s)
        d.process()
        ring = device_ring(amd, d, cap_frames)
        errs = []
        for s in range(3):
            assert d.state(s).stalled == 0
            fr, meta, rec = d.pop_frames(s, link=True)
            # (at 6 dB the tracker locks late: the oracle releases two of the four frames)
            assert len(fr) == d.state(s).frames_released and len(fr) >= 1 and (s == 2 or len(fr) == 4), (s, len(fr))
            for k in range(len(fr)):
                soft = d.soft(s, first=int(meta["payload_symbol"][k]), cap=CODED)
                m = link_model(oracle, soft)                 # the device's own soft symbols: this holds the new kernel exactly
                assert np.array_equal(m["frame"], fr[k]) and m["metric"] == meta["viterbi_metric"][k], (s, k)
                print("iq", s, k, rec[k], float(amd.link_esn0_db(rec[k])))
                check_record(rec[k], m, ("iq", s, k))
                assert ring[s, k].tobytes() == rec[k].tobytes(), (s, k)   # frame k at slot k % frame_capacity of the device view
            assert all_zero(ring[s, len(fr):])
            errs.append(int(rec["bit_errors"].sum()))
            if s == 0:
                assert np.array_equal(fr, tx)
        assert errs[2] > 0 and errs[2] > errs[0], errs
    finally:
        d.close()


# ------------------------------------------------------------------------------------------------ 5. reset and import
def test_reset_and_import(amd, oracle):
    tx = oracle.bert_frames(6)
    clean = oracle.modulate(tx)
    caps = [clean, impair(clean, ebn0_db=12.0, seed=5)]
    M = clean.size // 2 + 64
    cap_frames = M // (2168 * 38) + 4
    cut = 2 * (3 * 86720 + 40000)                           # three frames and a half
    a = amd.Demod(2, max_samples=M, streaming=True)
    b = amd.Demod(2, max_samples=M, streaming=True)
    try:
        a.enable_link_report()
        b.enable_link_report()
        for s in range(2):
            a.push(s, caps[s][:cut])
        a.process()
        left = []
        for s in range(2):
            n = a.state(s).frames_released
            assert n >= 2
            fr, _, rec = a.pop_frames(s, cap=n - 1, link=True)
            assert len(fr) == n - 1 and rec["valid"].all()
            left.append(n - 1)                              # the frame that stays unpopped
        ring_a = device_ring(amd, a, cap_frames)
        assert all(ring_a[s, left[s]]["valid"] == 1 for s in range(2))
        for s in range(2):                                  # the destination slots hold records of their own before the import
            b.push(s, caps[s][:cut])
        b.process()
        assert (device_ring(amd, b, cap_frames)["valid"].sum(axis=1) >= 2).all()
        b.import_streams([1, 0], a.export_streams([0, 1]))  # stream 0 -> slot 1, stream 1 -> slot 0
        assert all_zero(device_ring(amd, b, cap_frames))
        for s in range(2):
            b.push(1 - s, caps[s][cut:])
            b.flush(1 - s)
        b.process()
        for s in range(2):
            fr, meta, rec = b.pop_frames(1 - s, link=True)
            assert len(fr) == 6 - left[s], (s, len(fr))
            assert all_zero(rec[0]) and np.array_equal(fr[0], tx[left[s]])       # travelled unpopped: valid = 0
            for k in range(1, len(fr)):
                m = link_model(oracle, b.soft(1 - s, first=int(meta["payload_symbol"][k]), cap=CODED))
                assert np.array_equal(m["frame"], fr[k]), (s, k)
                check_record(rec[k], m, ("import", s, k))
                assert rec[k]["valid"] == 1
        # ---- opv_reset_stream clears the slot's records, and only that slot's
        ring_b = device_ring(amd, b, cap_frames)
        assert ring_b[0]["valid"].sum() >= 2 and ring_b[1]["valid"].sum() >= 2
        b.reset(0)
        after = device_ring(amd, b, cap_frames)
        assert all_zero(after[0]) and after[1].tobytes() == ring_b[1].tobytes()
        # the source went on as before: its unpopped frame still has its record
        fr, _, rec = a.pop_frames(0, link=True)
        assert len(fr) == 1 and rec[0]["valid"] == 1 and rec[0].tobytes() == ring_a[0, left[0]].tobytes()
    finally:
        b.close()
        a.close()


# ------------------------------------------------------------------------------------------------ 6. misuse
def test_misuse_leaves_the_context_usable(amd, oracle):
    L = amd.lib()
    d = amd.Demod(3, max_samples=SMALL, streaming=True)
    try:
        soft = np.ascontiguousarray(S.payload(oracle, 0))
        rec = np.zeros(4, amd.LINK_DTYPE)
        out, meta = np.zeros((4, 134), np.uint8), np.zeros(4, amd.META_DTYPE)
        ptr = C.c_void_p()
        assert L.opv_enable_link_report(None, 1) == EINVAL
        assert L.opv_device_link(None, C.byref(ptr)) == EINVAL
        assert L.opv_pop_frames_link(None, 0, out.ctypes.data, 4, meta.ctypes.data, rec.ctypes.data) == EINVAL
        d.enable_link_report()
        assert L.opv_device_link(d.h, None) == EINVAL
        assert L.opv_device_link(d.h, C.byref(ptr)) == 0 and ptr.value
        for s in (3, -1):
            assert L.opv_pop_frames_link(d.h, s, out.ctypes.data, 4, meta.ctypes.data, rec.ctypes.data) == EINVAL
        assert L.opv_pop_frames_link(d.h, 0, out.ctypes.data, 4, meta.ctypes.data, None) == EINVAL
        assert L.opv_pop_frames_link(d.h, 0, out.ctypes.data, 4, meta.ctypes.data, rec.ctypes.data) == 0     # nothing to pop
        for args in ((None, soft.ctypes.data, 1, rec.ctypes.data), (d.h, None, 1, rec.ctypes.data),
                     (d.h, soft.ctypes.data, 1, None), (d.h, soft.ctypes.data, 0, rec.ctypes.data)):
            assert L.opv_link_payloads(*args) == EINVAL, args
        # still usable, stand-alone and in context
        r = d.link_payloads(soft)
        assert (r[0]["valid"], r[0]["bit_errors"], r[0]["weak"], r[0]["m1"], r[0]["ma"]) == (1, 0, 0, S.A, S.A)
        d.push_soft(1, S.cat(S.zeros(5), S.frame(oracle, 0), S.zeros(30))[:2200])
        d.process()
        fr, _, rec1 = d.pop_frames(1, link=True)
        assert len(fr) == 1 and rec1[0].tobytes() == r[0].tobytes()   # the in-context and the stand-alone kernel: the same bits
    finally:
        d.close()
