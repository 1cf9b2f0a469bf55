"""How the GPU modules of receive diversity RUN a context with a diversity object and hold what a group handed out to
tests/diversity_model.py, one definition each (tests/test_gpu_diversity.py, tests/test_gpu_diversity_limits.py). Needs no device
to import.

    Run(amd, groups, max_samples, ...)      one context, one diversity object, made branch logs pushed in pieces
    check_group(oracle, got, exp, tag)      a group's payloads, masks, symbols, decode and link records == the model's frames
    released(syms, at) / earliest(syms, at) what a made log's tracker has released, and its E_b, once `at` symbols were consumed
"""
import numpy as np

import diversity_model as DM
from link_model import check_record

SMALL = 32                                     # max_samples: cap_soft 4096, cap_frames 4
MID = 330000                                   # cap_soft 16384, cap_frames 8
BIG = 1000000                                  # cap_soft 32768, cap_frames 16: a whole branch log in one push
CODED, FSYMS = 2144, 2168


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and (np.array_equal(a, b, equal_nan=True) if a.dtype.kind == "f" else np.array_equal(a, b))


class Run:
    """one context, one diversity object: pushes branch logs in pieces, a process + round after each, and keeps what came out.
    streams: the context's stream of every branch, [[...], ...] (default: consecutive, in group and branch order); n_streams: the
    context's size (default: one per branch); others: {stream: soft log} of ungrouped streams fed in the same calls"""

    def __init__(self, amd, groups, max_samples, window=8, normalise=False, streams=None, n_streams=None, others=None):
        self.amd = amd
        self.logs = [b.soft for g in groups for b in g]
        if streams is None:
            ids, streams = iter(range(len(self.logs))), []
            for g in groups:
                streams.append([next(ids) for _ in g])
        self.streams = [list(g) for g in streams]
        flat = [s for g in self.streams for s in g]
        assert len(flat) == len(self.logs) and [len(g) for g in self.streams] == [len(g) for g in groups]
        self.by_stream = dict(zip(flat, self.logs))
        for s, log in (others or {}).items():
            assert s not in self.by_stream
            self.by_stream[s] = log
        self.d = amd.Demod(n_streams or len(self.logs), max_samples=max_samples, streaming=True)
        self.div = amd.Diversity(self.d, self.streams, window=window, normalise=normalise)
        G = len(groups)
        self.frames, self.meta, self.link = [[] for _ in range(G)], [[] for _ in range(G)], [[] for _ in range(G)]
        self.payloads, self.tapped, self.pops = [[] for _ in range(G)], [0] * G, [[] for _ in range(G)]
        self.emitted = [[] for _ in range(G)]               # group frames emitted per collect()
        self.own = {s: ([], []) for s in self.by_stream}    # the streams' own pops
        self.at = 0

    def close(self):
        self.div.close()
        self.d.close()

    def pop_branches(self):
        for s in self.by_stream:
            f, m = self.d.pop_frames(s)
            self.own[s][0].append(f)
            self.own[s][1].append(m)

    def collect(self, pop=True):
        for g in range(len(self.streams)):
            st = self.div.state(g)
            self.emitted[g].append(st.frames_emitted - self.tapped[g])
            for f in range(self.tapped[g], st.frames_emitted):
                self.payloads[g].append(self.div.tap_payload(g, f))
            self.tapped[g] = st.frames_emitted
            if pop:
                f, m, l = self.div.pop_frames(g, link=True)
                self.frames[g].append(f)
                self.meta[g].append(m)
                self.link[g].append(l)
                self.pops[g].append(len(f))

    def step(self, upto, rounds=True, pop=True, pop_branches=True):
        """symbols [at, upto) of every log, one process, one diversity round"""
        for s, log in self.by_stream.items():
            if log[self.at:upto].size:
                self.d.push_soft(s, log[self.at:upto])
        self.at = upto
        self.d.process()
        if pop_branches:
            self.pop_branches()
        if rounds:
            self.div.round()
            self.collect(pop)

    def feed(self, piece, **kw):
        n = max(len(log) for log in self.by_stream.values())
        while self.at < n:
            self.step(min(n, self.at + piece), **kw)

    def result(self, g):
        return (np.concatenate(self.frames[g]), np.concatenate(self.meta[g]), np.concatenate(self.link[g]), self.payloads[g])


def check_group(oracle, got, exp, tag, moments=True):
    """what a group handed out == the model's frames `exp` (diversity_model.finish): payloads of EVERY emitted frame, the rest for
    the frames the decoder did not drop"""
    fr, meta, link, payloads = got
    assert len(payloads) == len(exp), (tag, len(payloads), len(exp))
    for i, (p, e) in enumerate(zip(payloads, exp)):
        assert same(p, e["payload"]), (tag, i, "payload")
    kept = [e for e in exp if e["metric"] >= 0]
    assert len(fr) == len(kept), (tag, len(fr), len(kept))
    for i, e in enumerate(kept):
        m = meta[i]
        assert int(m["members"]) == e["members"] and int(m["summed"]) == e["summed"], (tag, i, m, e["members"], e["summed"])
        assert [int(v) for v in m["payload_symbol"]] == e["syms"], (tag, i)
        assert int(m["sync_ok"]) == e["sync_ok"] and same(m["sync_quality"], np.float64(e["sync_quality"])), (tag, i, m)
        assert int(m["viterbi_metric"]) == e["metric"] and same(fr[i], e["frame"]), (tag, i, "decode")
        if "link" in e:
            check_record(link[i], e["link"], (tag, i))
    return kept


# ---- a made log's tracker once it has consumed the log's first `at` symbols (tests/diversity_inputs.py: clean sync words) ----
def released(syms, at):
    """the payload symbols of the records released so far: a payload that starts at p is released ON symbol p + 2143"""
    return [int(p) for p in syms if int(p) + CODED - 1 < at]


def earliest(syms, at):
    """E_b as the matching rule needs it. While a record is still to come the tracker is collecting it, or LOCKED and about to
    check its sync word: both give E_b = that payload's first symbol (csrc/opv_div_rules.h: opv_div_earliest_of). Behind the last
    record (LOCKED on silence, then HUNTING at the log's end) E_b lies behind every record of the group: it never delays a decision,
    which the rule treats like a branch that has ended. A branch that is HUNTING (before its first sync word, or through erased
    ones) has E_b about `at`, while every record released so far starts 2144 symbols or more in front of `at`: it delays nothing
    either, and neither does the first payload symbol still to come that stands in for it here."""
    later = [int(p) for p in syms if int(p) + CODED - 1 >= at]
    return later[0] if later else DM.ENDED


HUNTING, LOCKED = 0, 2


def ends(recs, logs):
    """E_b of every branch whose WHOLE log its tracker has consumed (recs: diversity_model.branch_records of the logs). A tracker
    that ends LOCKED checks its next sync word 2168 symbols behind the last one, or is collecting the flywheel payload behind a
    missed one: either way E_b = the last record's payload symbol + 2168. One that ends HUNTING has E_b behind its log's last
    window, which lies behind every record of the group plus the window: the decisions do not depend on the exact value."""
    out = []
    for r, log in zip(recs, logs):
        assert r["final_state"] in (HUNTING, LOCKED)
        out.append(r["sym"][-1] + FSYMS if r["final_state"] == LOCKED else len(log) - 23)
    return out


def ahead_model(recs, logs, rounds, cap_frames, cap_soft, window=8):
    """branches that ran to their logs' ends before the first diversity round, then `rounds` rounds with every emitted frame
    popped after each -> (Group, [(frames of the round, records_lost, softs_lost, stalled), ...])"""
    m = DM.Group(len(recs), window)
    syms, E, n = [r["sym"] for r in recs], ends(recs, logs), [len(log) for log in logs]
    per = []
    for _ in range(rounds):
        out = m.round(syms, E, free=cap_frames, cap_frames=cap_frames, n_soft=n, cap_soft=cap_soft)
        per.append((out, m.records_lost, m.softs_lost, m.stalled))
    return m, per
