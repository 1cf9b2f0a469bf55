"""CPU model of receive diversity (include/opv_demod.h: opv_div_*), built on numpy and the oracle alone.

    match(records, window, earliest=None, cursors=None)  the matching rule over per-branch lists of payload symbols
    Group(n_branches, window)                             the same rule round by round, with the rings' losses and the stall
    branch_records(oracle, soft)                          a branch log's frame records and payloads from oracle.track
    combine(payloads, factors)                            the sum in the stated order, one rounding per operation
    group_frames(oracle, branches, window, ...)           everything a group emits for complete branch logs

The rule, as csrc/opv_div_rules.h states it: the anchor p0 is the smallest payload symbol among the branches' next unconsumed
records; the frame is final once every branch without an unconsumed record has E_b > p0 + window; members are the branches
whose next record starts within `window` of p0."""
import numpy as np

import link_model

CODED = 2144
FSYMS = 2168
ENDED = 0xFFFFFFFFFFFFFFFF


class Group:
    """cursors, counters and the emitted frames of one group; round() is one k_div_match"""

    def __init__(self, n_branches, window):
        self.B, self.W = n_branches, window
        self.cursor = [0] * n_branches
        self.records_lost = self.softs_lost = 0
        self.stalled = 0
        self.frames = []                                    # dict(anchor, members, syms, soft_gone, index=[record index per branch])

    def round(self, syms, earliest, free=None, cap_frames=None, n_soft=None, cap_soft=None):
        """syms[b]: payload symbols of ALL records branch b has released so far; earliest[b]: E_b (ENDED: none will come);
        free: free slots of the output ring (None: unbounded); cap_frames: slots of the branches' record rings; n_soft[b] /
        cap_soft: for the payloads that have left their soft ring. Returns the frames emitted by this round."""
        out = []
        self.stalled = 0
        if cap_frames is not None:
            for b in range(self.B):
                behind = len(syms[b]) - self.cursor[b]
                if behind > cap_frames:
                    self.records_lost += behind - cap_frames
                    self.cursor[b] = len(syms[b]) - cap_frames
        while True:
            have = [b for b in range(self.B) if self.cursor[b] < len(syms[b])]
            if not have:
                break
            nxt = {b: int(syms[b][self.cursor[b]]) for b in have}
            p0 = min(nxt.values())                          # (a tie: the lowest branch, the same p0)
            if any(int(earliest[b]) != ENDED and int(earliest[b]) <= p0 + self.W for b in range(self.B) if b not in nxt):
                break
            if free is not None and len(out) >= free:
                self.stalled = 1
                break
            mem = [b for b in have if nxt[b] - p0 <= self.W]
            gone = [b for b in mem if n_soft is not None and nxt[b] + cap_soft < n_soft[b]]
            self.softs_lost += len(gone)
            f = dict(anchor=p0, members=sum(1 << b for b in mem), syms=[nxt.get(b, 0) if b in mem else 0 for b in range(8)],
                     soft_gone=sum(1 << b for b in gone), index={b: self.cursor[b] for b in mem})
            for b in mem:
                self.cursor[b] += 1
            out.append(f)
        self.frames += out
        return out


def match(records, window, earliest=None, cursors=None):
    """(frames, cursors) of one round over the given record lists; earliest defaults to "every branch has ended" """
    g = Group(len(records), window)
    if cursors is not None:
        g.cursor = [int(c) for c in cursors]
    g.round(records, [ENDED] * len(records) if earliest is None else earliest)
    return g.frames, g.cursor


def seq_scale(payload):
    """the decoder's scale: the SEQUENTIAL sum of |soft| in index order / 2144 (np.cumsum adds in order)"""
    with np.errstate(over="ignore", invalid="ignore"):
        return float(np.cumsum(np.abs(np.asarray(payload, np.float64)))[-1] / CODED)


def branch_records(oracle, soft):
    """oracle.track of one branch log -> dict(sym, quality, sync_ok, fscale, payloads, metrics, frames, final_state)"""
    t = oracle.track(soft)
    return dict(sym=[int(v) - (CODED - 1) for v in t["frame_sym"]], quality=[float(v) for v in t["quality"]],
                sync_ok=[int(v) for v in t["sync_ok"]], fscale=[seq_scale(p) for p in t["payloads"]], payloads=t["payloads"],
                metrics=t["metrics"], frames=t["frames"], final_state=t["final_state"])


def factor(w, normalise, fscale):
    if not w > 0.0:
        return 0.0
    if not normalise:
        return float(w)
    if not (fscale > 0.0 and np.isfinite(fscale)):
        return 0.0
    return float(np.float64(w) / np.float64(fscale))


def combine(payloads, factors):
    """e_0 * p_0, then + e_b * p_b in the given order: separate IEEE multiplications and additions"""
    if not payloads:
        return np.zeros(CODED, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        acc = np.float64(factors[0]) * np.asarray(payloads[0], np.float64)
        for e, p in zip(factors[1:], payloads[1:]):
            acc = acc + np.float64(e) * np.asarray(p, np.float64)
    return acc


def finish(oracle, f, recs, weights, normalise, want_link=True):
    """a matched frame `f` (Group.round) -> its sum, decode and link fields; recs[b] = branch_records or an equivalent dict"""
    summed, pl, fac, ok, q = 0, [], [], 0, None
    for b in sorted(f["index"]):
        k = f["index"][b]
        if (f["soft_gone"] >> b) & 1:
            continue
        e = factor(weights[b], normalise, recs[b]["fscale"][k])
        if e == 0.0:
            continue
        summed |= 1 << b
        pl.append(recs[b]["payloads"][k])
        fac.append(e)
        ok |= int(recs[b]["sync_ok"][k] != 0)
        qb = recs[b]["quality"][k]
        if q is None or qb > q:
            q = qb
    payload = combine(pl, fac)
    out = dict(f, summed=summed, payload=payload, sync_ok=ok, sync_quality=0.0 if q is None else q)
    if want_link:
        out["link"] = link_model.link_model(oracle, payload)
        out["metric"], out["frame"] = out["link"]["metric"], out["link"]["frame"]
    else:
        d = oracle.frame_decode(payload)
        out["metric"], out["frame"] = d["metric"], d["frame"]
    return out


def group_frames(oracle, recs, window, weights=None, normalise=False, want_link=True):
    """every frame a group emits once all its branches have ended; weights: [B] or a function of the emitted frame's index"""
    frames, _ = match([r["sym"] for r in recs], window)
    out = []
    for i, f in enumerate(frames):
        w = [1.0] * len(recs) if weights is None else (weights(i) if callable(weights) else weights)
        out.append(finish(oracle, f, recs, w, normalise, want_link))
    return out
