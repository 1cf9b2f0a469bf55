"""CPU-only: receive diversity's matching rule (opv_div_match, the host entry of csrc/opv_div_rules.h) held to the numpy model
tests/diversity_model.py; the struct layouts against gcc; the refusals that need no device; and - with the oracle alone - that
the made branch logs of the GPU tests (tests/diversity_inputs.py) are not vacuous: a group frame that every member branch decodes
wrongly alone and the combination decodes to the transmitted frame, and a frame with a strict subset of the branches; and that
the logs of tests/test_gpu_diversity_limits.py reach the edges they are named after (eight branches that need each other and show
the order of the sum, windows of 0 and 64 met and missed by one symbol, unequal losses on all eight lanes)."""
import re

import numpy as np
import pytest

import diversity_inputs as DI
import diversity_model as DM
from amd_lib import ROOT
from fixtures_built import amd  # noqa: F401
from struct_layout import check_ctypes_layout

EINVAL = -1
FSYMS = 2168
NAMES = ["opv_div_create", "opv_div_destroy", "opv_div_set_weights", "opv_div_round", "opv_div_pop_frames", "opv_div_get_state",
         "opv_div_tap_payload", "opv_div_match", "opv_div_earliest"]


def same_frames(got, exp, tag):
    """opv_div_match's frames (DIV_FRAME_DTYPE) == the model's"""
    assert len(got) == len(exp), (tag, len(got), len(exp))
    for k, (g, e) in enumerate(zip(got, exp)):
        assert int(g["anchor"]) == e["anchor"] and int(g["members"]) == e["members"], (tag, k, g, e)
        assert [int(v) for v in g["payload_symbol"]] == e["syms"], (tag, k, g, e)


def both(amd, recs, W, earliest=None, tag=""):
    e = [DM.ENDED] * len(recs) if earliest is None else earliest
    got, cur = amd.div_match(recs, e, W)
    exp, ecur = DM.match(recs, W, e)
    same_frames(got, exp, tag)
    assert [int(c) for c in cur] == ecur, (tag, cur, ecur)
    return exp


def random_lists(rng, B, W, n=12, base=1000):
    """B branches of one transmission of n frames: offsets inside the window, frames missing at random, a late start, an early
    end, a loss of lock (a gap) and a re-lock on a new grid"""
    off = rng.integers(0, W + 1, B) if W else np.zeros(B, np.int64)
    recs = []
    for b in range(B):
        first = int(rng.integers(0, 4)) if rng.random() < 0.4 else 0
        last = n - int(rng.integers(0, 4)) if rng.random() < 0.4 else n
        regrid = int(rng.integers(first, n)) if rng.random() < 0.3 else n
        syms = []
        for k in range(first, last):
            if rng.random() < 0.15:
                continue
            jump = int(rng.integers(-40, 700)) if k >= regrid else 0
            syms.append(base + FSYMS * k + int(off[b]) + jump)
        recs.append(sorted(set(syms)))
    return recs


def test_header_and_exports(amd):
    text = (ROOT / "include" / "opv_demod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in amd.EXPORTS and hasattr(amd.lib(), n), n
    assert re.search(r"#define OPV_ABI_VERSION 7\b", text) and amd.lib().opv_abi_version() == 7
    assert "restarts at the" in text                        # the reset / import rule is stated where a caller reads it


def test_struct_layouts(amd, tmp_path):
    check_ctypes_layout(tmp_path, amd.DivCfg, "opv_div_cfg", 16, ["n_groups", "window", "normalise", "reserved"])
    check_ctypes_layout(tmp_path, amd.DivState, "opv_div_state", 24,
                        ["frames_emitted", "frames_decoded", "frames_perfect", "records_lost", "softs_lost", "stalled"])
    off = check_ctypes_layout(tmp_path, amd.DivMeta, "opv_div_meta", 88,
                              ["payload_symbol", "members", "summed", "viterbi_metric", "sync_ok", "sync_quality"])
    assert off == {"payload_symbol": 0, "members": 64, "summed": 68, "viterbi_metric": 72, "sync_ok": 76, "sync_quality": 80}
    assert amd.DIV_META_DTYPE.itemsize == 88 and {f: amd.DIV_META_DTYPE.fields[f][1] for f in off} == off
    assert amd.DIV_REC_DTYPE.itemsize == 24 and amd.DIV_FRAME_DTYPE.itemsize == 80


def test_refusals_without_a_device(amd):
    L = amd.lib()
    import ctypes as C
    h = C.c_void_p()
    cfg = amd.DivCfg(1, 8, 0, 0)
    one = (C.c_int * 1)(1)
    assert L.opv_div_create(C.byref(h), None, C.byref(cfg), one, one) == EINVAL and not h.value
    assert L.opv_div_create(None, None, C.byref(cfg), one, one) == EINVAL
    for call in (lambda: L.opv_div_round(None), lambda: L.opv_div_set_weights(None, 0, None),
                 lambda: L.opv_div_get_state(None, 0, None), lambda: L.opv_div_pop_frames(None, 0, None, 0, None, None),
                 lambda: L.opv_div_tap_payload(None, 0, 0, None)):
        assert call() == EINVAL
    L.opv_div_destroy(None)                                 # a no-op
    for B, W in ((0, 8), (9, 8), (2, 65)):
        with pytest.raises(amd.OpvError):
            amd.div_match([[1]] * B, [DM.ENDED] * B, W)
    with pytest.raises(amd.OpvError):
        amd.div_match([[1, 2]], [DM.ENDED], 8, cursors=[3])  # a cursor beyond the list


def test_earliest_rule(amd):
    E = amd.div_earliest
    assert E(1, 1, 5000, 5001) == 5001 and E(1, 2, 5000, 7145) == 5001          # a pending payload starts behind its anchor
    assert E(0, 0, 0, 0) == 24 and E(0, 0, 0, 23) == 24 and E(0, 0, 77, 24) == 25 and E(0, 0, 0, 1 << 40) == (1 << 40) + 1
    assert E(0, 2, 5000, 7145) == 5000 + 2168 + 1
    assert E(0, 2, (1 << 32) - 5, 0) == (1 << 32) - 5 + 2169
    assert E(1, 2, 5000, 0, True) == DM.ENDED == amd.DIV_ENDED


@pytest.mark.parametrize("W", [0, 8, 64])
def test_window_edges_chains_and_ties(amd, W):
    p = 5000
    # offsets of exactly W (joined) and W + 1 (separate)
    f = both(amd, [[p], [p + W]], W, tag="joined")
    assert [x["members"] for x in f] == [3]
    f = both(amd, [[p], [p + W + 1]], W, tag="separate")
    assert [x["members"] for x in f] == [1, 2]
    # a chain A: p, B: p + W, C: p + 2 W: the anchor's window decides, C is a frame of its own (W = 0: all three are one)
    f = both(amd, [[p], [p + W], [p + 2 * W]], W, tag="chain")
    assert [x["members"] for x in f] == ([7] if W == 0 else [3, 4])
    # ties: every branch on the same symbol; the anchor is that symbol
    f = both(amd, [[p, p + FSYMS]] * 8, W, tag="tie")
    assert [(x["anchor"], x["members"]) for x in f] == [(p, 255), (p + FSYMS, 255)]
    # payload symbols across 2^32
    q = (1 << 32) - 3
    f = both(amd, [[q - FSYMS, q, q + FSYMS], [q - FSYMS + W, q + W, q + FSYMS + W]], W, tag="2^32")
    assert [x["members"] for x in f] == [3, 3, 3] and f[2]["syms"][1] == q + FSYMS + W > 1 << 32


@pytest.mark.parametrize("B", [1, 2, 3, 8])
def test_match_equals_the_model_on_random_lists_and_every_prefix_is_a_prefix(amd, B):
    rng = np.random.default_rng(100 + B)
    for trial in range(60):
        W = int(rng.choice([0, 1, 8, 64]))
        base = int(rng.choice([1000, (1 << 32) - 7 * FSYMS]))
        recs = random_lists(rng, B, W, base=base)
        final = both(amd, recs, W, tag=(B, trial))
        assert sum(bin(f["members"]).count("1") for f in final) == sum(len(r) for r in recs)     # every record in exactly one frame
        # rounds: prefixes of the lists with E_b anywhere up to the branch's true next payload; cursors carried from round to round
        cur, seen = [0] * B, []
        lens = [0] * B
        for _ in range(6):
            lens = [int(rng.integers(lens[b], len(recs[b]) + 1)) for b in range(B)]
            E = []
            for b in range(B):
                nxt = recs[b][lens[b]] if lens[b] < len(recs[b]) else None
                lo = recs[b][lens[b] - 1] + 1 if lens[b] else 0
                E.append(DM.ENDED if nxt is None and rng.random() < 0.5 else int(rng.integers(lo, (nxt if nxt is not None else lo + 3 * FSYMS) + 1)))
            pre = [recs[b][:lens[b]] for b in range(B)]
            got, cur2 = amd.div_match(pre, E, W, cursors=cur)
            exp, ecur = DM.match(pre, W, E, cursors=cur)
            same_frames(got, exp, (B, trial, "round"))
            assert [int(c) for c in cur2] == ecur
            cur = ecur
            seen += exp
            assert [(f["anchor"], f["members"]) for f in seen] == [(f["anchor"], f["members"]) for f in final[:len(seen)]], (B, trial)
        got, _ = amd.div_match(recs, [DM.ENDED] * B, W, cursors=cur)            # every branch has ended: the rest comes
        assert len(seen) + len(got) == len(final)
        assert [int(g["anchor"]) for g in got] == [f["anchor"] for f in final[len(seen):]]


def test_output_cap_stops_the_match_without_consuming(amd):
    recs = [[1000 + FSYMS * k for k in range(5)], [1003 + FSYMS * k for k in range(5)]]
    got, cur = amd.div_match(recs, [DM.ENDED] * 2, 8, cap=2)
    assert len(got) == 2 and list(cur) == [2, 2]
    rest, cur = amd.div_match(recs, [DM.ENDED] * 2, 8, cursors=cur)
    assert len(rest) == 3 and list(cur) == [5, 5]


@pytest.fixture(scope="module")
def groups(oracle):
    gs = DI.main_groups(oracle)
    return gs, [[DM.branch_records(oracle, b.soft) for b in g] for g in gs]


def test_made_logs_are_not_vacuous(oracle, groups):
    """among the GPU tests' logs: a group frame whose every member decodes to wrong bytes alone while the combination decodes to
    the transmitted frame; a frame with a strict subset of the branches; a flywheel member; a NaN that reaches a sum"""
    gs, recs = groups
    tx = oracle.bert_frames(DI.N_FRAMES)
    rescued = subset = flywheel = nan = 0
    for g, rr in zip(gs, recs):
        for f in DM.group_frames(oracle, rr, 8, want_link=False):
            k = (f["anchor"] - DI.LEAD + 2 - 24) // FSYMS
            n_mem = bin(f["members"]).count("1")
            subset += 0 < n_mem < len(g)
            flywheel += any(rr[b]["sync_ok"][i] == 0 and rr[b]["fscale"][i] > 0 for b, i in f["index"].items())
            nan += bool(np.isnan(f["payload"]).any())
            if n_mem < 2 or not 0 <= k < DI.N_FRAMES:
                continue
            alone_wrong = all(not np.array_equal(rr[b]["frames"][i], tx[k]) for b, i in f["index"].items())
            rescued += alone_wrong and f["metric"] >= 0 and np.array_equal(f["frame"], tx[k])
    assert rescued >= 1 and subset >= 1 and flywheel >= 1 and nan >= 1, (rescued, subset, flywheel, nan)


def test_iq_noise_level_of_the_gpu_test_shows_the_gain(oracle):
    """the real-IQ GPU test's channel settings, on the CPU with the oracle's own soft symbols (oracle_lib.channel_model is the
    device channel's model): every single-branch frame shows channel-bit errors, every combined frame no more than the better
    of its members, and fewer on at least one"""
    from link_model import link_model
    from oracle_lib import channel_model
    tx = oracle.bert_frames(6)
    clean = oracle.modulate(tx)
    recs = []
    for seed in (1, 2):
        r = oracle.receive(channel_model(clean, gain=0.25, f0_hz=0.0, sigma=4500.0, seed=seed), streaming=True)
        sym = [int(v) - 2143 for v in r["frame_sym"]]
        pl = [r["soft"][p:p + 2144] for p in sym]
        recs.append(dict(sym=sym, quality=[0.0] * len(sym), sync_ok=[1] * len(sym),        # (neither enters the sum)
                         fscale=[DM.seq_scale(p) for p in pl], payloads=pl))
    fr = DM.group_frames(oracle, recs, 8)
    assert len(fr) == 6 and all(f["members"] == 3 and f["summed"] == 3 for f in fr)
    single = [[link_model(oracle, recs[b]["payloads"][i])["bit_errors"] for b, i in sorted(f["index"].items())] for f in fr]
    comb = [f["link"]["bit_errors"] for f in fr]
    assert all(min(s) > 0 for s in single) and all(c <= min(s) for c, s in zip(comb, single)), (single, comb)
    assert any(c < min(s) for c, s in zip(comb, single))
    assert all(np.array_equal(f["frame"], tx[k]) for k, f in enumerate(fr))


# ---- the limits: what tests/test_gpu_diversity_limits.py runs on the device is not vacuous --------------------------------------
def test_eight_scattered_branches_need_each_other_and_the_order_of_the_sum_shows(oracle):
    """the group of eight (diversity_inputs.eight_groups): with unit weights every branch alone decodes frames 1-4 wrongly and the
    combination decodes all six; with EIGHT_WEIGHTS the sum in DESCENDING branch order - and the sum in stream order - differs in
    bits of the payload of every frame that carries a signal"""
    (g8, g5), _ = DI.eight_groups(oracle)
    recs = [DM.branch_records(oracle, b.soft) for b in g8]
    tx = oracle.bert_frames(DI.N_FRAMES)
    fr = DM.group_frames(oracle, recs, 8, want_link=False)
    assert [f["members"] for f in fr] == [0xFF] * 10 and [f["metric"] >= 0 for f in fr] == [True] * 6 + [False] * 4
    for k in range(DI.N_FRAMES):
        assert np.array_equal(fr[k]["frame"], tx[k]), k
        if k in DI.EIGHT_LOUD:
            assert all(not np.array_equal(recs[b]["frames"][k], tx[k]) for b in range(8)), k
    w = DI.EIGHT_WEIGHTS
    for k, f in enumerate(DM.group_frames(oracle, recs, 8, weights=w, want_link=False)[:DI.N_FRAMES]):
        for order in (sorted(f["index"], reverse=True), sorted(f["index"], key=lambda b: DI.EIGHT_STREAMS[b])):
            other = DM.combine([recs[b]["payloads"][f["index"][b]] for b in order], [w[b] for b in order])
            assert np.sum(other != f["payload"]) > 100, (k, order)
    assert sorted(DI.EIGHT_STREAMS) != DI.EIGHT_STREAMS and sorted(DI.FIVE_STREAMS) != DI.FIVE_STREAMS
    assert not set(DI.EIGHT_STREAMS) & set(DI.FIVE_STREAMS) and DI.NEIGHBOUR not in DI.EIGHT_STREAMS + DI.FIVE_STREAMS
    # the group of five: a strict subset while branch 1 hunts, another once branch 2 has ended
    f5 = DM.group_frames(oracle, [DM.branch_records(oracle, b.soft) for b in g5], 8, want_link=False)
    assert [f["members"] for f in f5] == [0x1D] * 2 + [0x1F] * 6 + [0x1B] * 2


def window_masks(W, shifts):
    inside = abs(shifts[0] - shifts[1]) <= W
    return [3] * 10 if inside else ([1, 2] if shifts[0] < shifts[1] else [2, 1]) * 10


@pytest.mark.parametrize("W,shifts", DI.WINDOW_CASES)
def test_window_0_and_64_logs_sit_on_both_sides_of_the_window(oracle, amd, W, shifts):
    recs = [DM.branch_records(oracle, b.soft) for b in DI.window_pair(oracle, shifts)]
    fr = both(amd, [r["sym"] for r in recs], W, tag=(W, shifts))
    assert [f["members"] for f in fr] == window_masks(W, shifts)
    assert all(f["syms"][1] - f["syms"][0] == shifts[1] - shifts[0] for f in fr if f["members"] == 3)


def test_eight_branches_that_ran_ahead_lose_unequally(oracle):
    """diversity_inputs.ahead_group in a context of 8 frame slots and 16 384 soft symbols: the per-branch record losses differ,
    lanes 4..7 contribute, and one emitted frame has members that are summed next to members whose payload has left its ring"""
    from diversity_runs import ahead_model
    g = DI.ahead_group(oracle)
    recs = [DM.branch_records(oracle, b.soft) for b in g]
    logs = [b.soft for b in g]
    alone = [ahead_model([r], [log], 1, 8, 16384)[0].records_lost for r, log in zip(recs, logs)]
    assert alone == [8, 8, 6, 8, 8, 5, 7, 8] and len(set(alone[4:])) > 1
    m, per = ahead_model(recs, logs, 3, 8, 16384)
    assert m.records_lost == sum(alone) == 58 and sum(alone[:4]) != m.records_lost
    assert [(len(out), lost, gone, stalled) for out, lost, gone, stalled in per] == [(8, 58, 17, 1), (3, 58, 17, 0), (0, 58, 17, 0)]
    assert len(set(len(log) for log in logs)) == 8
    mixed = [f for f in m.frames if f["soft_gone"] and f["members"] & ~f["soft_gone"]]
    assert [(f["members"], f["soft_gone"]) for f in mixed] == [(0xFF, 0x92)]
    assert any(f["members"] == f["soft_gone"] for f in m.frames) and any(f["members"] not in (0, 0xFF) and not f["soft_gone"] for f in m.frames)
