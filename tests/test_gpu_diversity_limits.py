"""Receive diversity on the device at the limits of what the code says it supports, and at far positions - the shapes that
tests/test_gpu_diversity.py does not reach, held the same way: made branch logs staged through opv_tap_push_soft, everything
compared with `==` against tests/diversity_model.py plus the oracle's decoder (combined payloads bit for bit through
opv_div_tap_payload, masks, payload symbols, bytes, metrics, link integers; the link's fp64 moments under
link_model.check_record's own bound).

  1. eight branches on scattered streams whose branch order is not stream order, unit and six-decade weights; five branches
     next to them; an ungrouped neighbour held to oracle.track
  2. windows of 0 and 64 symbols, on and one symbol outside the window
  3. 65 groups (one more than a k_div_scale block of 64 lanes) that emit 0, 1 and 2 frames in the same round
  4. a round whose grids were sized for ONE frame and that emits five
  5. eight branches that ran ahead by different amounts: unequal record losses on lanes 0..7, soft losses inside a frame
  6. branches imported from another context into a live group, with payload symbols across 2^32 and beyond 2^40 (real IQ)
  7. normalised mode at eight branches with one scale that is not finite

Every case asserts from the model (or, for 6, from the unshifted control run) that it reaches the edge it is named after before
the device's results are compared; tests/test_diversity_host.py shows the same for 1, 2 and 5 without a device. Every index the
kernels form here lies inside its ring: streams are checked by opv_div_create, the soft rings are indexed through their
power-of-two masks, the output rings through f % cap, and a restarted cursor is clamped to the stream's frame count."""
import numpy as np
import pytest

import diversity_inputs as DI
import diversity_model as DM
from diversity_runs import CODED, FSYMS, MID, Run, ahead_model, check_group, earliest, released, same
from far_probe import probe, shifted_blob  # noqa: F401
from fixtures import amd  # noqa: F401

pytestmark = pytest.mark.gpu


def held(oracle, r, g, exp, tag):
    """group g of a finished run == the model's frames, counters included; -> the frames the decoder kept"""
    kept = check_group(oracle, r.result(g), exp, tag)
    st = r.div.state(g)
    assert (st.frames_emitted, st.frames_decoded, st.records_lost, st.softs_lost, st.stalled) == (len(exp), len(kept), 0, 0, 0), tag
    assert st.frames_perfect == sum(e["metric"] == 0 for e in kept), tag
    return kept


# ------------------------------------------------------------------------------------------------ 1. eight scattered branches
@pytest.fixture(scope="module")
def eight(oracle):
    """the groups of eight and five, their branch records, the neighbour's track and the model's frames for both weightings:
    computed once, shared, never changed"""
    gs, nb = DI.eight_groups(oracle)
    recs = [[DM.branch_records(oracle, b.soft) for b in g] for g in gs]
    exp8 = {"unit": DM.group_frames(oracle, recs[0], 8), "weighted": DM.group_frames(oracle, recs[0], 8, weights=DI.EIGHT_WEIGHTS)}
    return gs, nb, recs, exp8, DM.group_frames(oracle, recs[1], 8), oracle.track(nb)


@pytest.mark.parametrize("weighting", ["unit", "weighted"])
def test_eight_branches_on_scattered_streams_in_branch_order(amd, oracle, eight, weighting):
    gs, nb, recs, exp8, exp5, nb_exp = eight
    exp = exp8[weighting]
    assert [e["members"] for e in exp] == [0xFF] * 10 and [e["summed"] for e in exp] == [0xFF] * 10
    assert [e["metric"] >= 0 for e in exp] == [True] * 6 + [False] * 4                 # four silent flywheel frames, dropped
    assert any(not same(a["payload"], b["payload"]) for a, b in zip(exp8["unit"], exp8["weighted"]))
    r = Run(amd, gs, MID, streams=[DI.EIGHT_STREAMS, DI.FIVE_STREAMS], n_streams=16, others={DI.NEIGHBOUR: nb})
    try:
        if weighting == "weighted":
            r.div.set_weights(0, DI.EIGHT_WEIGHTS)
        r.feed(1999)
        r.step(r.at)                                        # a final round with nothing new
        held(oracle, r, 0, exp, ("eight", weighting))
        kept5 = held(oracle, r, 1, exp5, ("five", weighting))
        assert {e["members"] for e in kept5} == {0x1D, 0x1F}
        # every branch was served as ever, whichever slot it sits in
        for g, streams in enumerate(r.streams):
            for b, s in enumerate(streams):
                keep = recs[g][b]["metrics"] >= 0
                assert same(np.concatenate(r.own[s][0]), recs[g][b]["frames"][keep]), (g, b, s)
        # the neighbour does not notice the groups
        fr, meta = np.concatenate(r.own[DI.NEIGHBOUR][0]), np.concatenate(r.own[DI.NEIGHBOUR][1])
        keep = nb_exp["metrics"] >= 0
        assert same(fr, nb_exp["frames"][keep]) and same(meta["viterbi_metric"], nb_exp["metrics"][keep])
        assert same(meta["release_symbol"], nb_exp["frame_sym"][keep]) and same(meta["payload_symbol"], nb_exp["frame_sym"][keep] - 2143)
        assert same(meta["sync_quality"], nb_exp["quality"][keep]) and same(meta["sync_ok"], nb_exp["sync_ok"][keep])
        st = r.d.state(DI.NEIGHBOUR)
        assert (st.total_symbols, st.sync_state, st.frames_released, st.stalled) == (nb_exp["n_soft"], nb_exp["final_state"], len(keep), 0)
        for s in (8, 15):                                   # and the idle streams stay idle
            assert r.d.state(s).total_symbols == 0 and r.d.state(s).frames_released == 0
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 2. windows of 0 and 64
@pytest.mark.parametrize("W,shifts", DI.WINDOW_CASES)
def test_window_0_and_64_on_and_outside_the_window(amd, oracle, W, shifts):
    g = DI.window_pair(oracle, shifts)
    recs = [DM.branch_records(oracle, b.soft) for b in g]
    exp = DM.group_frames(oracle, recs, W)
    inside = abs(shifts[0] - shifts[1]) <= W
    assert [e["members"] for e in exp] == ([3] * 10 if inside else ([1, 2] if shifts[0] < shifts[1] else [2, 1]) * 10)
    r = Run(amd, [g], MID, window=W)
    try:
        r.feed(2999)
        r.step(r.at)
        kept = held(oracle, r, 0, exp, ("window", W, shifts))
        assert len(kept) == (6 if inside else 12)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 3. many groups
def moved(exp, d):
    """the model's frames of a group whose every log has d zero symbols more in front"""
    return [dict(e, anchor=e["anchor"] + d, syms=[v + d if (e["members"] >> b) & 1 else 0 for b, v in enumerate(e["syms"])]) for e in exp]


def test_65_groups_emit_0_1_and_2_frames_in_one_round(amd, oracle):
    recipes = DI.many_recipes(oracle)
    recs = {n: [DM.branch_records(oracle, b.soft) for b in g] for n, g in recipes.items()}
    exp = {n: DM.group_frames(oracle, rr, 8) for n, rr in recs.items()}              # once per recipe, moved by the prefix below
    kind = [(DI.MANY_COUNTS[g % 5], (g % 7) * DI.MANY_PREFIX) for g in range(DI.MANY_GROUPS)]
    groups = [DI.prefixed(recipes[n], pre) for n, pre in kind]
    n_all = max(len(b.soft) for g in groups for b in g)
    ats = list(range(1999, n_all, 1999)) + [n_all, n_all]                            # Run.feed(1999) and a last round with nothing new
    per_round = {}
    for n, pre in set(kind):
        m = DM.Group(n, 8)
        syms = [[p + pre for p in rr["sym"]] for rr in recs[n]]
        per_round[n, pre] = [len(m.round([released(s, at) for s in syms], [earliest(s, at) for s in syms])) for at in ats]
        assert sum(per_round[n, pre]) == len(exp[n]), (n, pre)
    side_by_side = [i for i in range(len(ats)) if {0, 1, 2} <= {per_round[k][i] for k in kind}]
    assert side_by_side, "no round in which groups emit 0, 1 and 2 frames"
    assert sum(len(g) for g in groups) == 247 and DI.MANY_GROUPS == 65
    r = Run(amd, groups, MID)
    try:
        r.feed(1999)
        r.step(r.at)
        for g, k in enumerate(kind):
            assert r.emitted[g] == per_round[k], (g, k, r.emitted[g], per_round[k])
        assert all({0, 1, 2} <= {r.emitted[g][i] for g in range(DI.MANY_GROUPS)} for i in side_by_side)
        for g, (n, pre) in enumerate(kind):
            held(oracle, r, g, moved(exp[n], pre), ("many", g, n, pre))
        for g in (0, 63, 64):
            assert sum(r.pops[g]) >= 6 and sum(r.emitted[g]) >= 10, g
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 4. a backlog behind an estimate of 1
def test_a_round_sized_for_one_frame_emits_five(amd, oracle):
    """The output ring of eight fills and the group stalls; the branches go on (their own frames popped, their records waiting in
    the record rings of eight) until five group frames are final behind the stall. The group is popped and opv_div_round is called
    with no opv_process in between: its estimate is then exactly one frame per group, every grid has one block per group, and the
    five frames come from the kernels' strides - an odd count, so the last decoder pass has an idle half."""
    g = DI.backlog_pair(oracle)
    recs = [DM.branch_records(oracle, b.soft) for b in g]
    logs, syms = [b.soft for b in g], [rr["sym"] for rr in recs]
    assert [len(s) for s in syms] == [22, 22]
    model, emitted, popped = DM.Group(2, 8), [], 0
    r = Run(amd, [g], MID)

    def model_round():
        out = model.round([released(s, r.at) for s in syms], [earliest(s, r.at) for s in syms], free=8 - (len(emitted) - popped),
                          cap_frames=8, n_soft=[min(r.at, len(log)) for log in logs], cap_soft=16384)
        emitted.extend(out)
        st = r.div.state(0)
        assert (st.frames_emitted, st.records_lost, st.softs_lost, st.stalled) == (len(emitted), 0, 0, model.stalled), (r.at, len(emitted))
        return out
    try:
        while not model.stalled:                            # a round after every piece, the group never popped
            r.step(r.at + 1999, pop=False)
            model_round()
        assert len(emitted) == 8
        waiting = lambda: min(len(released(s, r.at)) for s in syms) - len(emitted)
        while waiting() < 5:                                # stalled: the branches' records wait
            r.step(r.at + 1999, pop=False)
            assert model_round() == [] and model.stalled == 1
        assert waiting() == 5 and r.at < len(logs[0]) - 3 * FSYMS
        r.collect()                                         # the pop ...
        assert r.pops[0] == [8]
        popped = 8
        r.div.round()                                       # ... and a round with nothing launched since the last one
        out = model_round()
        assert len(out) == 5 and model.stalled == 0
        r.collect()
        assert r.pops[0] == [8, 5] and r.emitted[0][-1] == 5
        popped = len(emitted)
        while r.at < len(logs[1]):
            r.step(min(len(logs[1]), r.at + 1999))
            model_round()
            popped = len(emitted)
        r.step(r.at)
        model_round()
        assert len(emitted) == 22
        exp = [DM.finish(oracle, f, recs, [1.0, 1.0], False) for f in emitted]
        kept = check_group(oracle, r.result(0), exp, "backlog")
        assert len(kept) == 18 and all(e["members"] == 3 and e["summed"] == 3 for e in exp)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 5. eight branches that ran ahead
def test_eight_branches_that_ran_ahead_by_different_amounts(amd, oracle):
    """test_a_branch_that_ran_ahead_loses_records_and_softs_counted at B = 8: logs of eight lengths, transmissions that end at six
    different frames, all run to their ends (the branches popped) before the first diversity round. The record rings of eight have
    lost 8, 8, 6, 8, 8, 5, 7 and 8 records; of the payloads still on record some have left the soft rings of 16 384 symbols, and
    in one emitted frame members 1, 4 and 7 have while the other five are summed."""
    g = DI.ahead_group(oracle)
    recs = [DM.branch_records(oracle, b.soft) for b in g]
    logs = [b.soft for b in g]
    model, per = ahead_model(recs, logs, 3, 8, 16384)
    alone = [ahead_model([rr], [log], 1, 8, 16384)[0].records_lost for rr, log in zip(recs, logs)]
    assert len(set(alone)) > 1 and all(alone[4:]) and len(set(alone[4:])) > 1 and sum(alone) == model.records_lost
    assert any(f["soft_gone"] and f["members"] & ~f["soft_gone"] for f in model.frames)
    assert [len(out) for out, *_ in per] == [8, 3, 0]
    r = Run(amd, [g], MID)
    try:
        r.feed(1999, rounds=False)
        for out, lost, gone, stalled in per:
            before = r.div.state(0).frames_emitted
            r.div.round()
            st = r.div.state(0)
            assert (st.frames_emitted - before, st.records_lost, st.softs_lost, st.stalled) == (len(out), lost, gone, stalled)
            r.collect()
        exp = [DM.finish(oracle, f, recs, [1.0] * 8, False) for f in model.frames]
        assert any(e["summed"] and e["summed"] != e["members"] for e in exp) and any(e["members"] and not e["summed"] for e in exp)
        kept = check_group(oracle, r.result(0), exp, "ahead")
        assert len(kept) >= 6
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 7. normalised mode at B = 8
def test_normalised_mode_at_eight_branches_with_a_scale_that_is_not_finite(amd, oracle):
    g = DI.normalised_eight(oracle)
    recs = [DM.branch_records(oracle, b.soft) for b in g]
    exp = DM.group_frames(oracle, recs, 8, normalise=True)
    plain = DM.group_frames(oracle, recs, 8, want_link=False)
    assert all(np.isnan(recs[5]["fscale"][k]) for k in range(DI.N_FRAMES))
    assert [(e["members"], e["summed"]) for e in exp[:DI.N_FRAMES]] == [(0xFF, 0xDF)] * DI.N_FRAMES
    assert all(np.isnan(p["payload"]).any() and not np.isnan(e["payload"]).any() for p, e in zip(plain[:DI.N_FRAMES], exp))
    r = Run(amd, [g], MID, normalise=True)
    try:
        r.feed(2500)
        r.step(r.at)
        kept = held(oracle, r, 0, exp, "normalised eight")
        assert len(kept) == DI.N_FRAMES and all(e["summed"] != e["members"] for e in kept)
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 6. imported branches, far positions
SLOTS = [9, 3]                                  # branch 0 and 1 of the group in the 12-stream destination
CUT = 3 * 86720 + 20000                         # samples fed at the source: about three frames
PIECE = 40000


@pytest.fixture(scope="module")
def receptions(oracle):
    return DI.two_receptions(oracle)


def far_run(amd, oracle, probe, xs, d_sym, created_after=False):
    """two receptions to CUT in a 2-stream source, exported, moved by d_sym symbols (and as many samples), imported into SLOTS of a
    12-stream destination with a diversity group over them; the rest in 40 000-sample pieces, a round after each. The group is
    held to the model built from the destination's OWN branch metas and soft symbols; -> what it handed out."""
    n = max(x.size // 2 for x in xs)
    src = amd.Demod(2, max_samples=n + 64, streaming=True)
    dst = amd.Demod(12, max_samples=n + 64, streaming=True)
    div = None
    try:
        n_src = []
        for at in range(0, CUT, PIECE):
            for s, x in enumerate(xs):
                src.push(s, x[2 * at: 2 * min(at + PIECE, CUT)])
            src.process()
        for s in range(2):
            n_src.append(len(src.pop_frames(s)[0]))
            assert n_src[s] == src.state(s).frames_released >= 2
        rc, blob = shifted_blob(probe, src.export_streams([0, 1]), d_sym, d_sym)
        assert rc == 0
        if not created_after:
            div = amd.Diversity(dst, [SLOTS])                   # alive before the import: the restart path of opv_div_round
        dst.import_streams(SLOTS, blob)
        if created_after:
            div = amd.Diversity(dst, [SLOTS])                   # its cursors start from the imported frame counts
        recs = [dict(sym=[], quality=[], sync_ok=[], fscale=[], payloads=[]) for _ in SLOTS]
        payloads, frames, meta, link = [], [], [], []
        pos, done = CUT, [False, False]
        while not all(done):
            for b, (s, x) in enumerate(zip(SLOTS, xs)):
                if pos < x.size // 2:
                    dst.push(s, x[2 * pos: 2 * min(pos + PIECE, x.size // 2)])
                elif not done[b]:
                    dst.flush(s)
                    done[b] = True
            pos += PIECE
            dst.process()
            for b, s in enumerate(SLOTS):
                _, m = dst.pop_frames(s)
                for row in m:
                    p = int(row["payload_symbol"])
                    pl = dst.soft(s, first=p, cap=CODED)
                    assert pl.size == CODED
                    recs[b]["sym"].append(p)
                    recs[b]["quality"].append(float(row["sync_quality"]))
                    recs[b]["sync_ok"].append(int(row["sync_ok"]))
                    recs[b]["fscale"].append(DM.seq_scale(pl))
                    recs[b]["payloads"].append(pl)
            div.round()
            st = div.state(0)
            payloads += [div.tap_payload(0, f) for f in range(len(payloads), st.frames_emitted)]
            f, m, l = div.pop_frames(0, link=True)
            frames.append(f)
            meta.append(m)
            link.append(l)
        st = div.state(0)
        assert (st.records_lost, st.softs_lost, st.stalled) == (0, 0, 0)
        got = (np.concatenate(frames), np.concatenate(meta), np.concatenate(link), payloads)
        exp = DM.group_frames(oracle, recs, 8)
        kept = check_group(oracle, got, exp, ("far", d_sym, created_after))
        # nothing released before the import is combined: every group frame pairs the k-th records released AFTER it
        assert n_src[0] == n_src[1] and len(kept) == len(exp) == 8 - n_src[0] == len(recs[0]["sym"]) == len(recs[1]["sym"])
        assert all(e["members"] == 3 and e["summed"] == 3 for e in exp)
        assert same(got[0], oracle.bert_frames(8)[n_src[0]:])
        return dict(frames=got[0], meta=got[1], link=got[2], payloads=payloads, n_src=n_src[0])
    finally:
        if div is not None:
            div.close()
        dst.close()
        src.close()


@pytest.fixture(scope="module")
def far_control(amd, oracle, probe, receptions):
    """the unshifted run: computed once, shared, never changed"""
    return far_run(amd, oracle, probe, receptions, 0)


def far_shift(case, ctl):
    """(d_sym, created_after) of a case, every placement asserted from the control run's payload symbols"""
    p = ctl["meta"]["payload_symbol"].astype(object)       # [frame][branch]
    pa, pb = int(p[1][0]), int(p[1][1])                     # the second frame released after the import
    assert pb - pa == DI.RECEPTION_DELAY // 40 == 3
    if case in ("anchor_below_member_above", "created_after_import"):
        d = ((1 << 32) - pb) & ~3
        assert pa + d < 1 << 32 <= pb + d
        return d, case == "created_after_import"
    if case == "payload_spans_2p32":
        d = ((1 << 32) - (pa + 1000)) & ~3
        assert pa + d < pb + d < 1 << 32 < pa + d + CODED - 1 < pb + d + CODED - 1
        return d, False
    if case == "beyond_2p40":
        return (1 << 40) + 8, False
    raise KeyError(case)


def test_branches_imported_into_a_live_group(far_control):
    """the control: no shift. Every frame released after the import is combined, none from before it (far_run asserts both)."""
    ctl = far_control
    assert 2 <= ctl["n_src"] <= 4 and len(ctl["frames"]) == 8 - ctl["n_src"]
    assert all(int(v) < 1 << 20 for v in ctl["meta"]["payload_symbol"][:, :2].reshape(-1))


@pytest.mark.parametrize("case", ["anchor_below_member_above", "payload_spans_2p32", "beyond_2p40", "created_after_import"])
def test_imported_branches_at_far_positions(amd, oracle, probe, receptions, far_control, case):
    ctl = far_control
    d_sym, created_after = far_shift(case, ctl)
    assert d_sym % 4 == 0 and d_sym >= 1 << 30
    far = far_run(amd, oracle, probe, receptions, d_sym, created_after)
    assert far["n_src"] == ctl["n_src"] and len(far["payloads"]) == len(ctl["payloads"])
    for a, b in zip(far["payloads"], ctl["payloads"]):
        assert a.tobytes() == b.tobytes(), case                                        # the same bits
    assert far["frames"].tobytes() == ctl["frames"].tobytes() and far["link"].tobytes() == ctl["link"].tobytes(), case
    for k in ("members", "summed", "viterbi_metric", "sync_ok", "sync_quality"):
        assert far["meta"][k].tobytes() == ctl["meta"][k].tobytes(), (case, k)
    a, b = far["meta"]["payload_symbol"].astype(object), ctl["meta"]["payload_symbol"].astype(object)
    assert [list(row[:2]) for row in a] == [[v + d_sym for v in row[:2]] for row in b] and not a[:, 2:].any(), case
