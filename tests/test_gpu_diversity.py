"""Receive diversity on the device (opv_div_*: k_div_match, k_div_combine and the thin scale / decode / link kernels behind them)
held to tests/diversity_model.py: made branch logs (tests/diversity_inputs.py) staged through opv_tap_push_soft, so every soft
symbol is exact and everything is compared with `==` - the combined payloads bit for bit (NaN positions included), the masks, the
payload symbols, bytes and metrics against the oracle's decoder on the model's payload, the link integers; the link's fp64
moments within the link report's own bound (tests/link_model.py). tests/test_diversity_host.py shows on the CPU that these logs
hold a frame only the combination decodes and frames with a strict subset of the branches."""
import numpy as np
import pytest

import diversity_inputs as DI
import diversity_model as DM
import soft_log_inputs as S
from diversity_runs import BIG, CODED, FSYMS, MID, SMALL, Run, check_group, same
from fixtures import amd  # noqa: F401
from stream_runs import code_of

pytestmark = pytest.mark.gpu
EINVAL, ECAPACITY, ESTATE = -1, -4, -6


@pytest.fixture(scope="module")
def main(oracle):
    """the three groups of the main test, their branch records and the model's frames: computed once, shared, never changed"""
    gs = DI.main_groups(oracle)
    recs = [[DM.branch_records(oracle, b.soft) for b in g] for g in gs]
    return gs, recs, [DM.group_frames(oracle, rr, 8) for rr in recs]


# ------------------------------------------------------------------------------------------------ 1. parity
def test_three_groups_equal_the_model(amd, oracle, main):
    gs, recs, exp = main
    r = Run(amd, gs, MID)
    try:
        r.feed(1999)
        r.step(r.at)                                        # a final round with nothing new
        for g in range(3):
            kept = check_group(oracle, r.result(g), exp[g], ("main", g))
            st = r.div.state(g)
            assert (st.frames_emitted, st.frames_decoded, st.records_lost, st.softs_lost, st.stalled) == (len(exp[g]), len(kept), 0, 0, 0), g
            assert st.frames_perfect == sum(e["metric"] == 0 for e in kept)
        assert any(0 < bin(e["members"]).count("1") < 3 for e in exp[0]) and any(np.isnan(e["payload"]).any() for e in exp[1])
        # the group of one branch hands out that stream's own frames
        fr, meta, _, _ = r.result(2)
        own_f, own_m = np.concatenate(r.own[5][0]), np.concatenate(r.own[5][1])
        assert same(fr, own_f) and same(meta["viterbi_metric"], own_m["viterbi_metric"])
        assert same(meta["payload_symbol"][:, 0], own_m["payload_symbol"]) and same(meta["sync_quality"], own_m["sync_quality"])
        assert same(meta["sync_ok"], own_m["sync_ok"]) and np.all(meta["members"] == 1) and np.all(meta["summed"] == 1)
        # and the branches themselves were served as ever
        for s, rr in enumerate([x for g in recs for x in g]):
            keep = rr["metrics"] >= 0
            assert same(np.concatenate(r.own[s][0]), rr["frames"][keep]), s
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 2. split independence
def test_one_piece_and_seven_odd_pieces_give_the_same_sequence(amd, oracle, main):
    gs, recs, exp = main
    n = len(gs[0][0].soft)
    whole = Run(amd, gs, BIG)
    parts = Run(amd, gs, BIG)
    try:
        whole.step(n)
        whole.step(n)
        cuts = [1, 2167, 2168 + 2191, 9001, 13339, 20011, n]           # seven odd pieces
        for c in cuts:
            parts.step(c)
        parts.step(n)
        for g in range(3):
            a, b = whole.result(g), parts.result(g)
            check_group(oracle, a, exp[g], ("whole", g))
            for x, y in zip(a[:3], b[:3]):
                assert x.tobytes() == y.tobytes(), g
            assert all(same(p, q) for p, q in zip(a[3], b[3])) and len(a[3]) == len(b[3])
            done = np.cumsum(parts.pops[g])                             # every intermediate pop is a prefix
            assert done[-1] == len(a[0]) and np.all(np.diff(done) >= 0)
            assert sum(1 for v in parts.pops[g] if v) > 1, parts.pops[g]
    finally:
        whole.close()
        parts.close()


# ------------------------------------------------------------------------------------------------ 3. normalised mode and weights
@pytest.fixture(scope="module")
def loud_group(oracle):
    rng = np.random.default_rng(5)
    g = [DI.Branch(DI.branch_log(oracle, rng, 0), 0), DI.Branch(DI.branch_log(oracle, rng, 3, amp=10 * S.A), 3, "10 x amplitude"),
         DI.Branch(DI.branch_log(oracle, rng, -2), -2)]
    return g, [DM.branch_records(oracle, b.soft) for b in g]


def test_normalised_mode(amd, oracle, loud_group):
    g, recs = loud_group
    exp = DM.group_frames(oracle, recs, 8, weights=[1.0, 0.5, 2.0], normalise=True)
    plain = DM.group_frames(oracle, recs, 8, want_link=False)
    assert any(not same(a["payload"], b["payload"]) for a, b in zip(exp, plain))
    r = Run(amd, [g], MID, normalise=True)
    try:
        r.div.set_weights(0, [1.0, 0.5, 2.0])
        r.feed(2500)
        r.step(r.at)
        kept = check_group(oracle, r.result(0), exp, "normalised")
        # (the silent flywheel frames behind the logs' ends have scale 0: matched, none summed, dropped)
        assert any(e["members"] and not e["summed"] for e in exp) and all(e["summed"] for e in kept)
    finally:
        r.close()


def test_weights_zero_and_a_change_between_rounds(amd, oracle, loud_group):
    g, recs = loud_group
    r = Run(amd, [g], MID)
    try:
        with pytest.raises(amd.OpvError) as e:
            r.div.set_weights(0, [1.0, -1.0, 1.0])
        assert code_of(e.value) == EINVAL
        with pytest.raises(amd.OpvError) as e:
            r.div.set_weights(0, [1.0, np.nan, 1.0])
        assert code_of(e.value) == EINVAL
        w0, w1 = [1.0, 0.0, 1.0], [0.25, 0.1, 3.0]
        r.div.set_weights(0, w0)
        while r.div.state(0).frames_emitted < 3:
            r.step(r.at + 1801)
        changed_at = r.div.state(0).frames_emitted
        r.div.set_weights(0, w1)
        r.feed(1801)
        r.step(r.at)
        exp = DM.group_frames(oracle, recs, 8, weights=lambda i: w0 if i < changed_at else w1)
        kept = check_group(oracle, r.result(0), exp, "weights")
        assert 3 <= changed_at < len(kept)
        assert any(e["summed"] != e["members"] and e["summed"] for e in kept[:changed_at])
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 4. stalls and losses
@pytest.fixture(scope="module")
def pair_group(oracle):
    rng = np.random.default_rng(9)
    g = [DI.Branch(DI.branch_log(oracle, rng, 0, loud=()), 0), DI.Branch(DI.branch_log(oracle, rng, 3, loud=()), 3)]
    return g, [DM.branch_records(oracle, b.soft) for b in g]


def test_a_full_output_ring_stalls_and_a_pop_resumes(amd, oracle, pair_group):
    g, recs = pair_group
    exp = DM.group_frames(oracle, recs, 8)
    r = Run(amd, [g], SMALL)
    try:
        while not r.div.state(0).stalled:                   # group frames are left unpopped until the ring of four is full
            r.step(r.at + 997, pop=False)
            assert r.at < len(g[0].soft)
        assert r.div.state(0).frames_emitted == 4
        r.div.round()                                       # still full: nothing emitted, nothing lost
        assert r.div.state(0).frames_emitted == 4 and r.div.state(0).stalled == 1
        r.collect()
        assert r.pops[0] == [4]
        r.div.round()                                       # the frame that was waiting in front of the full ring
        r.collect()
        assert r.pops[0] == [4, 1]
        r.feed(997)
        r.step(r.at)
        check_group(oracle, r.result(0), exp, "stall")
        st = r.div.state(0)
        assert (st.records_lost, st.softs_lost, st.stalled) == (0, 0, 0)
    finally:
        r.close()


def test_a_branch_that_ran_ahead_loses_records_and_softs_counted(amd, oracle):
    """ten frames per branch, the branches popped and run to their ends with no diversity round in between: six records of each
    have left the record ring of four, and of the four that remain three payloads have left the soft ring of 4096 symbols"""
    rng = np.random.default_rng(11)
    g = [DI.Branch(DI.branch_log(oracle, rng, sh, last=10, loud=(), n_frames=10, tail=40), sh) for sh in (0, 3)]
    recs = [DM.branch_records(oracle, b.soft) for b in g]
    n = len(g[0].soft)
    assert [len(rr["sym"]) for rr in recs] == [10, 10]
    r = Run(amd, [g], SMALL)
    try:
        r.feed(997, rounds=False)
        model = DM.Group(2, 8)
        syms = [rr["sym"] for rr in recs]
        earliest = [rr["sym"][-1] + FSYMS for rr in recs]   # both trackers end LOCKED, waiting for the eleventh sync word
        emitted = []
        for _ in range(2):
            r.div.round()
            st = r.div.state(0)
            emitted += model.round(syms, earliest, free=4 - len(emitted), cap_frames=4, n_soft=[n, n], cap_soft=4096)
            assert (st.frames_emitted, st.records_lost, st.softs_lost, st.stalled) == \
                (len(emitted), model.records_lost, model.softs_lost, model.stalled)
            r.collect(pop=False)
        r.collect()
        assert (model.records_lost, model.softs_lost, len(emitted)) == (12, 6, 4)
        exp = [DM.finish(oracle, f, recs, [1.0, 1.0], False) for f in emitted]
        assert [e["summed"] for e in exp] == [0, 0, 0, 3]
        kept = check_group(oracle, r.result(0), exp, "losses")
        assert len(kept) == 1 and np.array_equal(kept[0]["frame"], oracle.bert_frames(10)[9])
    finally:
        r.close()


# ------------------------------------------------------------------------------------------------ 6. refusals and lifetime
def test_refusals_and_a_detached_object(amd, oracle):
    d = amd.Demod(4, max_samples=SMALL, streaming=True)
    div = amd.Diversity(d, [[0, 1]])
    try:
        for groups, kw in (([[1, 2]], {}), ([[2, 2]], {}), ([[2, 4]], {}), ([[-1]], {}), ([[]], {}), ([[2]], dict(window=65)),
                           ([[2]], dict(window=-1)), ([], {})):
            with pytest.raises(amd.OpvError) as e:
                amd.Diversity(d, groups, **kw)
            assert code_of(e.value) == EINVAL, groups
        other = amd.Diversity(d, [[2], [3]], window=0)      # streams of no live object are free ...
        other.close()
        other = amd.Diversity(d, [[3, 2]], window=64)       # ... and again once their object has gone
        fr, meta = div.pop_frames(0)                        # a pop before any round
        assert len(fr) == 0 and div.state(0).frames_emitted == 0
        for call in (lambda: div.pop_frames(1), lambda: div.state(-1), lambda: div.tap_payload(0, 0), lambda: div.set_weights(0, [1.0])):
            with pytest.raises(amd.OpvError) as e:
                call()
            assert "one weight" in str(e.value) or code_of(e.value) == EINVAL
        d.close()                                           # the objects outlive their context
        for call in (div.round, lambda: div.pop_frames(0), lambda: div.state(0), lambda: div.set_weights(0, [1.0, 1.0]),
                     lambda: div.tap_payload(0, 0), other.round):
            with pytest.raises(amd.OpvError) as e:
                call()
            assert code_of(e.value) == ESTATE
    finally:
        other.close()
        div.close()
        d.close()


def test_reset_of_a_branch_mid_run(amd, oracle, pair_group):
    """branch 1 is reset after three frames and fed its whole log again, 700 symbols off branch 0's grid: the frames it releases
    after the reset are combined (alone: nothing of branch 0 lies within the window), nothing from before the reset is combined
    after it, and branch 0's remaining frames come alone too"""
    g, recs = pair_group
    log0, log1 = g[0].soft, g[1].soft
    cut = DI.LEAD + 3 * FSYMS + 400                         # three frames released on both branches, the fourth under way
    d = amd.Demod(2, max_samples=MID, streaming=True)
    div = amd.Diversity(d, [[0, 1]])
    try:
        def go(a0, a1):
            if a0.size:
                d.push_soft(0, a0)
            if a1.size:
                d.push_soft(1, a1)
            d.process()
            d.pop_frames(0)
            d.pop_frames(1)
            div.round()
            return div.pop_frames(0)
        got = [go(log0[:cut], log1[:cut])]
        assert [int(m) for m in got[0][1]["members"]] == [3, 3, 3]
        d.reset(1)
        again = S.cat(S.zeros(700), log1)
        rest = log0[cut:]
        for at in range(0, len(again), 3001):
            got.append(go(rest[at:at + 3001], again[at:at + 3001]))
        meta = np.concatenate([m for _, m in got])
        fr = np.concatenate([f for f, _ in got])
        after, fa = meta[3:], fr[3:]
        assert set(int(m) for m in after["members"]) == {1, 2}                            # none combined across the reset
        tx = oracle.bert_frames(DI.N_FRAMES)
        mine = after["members"] == 2
        assert [int(v) for v in after["payload_symbol"][mine, 1]] == [700 + DI.LEAD + 3 + 24 + FSYMS * k for k in range(6)]
        assert same(fa[mine], tx)                                                         # branch 1's six frames again, alone
        assert same(fa[~mine], tx[3:])                                                    # branch 0's frames 3, 4, 5, alone
        assert [int(v) for v in after["payload_symbol"][~mine, 0]] == [DI.LEAD + 24 + FSYMS * k for k in (3, 4, 5)]
        st = div.state(0)
        assert (st.records_lost, st.softs_lost) == (0, 0)
    finally:
        div.close()
        d.close()


# ------------------------------------------------------------------------------------------------ 5. real IQ
@pytest.mark.parametrize("frontend", [0, 4, 16])
def test_two_noisy_receptions_of_one_transmission(amd, oracle, frontend):
    """The same six frames through the device channel with two noise seeds, at a level where a single branch shows channel-bit
    errors in every frame (tests/oracle_lib.channel_model + the oracle on the CPU: 10 .. 26 per branch frame, 0 .. 2 combined).
    Samples are pushed and flushed; the model is built from the device's OWN soft symbols and branch metas, so the new kernels are
    held exactly; the gain of combining is asserted on the link records."""
    import torch
    tx = oracle.bert_frames(6)
    clean = oracle.modulate(tx)
    n = (clean.size // 2) & ~3
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(clean[:2 * n]).to(dev)
    d_out = torch.empty_like(d_in)
    d = amd.Demod(2, max_samples=n + 64, streaming=True)
    div = amd.Diversity(d, [[0, 1]])
    try:
        d.set_frontend(frontend)
        d.enable_link_report()
        for s, seed in enumerate((1, 2)):
            d.channel(d_in.data_ptr(), d_out.data_ptr(), n, gain=0.25, f0_hz=0.0, sigma=4500.0, seed=seed)
            d.sync()
            d.push(s, d_out.cpu().numpy())
            d.flush(s)
        d.process()
        div.round()
        recs, own = [], []
        for s in range(2):
            fr, meta, link = d.pop_frames(s, link=True)
            assert len(fr) == d.state(s).frames_released == 6, (s, len(fr))
            pl = [d.soft(s, first=int(p), cap=CODED) for p in meta["payload_symbol"]]
            recs.append(dict(sym=[int(p) for p in meta["payload_symbol"]], quality=[float(q) for q in meta["sync_quality"]],
                             sync_ok=[int(v) for v in meta["sync_ok"]], fscale=[DM.seq_scale(p) for p in pl], payloads=pl))
            own.append(link)
        exp = DM.group_frames(oracle, recs, 8)
        st = div.state(0)
        payloads = [div.tap_payload(0, f) for f in range(st.frames_emitted)]
        fr, meta, link = div.pop_frames(0, link=True)
        kept = check_group(oracle, (fr, meta, link, payloads), exp, ("iq", frontend))
        assert len(kept) == 6 and all(e["members"] == 3 and e["summed"] == 3 for e in kept) and same(fr, tx)
        singles = np.minimum(own[0]["bit_errors"], own[1]["bit_errors"])
        print("iq", frontend, "branch bit_errors", own[0]["bit_errors"], own[1]["bit_errors"], "combined", link["bit_errors"])
        assert np.all(own[0]["bit_errors"] > 0) and np.all(own[1]["bit_errors"] > 0)
        assert np.all(link["bit_errors"] <= singles) and np.any(link["bit_errors"] < singles)
    finally:
        div.close()
        d.close()
