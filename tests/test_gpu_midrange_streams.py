"""GPU: streaming contexts of 65 to 512 streams - the range k_msk_frontend_rb serves with two launch shapes under one name
(csrc/opv_round_rules.h, frontend_choice: 128 threads and an fp64 LDS ring a helper wave fills while the context has no more streams
than the device has CUs; 64 threads and the int16 ring beyond) - held to the ORACLE at length: every stream of every
context, every soft symbol, the chunk carry, the tracker's lines, the estimate and the final state, with the bounds
stream_checks.check_stream / events_match already carry. No comparison here is against another mapping of the product.

Inputs: workload.generate (per-stream payload, carrier offsets -2000 .. +2000 Hz with the two AFC-clamp streams in every 64,
16 dB), two sets, because a prefix of a capture has another EOF tail and therefore another oracle result:
  "long"  192 streams x 50 frames  (the 2048-sample ring wraps ~2100 times; AFC and timing loops long settled)
  "wide"  2 n_cu streams x 12 frames (> 500 wraps), of which the contexts of n_cu, n_cu + 1 and 2 n_cu streams read the first S
The oracle runs over both once (module fixture, a process pool over the job's host cores: none of them opens the GPU).

Which ring ran on either side of the CU boundary: the kernel's name is the same for both, and the library has no other
observable for it. So n_cu streams run twice - automatic (the fp64 ring, by opv_process' rule S <= n_cu) and with the
create-time hook OPV_FRONTEND_INT16_RING (the 64-thread shape, whatever the rule says) - and n_cu + 1 automatic (int16 by the
rule), all three against the oracle: both shapes are anchored at the boundary, whichever side the rule puts a context on."""
import threading
from concurrent.futures import ProcessPoolExecutor
from functools import partial

import pytest

from fixtures import amd  # noqa: F401
from soak_inputs import host_workers, oracle_receive_job
from stream_checks import check_stream, soft_err
from stream_runs import CHUNK, PIECES, collect, explain, make_demod

pytestmark = pytest.mark.gpu

EBN0 = 16.0
S_LONG, F_LONG = 192, 50
F_WIDE = 12


@pytest.fixture(scope="module")
def mid(amd):
    """both capture sets in HBM, the "long" one on the host too, and the oracle's result for every capture"""
    import time
    import torch
    from __graft_entry__ import load_pkg_module
    workload = load_pkg_module("workload")
    dev = torch.device("cuda", 0)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cu >= S_LONG, f"{n_cu} CUs: the {S_LONG}-stream contexts below are meant to be on the fp64 ring (S <= CUs)"
    sets = {}
    t0 = time.perf_counter()
    gen = amd.Demod(1, max_samples=1 << 16, streaming=True)
    try:
        for name, S, F in (("long", S_LONG, F_LONG), ("wide", 2 * n_cu, F_WIDE)):
            d_iq, _tx, n = workload.generate(amd, gen, torch, dev, range(S), F, EBN0)
            sets[name] = dict(S=S, F=F, n=n, d_iq=d_iq, host=d_iq.cpu().numpy())
    finally:
        gen.close()
    t1 = time.perf_counter()
    with ProcessPoolExecutor(host_workers()) as pool:
        for s in sets.values():
            s["exp"] = list(pool.map(partial(oracle_receive_job, want_soft=True), [s["host"][k] for k in range(s["S"])], chunksize=2))
    t2 = time.perf_counter()
    del sets["wide"]["host"]                                   # (only the pushes of the long set read host memory later)
    for name, s in sets.items():
        # the inputs are not vacuous - said by the ORACLE, before the product has seen them
        per = [len(e["frames"]) for e in s["exp"]]
        assert min(per) >= 1 and sum(per) >= 0.95 * s["S"] * (s["F"] - 1), (name, min(per), sum(per))
        assert all(e["n_soft"] == len(e["soft"]) for e in s["exp"])
        print(f"set {name}: {s['S']} streams x {s['F']} frames ({s['n']} samples), oracle frames {sum(per)}")
    print(f"captures generated and copied in {t1 - t0:.1f} s, oracle in {t2 - t1:.1f} s over {host_workers()} processes; {n_cu} CUs")
    sets["n_cu"] = n_cu
    yield sets
    sets.clear()
    torch.cuda.empty_cache()


def check_context(amd, d, exps, tag):
    """EVERY stream of context d against the oracle's result for its capture: check_stream in full (frames, metrics, release
    symbols, events and their printed lines, symbol count, all soft symbols < SOFT_TIGHT, estimate ==, final frequency, tracker
    state, chunk log), nothing stalled, no edge ties; the offset search's near-tie guard counted as
    test_512_stream_context_vs_oracle counts it (at most 4 of 512 streams guarded, scaled)."""
    S = len(exps)
    assert d.n_streams == S
    guarded, worst, worst_k = 0, -1.0, None
    for k, exp in enumerate(exps):
        got = collect(d, k)
        try:
            assert got["state"].stalled == 0, f"{tag} stream {k}: stalled 0x{got['state'].stalled:x}"
            check_stream(amd, got, exp, f"{tag} stream {k}", edge_ties=0, offset_ties=None)
        except AssertionError:
            explain(d, k, got, exp, f"{tag} stream {k}")
            raise
        guarded += got["state"].offset_ties > 0
        a, _ = soft_err(got["soft"], exp["soft"])
        if a > worst:
            worst, worst_k = a, k
    print(f"{tag}: {S} streams, worst soft max|d|/mean|soft| = {worst:.3e} on stream {worst_k}; near-tie guard fired on {guarded}")
    assert guarded <= max(1, S // 128), (tag, guarded)
    return worst, worst_k


def attach_all(d, s, first, S):
    for k in range(S):
        d.attach(k, s["d_iq"][first + k].data_ptr(), s["n"], eof=True)


# ------------------------------------------------------------------ parts 1 and 2
@pytest.mark.parametrize("which", ["192", "n_cu", "n_cu_int16_ring", "n_cu_plus_1", "2_n_cu"])
def test_every_stream_and_soft_symbol_vs_oracle(amd, mid, monkeypatch, which):
    """A streaming context of S streams, its captures attached whole, one opv_process: every stream in full against the oracle
    (check_context). S = 192 x 50 frames (the stream count from which the north-star rate is met; fp64 ring), S = n_cu (the last
    context on the fp64 ring: every CU holds a 98 KB workgroup), the same with the int16 ring forced (the 64-thread shape's
    direct oracle anchor at <= n_cu streams), S = n_cu + 1 (the first context the rule gives the int16 ring, LDS taken
    dynamically) and S = 2 n_cu (512 on an MI355X: the last stream count of this kernel), 12 frames each."""
    n_cu = mid["n_cu"]
    S = {"192": S_LONG, "n_cu": n_cu, "n_cu_int16_ring": n_cu, "n_cu_plus_1": n_cu + 1, "2_n_cu": 2 * n_cu}[which]
    s = mid["long" if which == "192" else "wide"]
    assert S <= s["S"]
    d = make_demod(amd, monkeypatch, which == "n_cu_int16_ring", S, max_samples=s["n"] + 64, streaming=True)
    try:
        attach_all(d, s, 0, S)
        d.process()
        d.sync()
        assert d.frontend_kernel() == "k_msk_frontend_rb"
        check_context(amd, d, s["exp"][:S], f"{which} (S = {S}, {s['F']} frames)")
    finally:
        d.close()


# ------------------------------------------------------------------ part 3
def test_192_streams_fed_in_odd_pushes_over_many_rounds(amd, mid):
    """The 192 x 50-frame contexts fed the way a live server feeds them: opv_push_iq in rounds, opv_process + opv_sync after each,
    opv_flush behind a stream's last samples, pops only at the end. The push sizes cycle through PIECES - the same for every
    stream of a round, but stream k's first push is k % 41 samples shorter, so that chunk origin and leftover differ across the
    workgroups of every launch. A streaming result does not depend on how the samples arrived (the chunker cuts at multiples of
    86 720 samples of the stream, reference src/opv-demod.cpp:1021-1076; test_incremental_push_equals_one_shot says it for one
    stream), so every stream must meet the SAME oracle result as the attached run, the chunk log included."""
    s = mid["long"]
    S, n, host = s["S"], s["n"], s["host"]
    assert any(p < 40 for p in PIECES) and any(p % 4 for p in PIECES) and {CHUNK - 1, CHUNK, CHUNK + 1} <= set(PIECES)
    assert any(p > 100000 and all(p % q for q in range(2, int(p ** 0.5) + 1)) for p in PIECES) and any(p % 256 == 0 for p in PIECES)
    d = amd.Demod(S, max_samples=n + 64, streaming=True)
    try:
        at, flushed, rounds = [0] * S, [False] * S, 0
        while not all(flushed):
            piece = PIECES[rounds % len(PIECES)]
            for k in range(S):
                m = min(piece - (k % 41 if rounds == 0 else 0), n - at[k])
                if m > 0:
                    d.push(k, host[k, 2 * at[k]: 2 * (at[k] + m)])
                    at[k] += m
                if at[k] == n and not flushed[k]:
                    d.flush(k)
                    flushed[k] = True
            d.process()
            d.sync()
            assert d.frontend_kernel() == "k_msk_frontend_rb", rounds
            rounds += 1
        print(f"{S} streams x {n} samples in {rounds} rounds")
        assert rounds >= 12
        check_context(amd, d, s["exp"], f"pushed in {rounds} rounds (S = {S}, {s['F']} frames)")
    finally:
        d.close()


# ------------------------------------------------------------------ part 4
def test_two_192_stream_contexts_competing_for_the_cus(amd, mid):
    """Two contexts of 192 streams in one process, each driven by its own host thread (attach, opv_process, opv_sync), released
    together: 384 workgroups of 98 KB of LDS for n_cu CUs, so workgroups of one context wait for the other's to leave. Ordinary
    use (two ranks of a server sharing a GPU); three repetitions with opv_reset_stream(-1) in between, every stream of both
    contexts in full against the oracle each time."""
    s, n_cu = mid["wide"], mid["n_cu"]
    S, firsts = 192, (0, n_cu)
    assert n_cu + S <= s["S"]
    ctxs = [amd.Demod(S, max_samples=s["n"] + 64, streaming=True) for _ in firsts]
    gate = threading.Barrier(len(ctxs))
    try:
        for rep in range(3):
            failed = [None] * len(ctxs)

            def work(i):
                try:
                    if rep:
                        ctxs[i].reset(-1)
                    attach_all(ctxs[i], s, firsts[i], S)
                    gate.wait(timeout=120)
                    ctxs[i].process()
                    ctxs[i].sync()
                except BaseException as e:           # surfaces in the main thread below
                    failed[i] = e
                    gate.abort()

            th = [threading.Thread(target=work, args=(i,)) for i in range(len(ctxs))]
            for t in th:
                t.start()
            for t in th:
                t.join()
            assert failed == [None] * len(ctxs), failed
            for i, d in enumerate(ctxs):
                assert d.frontend_kernel() == "k_msk_frontend_rb"
                check_context(amd, d, s["exp"][firsts[i]: firsts[i] + S], f"rep {rep} context {i} (captures {firsts[i]}..{firsts[i] + S - 1})")
    finally:
        for d in ctxs:
            d.close()
