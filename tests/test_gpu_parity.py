"""GPU parity tests (run with -m gpu on an MI355X): the HIP path, called through the C ABI
(include/opv_demod.h), against the CPU oracle and the reference-made golden fixtures.

Bars: decoded bytes, Viterbi metrics/decisions, sync positions and event lines bit-exact;
soft symbols within 1e-5 relative (north_star) — we assert a much tighter 1e-9 on the
scale-normalised error and report the measured value.
"""
import hashlib
import os
from pathlib import Path

import numpy as np
import pytest

from fixtures import amd  # noqa: F401
from hostile_inputs import AFC_ALPHA_FLAG, EXTREME_FLAGS, extreme_flags_capture, fuzz_captures, near_tie_captures, staged_ties_capture
from oracle_lib import CODED_BITS, FRAME_BYTES, Oracle, channel_model, impair, resample_clock
from soak_inputs import pathological_captures
from stream_checks import SOFT_RTOL, SOFT_TIGHT, _gapped_capture, _visible_gpus, check_stream, events_match, no_ties, soft_err

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent

OPV_TX_TABLE_FRAMES = 4096   # frames the build-time NCO checkpoint table covers (csrc/opv_tx_internal.h: OPV_TX_CKPT_FRAMES)


@pytest.mark.parametrize("streaming", [True, False])
def test_config1_loopback(amd, oracle, golden, iq10, streaming):
    """BASELINE config 0: opv-mod -S W5NYV -B 10 | opv-demod [-s]"""
    arrays, meta = golden
    d = amd.Demod(1, max_samples=iq10.size // 2 + 64, streaming=streaming)
    got = d.receive([iq10])[0]
    exp = oracle.receive(iq10, streaming=streaming)
    check_stream(amd, got, exp, f"c1 streaming={streaming}")
    mode = "stream" if streaming else "batch"
    assert np.array_equal(got["frames"], arrays[f"c1_{mode}_frames"])           # reference-made fixture
    assert amd.format_events(got["events"]) == meta[f"c1_{mode}"]["events"]
    a, _ = soft_err(got["soft"], arrays[f"c1_{mode}_soft"])
    assert a < SOFT_TIGHT
    d.close()


def test_initial_offset_flag(amd, oracle, iq10):
    d = amd.Demod(1, max_samples=iq10.size // 2 + 64, streaming=True, init_offset=1000.0)
    got = d.receive([iq10])[0]
    check_stream(amd, got, oracle.receive(iq10, streaming=True, init_offset=1000.0), "-o 1000")
    d.close()


@pytest.mark.parametrize("off,alpha", EXTREME_FLAGS)
def test_extreme_flag_values(amd, oracle, iq10, off, alpha):
    """-o beyond the AFC clamp (the reference takes any value for the symbols before the first AFC update,
    :1004-1005 / :302-303) and -a so large that the loop slams into its clamp every symbol."""
    x = extreme_flags_capture(iq10)
    for frontend in (1, 4, 16):
        d = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=True, init_offset=off, afc_alpha=alpha)
        d.set_frontend(frontend)
        got = d.receive([x])[0]
        check_stream(amd, got, oracle.receive(x, streaming=True, init_offset=off, afc_alpha=alpha), f"-o {off} -a {alpha} x{frontend}")
        d.close()


@pytest.mark.parametrize("ppm", [-25000.0, -3000.0, 3000.0, 25000.0])
def test_timing_loop_slipping(amd, oracle, iq10, ppm):
    """Sample-clock errors far beyond what the timing loop can follow (0.3 % and 2.5 %): it slips a symbol
    every few hundred / few dozen symbols and the TED output is large all the time; all three mappings (one, four and
    sixteen streams per wave), -s and batch."""
    x = impair(resample_clock(iq10, ppm), amp=5000.0, f0_hz=-300.0, ebn0_db=20.0, seed=9)
    exp_s, exp_b = oracle.receive(x, streaming=True), oracle.receive(x, streaming=False)
    for frontend in (1, 4, 16):
        for streaming, exp in ((True, exp_s), (False, exp_b)):
            d = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=streaming)
            d.set_frontend(frontend)
            check_stream(amd, d.receive([x])[0], exp, f"ppm {ppm} x{frontend} streaming={streaming}")
            d.close()


def test_afc_alpha_flag(amd, oracle, iq10):
    d = amd.Demod(1, max_samples=iq10.size // 2 + 64, streaming=True, afc_alpha=AFC_ALPHA_FLAG)
    got = d.receive([iq10])[0]
    check_stream(amd, got, oracle.receive(iq10, streaming=True, afc_alpha=AFC_ALPHA_FLAG), "-a 0.01")
    d.close()


def test_set_frontend_accepts_the_documented_mappings_only(amd):
    """opv_set_frontend: 0 (automatic), 1, 4, 16 (include/opv_demod.h); anything else is OPV_EINVAL with a message."""
    d = amd.Demod(1, max_samples=1 << 16, streaming=True)
    for ok in (0, 1, 4, 16, 0):
        d.set_frontend(ok)
    for bad in (2, 3, -1, -2, -3, 8, 64):
        with pytest.raises(amd.OpvError, match="opv_set_frontend"):
            d.set_frontend(bad)
    d.close()


def test_offset_search_energies(amd, oracle, iq10):
    d = amd.Demod(1, max_samples=iq10.size // 2 + 64, streaming=True)
    d.receive([iq10])
    off, e = oracle.estimate_offset(iq10[: 2 * 86720], energies=True)
    g = d.offset_energies(0)
    assert d.state(0).est_offset_hz == off == 1430.0
    rel = np.max(np.abs(g - e) / e)
    print("offset-search energy max rel err", rel)
    assert rel < 1e-12          # margins between candidates are >= 1e-8; the reference's own phase
                                # accumulation is ~1e-13 from exact arithmetic
    assert int(np.argmax(g[:121])) == int(np.argmax(e[:121]))
    d.close()


def test_offset_search_near_tie_guard(amd, oracle, iq10):
    """Constructed ties. For a REAL-valued capture (Q = 0) the search landscape is exactly symmetric, E(-o) = E(+o),
    so unless the peak sits at o = 0 the two best coarse candidates tie in exact arithmetic and the reference's
    winner (first maximum, strict '>') is decided by the rounding of its own 40 000-sample phase accumulation. The
    one-pass evaluation (agreement ~1e-13) cannot call that; its near-tie guard must notice (offset_ties >= 2)
    and re-evaluate the contenders in the reference's order of operations - and then return the oracle's estimate."""
    caps = near_tie_captures(iq10)             # (tests/hostile_inputs.py: four real tones, one with noise, real noise, two controls)
    d = amd.Demod(len(caps), max_samples=86720 + 64, streaming=True)
    got = d.receive(caps)
    n_guarded = 0
    for k, x in enumerate(caps):
        off, e = oracle.estimate_offset(x, energies=True)
        st = got[k]["state"]
        g = d.offset_energies(k)
        rel = np.max(np.abs(g - e) / np.maximum(e, 1e-300))
        print(f"capture {k}: oracle {off} Hz, product {st.est_offset_hz} Hz, offset_ties {st.offset_ties}, energies max rel {rel:.2e}")
        assert st.est_offset_hz == off, k
        assert rel < 1e-11, k
        n_guarded += st.offset_ties >= 2
        if d.offset_ties_on_host():           # what the host re-evaluated IS the reference's number (same loop, same libm)
            assert int(np.sum(g == e)) >= st.offset_ties - 1, (k, int(np.sum(g == e)), st.offset_ties)
    assert n_guarded >= 4, n_guarded           # the symmetric landscapes must have been noticed
    assert d.offset_ties_on_host()             # this image's glibc reproduces the pinned energy (csrc/opv_offset_host.cpp)
    d.close()
    # and on an ordinary capture the guard stays out of the way
    d = amd.Demod(1, max_samples=iq10.size // 2 + 64, streaming=True)
    d.receive([iq10])
    assert d.state(0).offset_ties == 0
    d.close()


@pytest.mark.parametrize("host", [True, False])
def test_offset_search_ties_decided_like_the_reference(amd, host, monkeypatch):
    """208 captures with an exactly symmetric search landscape (real-valued or purely imaginary samples: tones near and far from
    the tone pair, noise, single branches of MSK captures; soak_inputs.symmetric_openings) in one batch-mode context: mirrored
    candidates tie - exactly, in the reference (bit-identical energies for -o and +o: its strict '>', src/opv-demod.cpp:161,195,
    keeps the first), within 1e-13 in either order in the one-pass evaluation. The guard must notice and re-evaluate; with the
    tie decided on the host (the reference's loop on the reference's libm, csrc/opv_offset_host.cpp) the estimate equals the oracle's
    for every capture and every re-evaluated energy IS the oracle's, bit for bit. host=False (OPV_OFFSET_DISTRUST_LIBM: the
    device's sincos re-evaluates, the fallback for a host with another libm) must give the same estimates here - an exact
    mirror tie survives any sin / cos that is odd / even in its argument - but not the same last bits of the energies."""
    from concurrent.futures import ProcessPoolExecutor
    from soak_inputs import host_workers, oracle_offset_energies_chunk, symmetric_openings
    S = 208
    caps = symmetric_openings(int(os.environ.get("OPV_FUZZ_BASE", "20261003")) % 1000 + 23, S)
    if not host:
        monkeypatch.setenv("OPV_OFFSET_DISTRUST_LIBM", "1")
    d = amd.Demod(S, max_samples=46000, streaming=False)
    assert d.offset_ties_on_host() == host
    d.receive(caps)
    got = [d.state(k) for k in range(S)]
    taps = [d.offset_energies(k) for k in range(S)]
    d.close()
    W = host_workers()
    with ProcessPoolExecutor(W) as ex:
        res = list(ex.map(oracle_offset_energies_chunk, [caps[i::W] for i in range(W)]))
    exp = [None] * S
    for i, part in enumerate(res):
        exp[i::W] = part
    guarded = wrong = 0
    for k in range(S):
        off, e = exp[k]
        guarded += got[k].offset_ties >= 2
        if got[k].est_offset_hz != off:
            wrong += 1
        if host and got[k].offset_ties:
            assert int(np.sum(taps[k] == e)) >= got[k].offset_ties - 1, (k, got[k].offset_ties)
        assert np.max(np.abs(taps[k] - e) / np.maximum(e, 1e-300)) < 1e-11, k
    print(f"symmetric captures: {guarded} of {S} guarded, host={host}: {wrong} estimates differ from the oracle's")
    assert guarded >= S // 3 and wrong == 0, (guarded, wrong)


# (seed, k) of soak_inputs.offset_opening on which estimate_offset meets a NEAR tie - a contender within 1e-11 of the best energy in play
# and not equal to it: found by scripts/experiments/near_tie_hunt.py (CPU, the oracle) among openings (100..259) x 256: 19 of 40 960
NEAR_TIE_OPENINGS = [(100, 190), (103, 114), (108, 204), (108, 249), (114, 215), (124, 177), (147, 223), (151, 107), (156, 46), (179, 187), (189, 248), (191, 84), (202, 29), (206, 165), (214, 253), (240, 150), (243, 11), (249, 7), (255, 177)]


@pytest.mark.parametrize("host", [True, False])
def test_offset_search_near_ties_on_ordinary_captures(amd, oracle, host, monkeypatch):
    """The inputs the host-side tie decision exists for: ORDINARY noisy openings (random start, level, carrier offset, 3 - 22 dB) on
    which two candidates of estimate_offset (ref src/opv-demod.cpp:131-202) differ by less than 1e-11 relative without being
    equal - one opening in about two thousand; these 19 were found with the oracle - so that the strict '>' (:161,195) hangs on
    the last places of sin / cos. The guard must fire on every one of them and the estimate must equal the oracle's on all. The
    contenders are re-evaluated in the reference's order on the device first; only those that remain within 2e-13 of each other
    (what sin / cos could still move, k_offset_search.hip: kHostRel) go to the host's libm - here the finds are 1e-12 ... 1e-11
    apart, so the device decides them, and host=False (no host at all: the fallback) must agree.
    37 ordinary openings that are no near ties ride along: estimate equal, guard silent."""
    from soak_inputs import near_tie_class, offset_opening
    if not host:
        monkeypatch.setenv("OPV_OFFSET_DISTRUST_LIBM", "1")
    ids = list(NEAR_TIE_OPENINGS) + [(7, k) for k in range(37)]
    caps = [offset_opening(s, k) for s, k in ids]
    d = amd.Demod(len(caps), max_samples=46000, streaming=False)
    assert d.offset_ties_on_host() == host
    d.receive(caps)
    differ = fired = 0
    worst_reeval = 0.0
    for i, x in enumerate(caps):
        off, e = oracle.estimate_offset(x, energies=True)
        st, g = d.state(i), d.offset_energies(i)
        tie = i < len(NEAR_TIE_OPENINGS)
        assert bool(near_tie_class(e)) == tie, ids[i]            # the find reproduces from (seed, k)
        assert np.max(np.abs(g - e) / np.maximum(e, 1e-300)) < 1e-11, ids[i]
        if tie:
            fired += st.offset_ties >= 2                             # (a find within 1e-13 of the 1e-11 band's edge may sit outside the device's band)
            # the premise of the second level (k_offset_search.hip: kHostRel = 2e-13): an energy re-evaluated on the device in the
            # reference's order differs from the reference's only by what sin / cos differ - far below that band. The
            # st.offset_ties entries of the tap that agree best with the oracle ARE the re-evaluated ones.
            rel = np.sort(np.abs(g - e) / np.maximum(e, 1e-300))[: max(int(st.offset_ties) - 1, 1)]
            worst_reeval = max(worst_reeval, float(rel.max()))
        else:
            assert st.offset_ties == 0 and st.est_offset_hz == off, ids[i]
        assert st.est_offset_hz == off, (ids[i], st.est_offset_hz, off, host)
        differ += st.est_offset_hz != off
    print(f"near-tie openings: guard fired on {fired} of {len(NEAR_TIE_OPENINGS)}; host={host}: {differ} estimates differ from the oracle's; "
          f"re-evaluated energies agree with the oracle's to {worst_reeval:.1e} relative")
    assert worst_reeval < 2e-14, worst_reeval                    # a tenth of kHostRel
    assert fired >= len(NEAR_TIE_OPENINGS) - 2, fired
    d.close()


@pytest.mark.parametrize("host", [True, False])
def test_offset_search_on_weakly_correlated_inputs(amd, host, monkeypatch):
    """96 captures whose correlation with the tone pair is weak against their power (soak_inputs.weak_correlation_openings:
    out-of-band tones with noise, a strong interferer over a faint signal, a few LSB of noise on a DC offset, real tones with one
    LSB of noise on the other branch). An energy of the search carries an error ~ eps sqrt(energy x 40 x power), which on such
    inputs is orders of magnitude above eps x energy: both near-tie bands of k_offset_search.hip are scaled accordingly, so
    that a pair of candidates the last places of the arithmetic (first band) or of sin / cos (second band) could reorder is
    still re-evaluated / handed to the host. Every estimate equals the oracle's; the energies agree on that same scale."""
    from concurrent.futures import ProcessPoolExecutor
    from soak_inputs import host_workers, oracle_offset_energies_chunk, weak_correlation_openings
    S = 96
    caps = weak_correlation_openings(int(os.environ.get("OPV_FUZZ_BASE", "20261003")) % 1000 + 61, S)
    if not host:
        monkeypatch.setenv("OPV_OFFSET_DISTRUST_LIBM", "1")
    d = amd.Demod(S, max_samples=46000, streaming=False)
    assert d.offset_ties_on_host() == host
    d.receive(caps)
    got = [d.state(k) for k in range(S)]
    taps = [d.offset_energies(k) for k in range(S)]
    decided = d.offset_ties_decided_on_host()
    d.close()
    W = host_workers()
    with ProcessPoolExecutor(W) as ex:
        res = list(ex.map(oracle_offset_energies_chunk, [caps[i::W] for i in range(W)]))
    exp = [None] * S
    for i, part in enumerate(res):
        exp[i::W] = part
    guarded = wrong = 0
    weakest, worst = 1.0, 0.0
    for k in range(S):
        off, e = exp[k]
        x = caps[k][: 2 * 40 * (min(caps[k].size // 2, 40000) // 40)].astype(np.float64)
        power = float(np.sum(x * x))
        weakest = min(weakest, float(e.max() / (40.0 * power)))
        worst = max(worst, float(np.max(np.abs(taps[k] - e) / np.sqrt(40.0 * power * np.maximum(e, 1e-300)))))
        guarded += got[k].offset_ties >= 2
        wrong += got[k].est_offset_hz != off
    print(f"weakly correlated captures: energy / (40 x power) down to {weakest:.1e}; {guarded} of {S} guarded, {decided} decided by the host "
          f"(host={host}); energies agree to {worst:.1e} of sqrt(40 x power x energy); {wrong} estimates differ from the oracle's")
    assert worst < 1e-11 and wrong == 0, (worst, wrong)
    assert (decided > 0) == host or decided == 0


def test_process_returns_without_waiting_in_a_search_round(amd, oracle, iq10):
    """opv_process is asynchronous in EVERY round (include/opv_demod.h, ABI 7). The round in which offset searches run is the
    one that had a host wait inside until round 5: a tie in the last places of sin / cos is decided with the HOST's libm, and the
    caller used to wait for the search kernel and the decision. Now kernels stage the tied streams' inputs in pinned memory, a
    host function enqueued on the context's stream (hipLaunchHostFunc) decides them, and a kernel carries the results back -
    all behind the search and in front of the front-end, none of it on the caller's thread.
    2048 streams in one context, three of them constructed ties (real-valued captures: the mirrored candidates tie exactly), every
    search in the same round: the opv_process CALL returns in under 0.5 ms (the search kernel alone runs longer), the ties are
    decided by the host (the counter says so) like the reference decides them, and an ordinary stream is untouched."""
    import time
    import torch
    dev = torch.device("cuda", 0)
    S, n = 2048, 86720
    t = np.arange(n)
    ties = []
    for f_hz, amp, ph in ((33550.0, 9000.0, 0.3), (36000.0, 20000.0, 1.1), (47000.0, 12000.0, 2.0)):
        x = np.zeros(2 * n, np.int16)
        x[0::2] = np.rint(amp * np.cos(2 * np.pi * f_hz * t / 2168000.0 + ph))
        ties.append(x)
    plain = np.ascontiguousarray(iq10[: 2 * n])
    d_ties = [torch.from_numpy(x).to(dev) for x in ties]
    d_plain = torch.from_numpy(plain).to(dev)
    where = {3: 0, 700: 1, 2047: 2}
    d = amd.Demod(S, max_samples=n + 64, streaming=True)
    assert d.offset_ties_on_host()
    took = []
    for rnd in range(5):                          # the first round also loads the code objects; the later ones are the measurement (their minimum)
        if rnd:
            d.reset(-1)
        for k in range(S):
            d.attach(k, (d_ties[where[k]] if k in where else d_plain).data_ptr(), n, eof=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        d.process()
        took.append(time.perf_counter() - t0)
        d.sync()
        assert d.offset_ties_decided_on_host() == 3 * (rnd + 1) and d.offset_ties_left_to_device() == 0
    d.enable_timing(True)
    d.reset(-1)
    for k in range(S):
        d.attach(k, (d_ties[where[k]] if k in where else d_plain).data_ptr(), n, eof=True)
    d.process()
    ms = d.kernel_times()
    print(f"opv_process call in a search round, 2048 streams, 3 host-decided ties: {[f'{1e3 * v:.3f} ms' for v in took]}; "
          f"on the stream: search {ms['offset_search']:.3f} ms, front-end {ms['msk_frontend']:.3f} ms")
    assert min(took[1:]) < 0.5e-3, took
    assert 1e3 * min(took[1:]) < 0.5 * ms["offset_search"], (took, ms)       # the call does not contain the search kernel, let alone the decision
    for k, i in where.items():
        off, e = oracle.estimate_offset(ties[i], energies=True)
        st, g = d.state(k), d.offset_energies(k)
        assert st.est_offset_hz == off and st.offset_ties >= 2, (k, st.est_offset_hz, off, st.offset_ties)
        assert int(np.sum(g == e)) >= st.offset_ties - 1, k          # what the host re-evaluated IS the reference's number
    off, _ = oracle.estimate_offset(plain, energies=True)
    for k in (0, 4, 699, 701, 2046):
        assert d.state(k).est_offset_hz == off and d.state(k).offset_ties == 0, k
    d.close()


def test_tie_decision_in_stream_order_under_concurrency_async_push_and_early_destroy(amd, oracle, iq10):
    """What the stream-ordered host decision (hipLaunchHostFunc between k_offset_search and the front-end) must survive besides
    the plain case: (a) FOUR host threads, a context each, whose searches tie in the same moments - the host functions of four
    HIP streams run on the runtime's threads at once, each spreading its slots over worker threads; (b) the tied captures
    arriving through opv_push_iq_batch_async from pinned host memory with opv_process called BEFORE opv_push_wait - search,
    staging kernel and host function all queue behind the move on the device; (c) opv_reset_stream and opv_destroy called right
    behind opv_process, while the passes are still in flight (both drain the stream first). Estimates, energies and tie counts
    equal the oracle's / the reference's first maximum everywhere."""
    import threading
    import torch
    n = 86720
    t = np.arange(n)
    ties = []
    for f_hz, amp, ph in ((33550.0, 9000.0, 0.3), (41000.0, 15000.0, 0.9), (52000.0, 4000.0, 2.2)):
        x = np.zeros(2 * n, np.int16)
        x[0::2] = np.rint(amp * np.cos(2 * np.pi * f_hz * t / 2168000.0 + ph))
        ties.append(x)
    plain = np.ascontiguousarray(iq10[: 2 * n])
    caps = [ties[0], plain, ties[1], plain, ties[2], plain]
    exp = [oracle.estimate_offset(x, energies=True) for x in (ties[0], plain, ties[1], ties[2])]
    exp = {0: exp[0], 1: exp[1], 2: exp[2], 3: exp[1], 4: exp[3], 5: exp[1]}
    pinned = []
    for x in caps:
        buf = torch.empty(x.size, dtype=torch.int16).pin_memory()
        buf.numpy()[:] = x
        pinned.append(buf)
    out = [None] * 4

    def work(k):
        try:
            res = []
            for rep in range(4):
                d = amd.Demod(len(caps), max_samples=n + 64, streaming=True)
                assert d.offset_ties_on_host()
                if rep % 2:                                           # (b) the first chunk arrives asynchronously from pinned memory
                    d.push_batch(range(len(caps)), [b.numpy() for b in pinned], wait=False)
                    d.process()
                    d.push_wait()
                else:
                    for j, x in enumerate(caps):
                        d.push(j, x)
                    d.process()
                if rep == 3:                                          # (c) destroy right behind the round: nothing may be left running
                    d.close()
                    continue
                if rep == 2:                                          # (c) reset right behind the round, then the same round again
                    d.reset(-1)
                    for j, x in enumerate(caps):
                        d.push(j, x)
                    d.process()
                d.sync()
                res.append(([d.state(j).est_offset_hz for j in range(len(caps))], [d.state(j).offset_ties for j in range(len(caps))],
                            [d.offset_energies(j) for j in range(len(caps))], d.offset_ties_decided_on_host(), d.offset_ties_left_to_device()))
                d.close()
            out[k] = res
        except Exception as e:           # surfaces in the main thread below
            out[k] = e

    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for x in th:
        x.start()
    for x in th:
        x.join()
    for k in range(4):
        assert not isinstance(out[k], Exception), out[k]
        assert len(out[k]) == 3
        for rep, (est, nt, taps, decided, left) in enumerate(out[k]):
            assert left == 0 and decided == (6 if rep == 2 else 3), (k, rep, decided, left)     # (rep 2 ran the round twice)
            for j in range(len(caps)):
                off, e = exp[j]
                assert est[j] == off, (k, rep, j, est[j], off)
                if j % 2 == 0:
                    assert nt[j] >= 2 and int(np.sum(taps[j] == e)) >= nt[j] - 1, (k, rep, j, nt[j])
                else:
                    assert nt[j] == 0, (k, rep, j)


def test_more_ties_in_one_round_than_the_host_passes_stage(amd, oracle):
    """A round stages at most 8 passes x 512 streams = 4096 tied streams for the host (csrc/opv_device.h); a context whose inputs
    tie SYSTEMATICALLY - real-valued captures on every stream, the mirrored candidates tie exactly - can list more. 4200 streams
    of one short real-valued capture in one batch-mode round: 4096 are decided by the host, 104 keep the device's decision and
    are counted, and (an exact mirror tie survives any odd / even sin / cos) every estimate equals the oracle's either way."""
    import torch
    S, n = 4200, 4000
    x = staged_ties_capture(n)
    off, e = oracle.estimate_offset(x, energies=True)
    assert off in (-1530.0, 1530.0)                                  # (a convex, exactly symmetric landscape: the edges tie)
    d_x = torch.from_numpy(x).to("cuda")
    d = amd.Demod(S, max_samples=n + 64, streaming=False)
    assert d.offset_ties_on_host()
    for k in range(S):
        d.attach(k, d_x.data_ptr(), n, eof=True)
    d.process()
    d.sync()
    assert d.offset_ties_decided_on_host() == 4096 and d.offset_ties_left_to_device() == S - 4096
    est = np.array([d.state(k).est_offset_hz for k in range(S)])
    ties = np.array([d.state(k).offset_ties for k in range(S)])
    assert np.all(est == off) and np.all(ties >= 2), (np.unique(est), ties.min())
    d.close()


@pytest.mark.parametrize("tag", ["clean", "p700_16dB_pll20"])
def test_coherent_prefix_parity(amd, iq10, tag):
    """`-c`: csrc/k_coherent.hip against the reference-made fixtures tests/golden/coherent.*.
    The reference's Costas loop is chaotic (1e-15 rad -> O(1) within ~12 000 symbols), so the bar is PREFIX parity:
    same offset estimate, same symbol count, soft symbols within 1e-9 of the reference's for the first 2000 symbols;
    where the trajectories part later is reported, not asserted."""
    import json
    g = ROOT / "tests" / "golden"
    meta = json.loads((g / "coherent.json").read_text())[tag]
    ref_soft = np.load(g / "coherent.npz")[tag + "_soft"]
    x = iq10 if tag == "clean" else impair(iq10, 2000.0, 700.0, 16.0, seed=11)
    assert hashlib.sha256(x.tobytes()).hexdigest() == meta["iq_sha256"]
    d = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=False, coherent=True, pll_bw=meta["pll_bw"])
    got = d.receive([x])[0]
    d.close()
    assert got["state"].est_offset_hz == meta["est_offset"]
    assert got["state"].total_symbols == len(ref_soft) == len(got["soft"])
    e = np.abs(got["soft"] - ref_soft) / np.mean(np.abs(ref_soft))
    part = np.nonzero(e > 1e-6)[0]
    print(f"-c {tag}: max err over the first 2000 symbols {e[:2000].max():.2e}; over 1e-6 from symbol "
          f"{int(part[0]) if part.size else None} of {len(e)}; frames {len(got['frames'])} (reference {meta['n_frames']})")
    assert e[:2000].max() < 1e-9


def test_frame_decoder_taps_exact(amd, oracle, golden):
    """FrameDecoder::decode in isolation on reference-made payloads: everything bit-exact."""
    arrays, _ = golden
    d = amd.Demod(1, max_samples=1 << 20)
    r = d.decode_payloads(arrays["taps_payload_soft"], taps=True)
    assert np.array_equal(r["frames"], arrays["taps_frames"])
    assert np.array_equal(r["metrics"], arrays["taps_metric"])
    assert np.array_equal(r["deint"], arrays["taps_deint"])
    assert np.array_equal(r["bits"], arrays["taps_bits"])
    d.close()


def test_frame_decoder_random_payloads_exact(amd, oracle):
    """Noise-like payloads (every quantiser level, ties in the trellis, non-zero metrics)."""
    rng = np.random.default_rng(11)
    n = 64
    soft = rng.standard_normal((n, CODED_BITS)) * 3e10
    soft[1] *= 1e-9
    soft[2] = 0.0                      # silent frame -> dropped (-1)
    soft[3] = np.round(soft[3] / 1e10) * 1e10   # many exact ties
    soft[4, ::2] = 0.0
    d = amd.Demod(1, max_samples=1 << 20)
    r = d.decode_payloads(soft, taps=True)
    for k in range(n):
        e = oracle.frame_decode(soft[k])
        assert r["metrics"][k] == e["metric"], k
        if e["metric"] < 0:
            continue
        assert np.array_equal(r["q"][k], e["q"]), k
        assert np.array_equal(r["deint"][k], e["deint"]), k
        assert np.array_equal(r["bits"][k], e["bits"]), k
        assert np.array_equal(r["frames"][k], e["frame"]), k
    d.close()


@pytest.mark.parametrize("tag", ["p2000_12dB", "m2000_6dB", "p700_16dB", "p2000_clean"])
def test_noisy_configs_vs_reference_fixtures(amd, golden, iq100, tag):
    """BASELINE config 2 family (offset + AWGN), 100 frames, against reference-made fixtures."""
    arrays, meta = golden
    m = meta["noisy_100"][tag]
    x = impair(iq100, **m["recipe"])
    assert hashlib.sha256(x.tobytes()).hexdigest() == m["input_sha256"]
    d = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=True)
    got = d.receive([x])[0]
    assert len(got["frames"]) == m["n_frames"]
    assert np.array_equal(got["frames"], arrays[f"n_{tag}_frames"])
    assert np.array_equal(got["meta"]["viterbi_metric"], arrays[f"n_{tag}_metrics"])
    assert np.array_equal(got["meta"]["release_symbol"], arrays[f"n_{tag}_frame_sym"])
    ev = "\n".join(amd.format_events(got["events"]))
    assert hashlib.sha256(ev.encode()).hexdigest() == m["events_sha256"]
    a, r = soft_err(got["soft"][::97], arrays[f"n_{tag}_soft_strided"])
    print(tag, "soft err", a, r)
    assert a < SOFT_TIGHT and r < SOFT_RTOL
    assert got["state"].est_offset_hz == m["est_offset"]
    d.close()


def test_many_streams_one_context(amd, oracle, iq10):
    """BASELINE config 3 shape (batched independent streams), small: 9 streams, mixed channels."""
    caps = [iq10]
    for k in range(8):
        caps.append(impair(iq10, amp=1500.0 + 900 * k, f0_hz=-2000 + 500.0 * k, ebn0_db=14.0 + k, seed=k))
    d = amd.Demod(len(caps), max_samples=iq10.size // 2 + 64, streaming=True)
    got = d.receive(caps)
    for k, x in enumerate(caps):
        check_stream(amd, got[k], oracle.receive(x, streaming=True), f"stream {k}")
    d.close()


def test_incremental_push_equals_one_shot(amd, oracle, iq10):
    """opv-modem feeds the demodulator in 16 KB reads (reference src/opv-modem.cpp:734,753)."""
    d = amd.Demod(1, max_samples=iq10.size // 2 + 64, streaming=True)
    step = 2 * 4096
    frames = []
    for o in range(0, iq10.size, step):
        d.push(0, iq10[o:o + step])
        d.process()
        f, _ = d.pop_frames(0)
        frames.append(f)
    d.flush(0)
    d.process()
    f, _ = d.pop_frames(0)
    frames.append(f)
    frames = np.concatenate(frames)
    exp = oracle.receive(iq10, streaming=True)
    assert np.array_equal(frames, exp["frames"])
    a, _ = soft_err(d.soft(0), exp["soft"])
    assert a < SOFT_TIGHT
    events_match(amd, d.pop_events(0), exp["events"])
    d.close()


def test_short_and_ragged_inputs(amd, oracle, iq10):
    for n in (0, 1, 49, 51, 4000, 86719, 86720, 86721, 100000):
        d = amd.Demod(1, max_samples=200000, streaming=True)
        got = d.receive([iq10[: 2 * n]])[0]
        exp = oracle.receive(iq10[: 2 * n], streaming=True)
        assert got["state"].total_symbols == exp["n_soft"], n
        assert np.array_equal(got["frames"], exp["frames"]), n
        assert len(exp["frames"]) == (1 if n >= 100000 else 0)
        assert len(got["chunks"]) == len(exp["chunks"]), n
        if exp["n_soft"]:
            a, _ = soft_err(got["soft"], exp["soft"])
            assert a < SOFT_TIGHT, n
        d.close()
    d = amd.Demod(1, max_samples=200000, streaming=False)
    got = d.receive([iq10[: 2 * 30]])[0]
    assert got["state"].total_symbols == 0 and got["state"].est_offset_hz == 0.0
    d.close()


def test_every_tail_length_uses_its_last_samples(amd, oracle, iq10):
    """45 consecutive capture lengths (all residues mod 4 and mod 40): for some of them the last
    symbol's late gate interpolates on the capture's very last sample, which sits in an incomplete
    16-byte piece of the last LDS tile (k_frontend copies that piece sample by sample and never reads
    past n_avail). Batch and streaming."""
    for streaming in (True, False):
        for n in range(91003, 91048):
            d = amd.Demod(1, max_samples=100000, streaming=streaming)
            got = d.receive([iq10[: 2 * n]])[0]
            d.close()
            exp = oracle.receive(iq10[: 2 * n], streaming=streaming)
            assert got["state"].total_symbols == exp["n_soft"], (streaming, n)
            a, _ = soft_err(got["soft"], exp["soft"])
            assert a < SOFT_TIGHT, (streaming, n, a)
            assert np.allclose(got["chunks"], exp["chunks"], rtol=0, atol=1e-9), (streaming, n)


def test_errors_are_loud(amd):
    with pytest.raises(amd.OpvError):
        amd.Demod(0)
    d = amd.Demod(1, max_samples=1000)
    with pytest.raises(amd.OpvError):
        d.push(0, np.zeros(2 * 2000, np.int16))     # capacity
    d.flush(0)
    with pytest.raises(amd.OpvError):
        d.push(0, np.zeros(20, np.int16))           # push after flush
    d.close()


def test_api_misuse_returns_errors_and_leaves_the_context_usable(amd):
    """Null pointers, stream indices out of range, absurd sizes, unaligned device pointers, missing communicators through
    every entry point of include/opv_demod.h that takes a context: a negative code (or 0 for the documented no-ops: empty
    pushes, empty pops), never a crash, and the context still processes afterwards."""
    import ctypes as C
    L = amd.lib()
    ctx = C.c_void_p()
    cfg = amd.Cfg()
    cfg.streaming, cfg.afc_alpha, cfg.max_samples, cfg.device = 1, 0.001, 100000, 0
    for args in ((None, 1, C.byref(cfg)), (C.byref(ctx), 1, None), (C.byref(ctx), 0, C.byref(cfg)), (C.byref(ctx), -5, C.byref(cfg))):
        assert L.opv_create(*args) < 0
    far = amd.Cfg()
    far.streaming, far.afc_alpha, far.max_samples, far.device = 1, 0.001, 100000, 99
    assert L.opv_create(C.byref(ctx), 1, C.byref(far)) == -2                       # OPV_ENODEV
    for field, val in (("init_offset_hz", float("inf")), ("init_offset_hz", float("nan")), ("afc_alpha", float("-inf")), ("pll_bw_hz", float("inf"))):
        inf = amd.Cfg()                                                            # (the reference spins forever in its phase wraps on these)
        inf.streaming, inf.afc_alpha, inf.max_samples, inf.device, inf.have_init_offset, inf.coherent = field != "pll_bw_hz", 0.001, 100000, 0, 1, 1
        setattr(inf, field, val)
        assert L.opv_create(C.byref(ctx), 1, C.byref(inf)) == -1, field           # OPV_EINVAL
    assert L.opv_create(C.byref(ctx), 3, C.byref(cfg)) == 0
    iq = np.zeros(2000, np.int16)
    p = iq.ctypes.data
    bad = [("opv_push_iq", (None, 0, p, 10)), ("opv_push_iq", (ctx, 7, p, 10)), ("opv_push_iq", (ctx, -1, p, 10)), ("opv_push_iq", (ctx, 0, None, 10)),
           ("opv_push_iq", (ctx, 0, p, 10 ** 9)), ("opv_push_iq_batch", (ctx, -1, None, None, None)), ("opv_push_iq_batch", (ctx, 2, None, None, None)),
           ("opv_flush", (ctx, 9)), ("opv_flush", (None, 0)), ("opv_attach_device_iq", (ctx, 0, C.c_void_p(3), 100, 1)),
           ("opv_attach_device_iq", (ctx, 0, None, 100, 1)), ("opv_process", (None,)), ("opv_sync", (None,)), ("opv_set_frontend", (ctx, 3)),
           ("opv_set_frontend", (None, 1)), ("opv_reset_stream", (ctx, 5)), ("opv_pop_frames", (ctx, 9, p, 1, None)), ("opv_get_state", (ctx, 0, None)),
           ("opv_get_state", (ctx, 4, p)), ("opv_tap_offset_energies", (ctx, 0, None)), ("opv_tap_wave_info", (ctx, 8, p)), ("opv_tap_occupancy", (ctx, None)),
           ("opv_decode_payloads", (ctx, None, 3, p, p, None, None, None)), ("opv_channel_device", (ctx, None, None, 16, C.c_double(1), C.c_double(0), C.c_double(0), 1)),
           ("opv_channel_device", (ctx, C.c_void_p(16), C.c_void_p(32), 3, C.c_double(1), C.c_double(0), C.c_double(0), 1)),
           ("opv_resample_device", (ctx, None, 10, None, 10, C.c_double(0))), ("opv_tx_modulate_device", (ctx, None, 3, None)),
           ("opv_tx_modulate_device", (ctx, p, 1, C.c_void_p(4))), ("opv_tx_modulate_device_to_host", (ctx, None, 0, None)),
           ("opv_gather_frames", (ctx, None, 0, None, None)), ("opv_gather_frames", (None, None, 0, None, None)), ("opv_gather_frames_all", (None, None, 0, 0, None, None)),
           ("opv_comm_init", (None, 1, 0, None, 0)), ("opv_comm_init_all", (None, 0, None)), ("opv_comm_unique_id", (None,)), ("opv_kernel_times", (ctx, None)),
           ("opv_enable_timing", (None, 1)),
           ("opv_tap_push_soft", (None, 0, p, 10)), ("opv_tap_push_soft", (ctx, 7, p, 10)), ("opv_tap_push_soft", (ctx, -1, p, 10)),
           ("opv_tap_push_soft", (ctx, 0, None, 10)), ("opv_tap_push_soft", (ctx, 0, p, 0)), ("opv_tap_push_soft", (ctx, 0, p, 10 ** 9))]
    noop = [("opv_push_iq", (ctx, 0, p, 0)), ("opv_push_iq", (ctx, 0, None, 0)), ("opv_push_iq_batch", (ctx, 0, None, None, None)),
            ("opv_pop_frames", (ctx, 0, None, 10, None)), ("opv_pop_frames", (ctx, 0, p, 0, None)), ("opv_pop_events", (ctx, 0, None, 5)),
            ("opv_tap_soft", (ctx, 0, 0, None, 10)), ("opv_decode_payloads", (ctx, p, 0, p, p, None, None, None))]
    for group, want_error in ((bad, True), (noop, False)):
        for name, args in group:
            f = getattr(L, name)
            saved, f.argtypes = f.argtypes, None
            saved_res, f.restype = f.restype, C.c_int
            try:
                r = f(*[C.c_uint64(a) if isinstance(a, int) and a >= 2 ** 31 else a for a in args])
            finally:
                f.argtypes, f.restype = saved, saved_res
            assert (r < 0) if want_error else (r == 0), (name, args, r)
    assert L.opv_push_iq(ctx, 0, p, 100) == 0 and L.opv_process(ctx) == 0 and L.opv_sync(ctx) == 0
    L.opv_destroy(ctx)
    L.opv_destroy(None)


# ------------------------------------------------------------------ full-size cases
def test_config1_full_size_vs_reference_hashes(amd, golden):
    """BASELINE configs[1] at full size: 1000 clean frames, one stream. The input is the product's
    own modulator (sha256-pinned to `opv-mod -S W5NYV -B 1000`); the decoded bytes and the tracker
    event text must hash to what the REFERENCE BINARY produced (tests/golden/golden.json)."""
    _, meta = golden
    pins = meta["opv_mod_bert_W5NYV"]
    tx = amd.bert_frames(1000)
    iq = amd.modulate(tx)
    assert hashlib.sha256(iq.tobytes()).hexdigest() == pins["1000"]["sha256"]
    d = amd.Demod(1, max_samples=iq.size // 2 + 64, streaming=True)
    d.push(0, iq)
    d.flush(0)
    d.process()
    fr, meta_f = d.pop_frames(0)
    assert hashlib.sha256(fr.tobytes()).hexdigest() == pins["1000_frames_stream"]["sha256"]
    ev = "\n".join(amd.format_events(d.pop_events(0)))
    assert hashlib.sha256(ev.encode()).hexdigest() == pins["1000_frames_stream"]["events_sha256"]
    assert np.array_equal(fr, tx) and (meta_f["viterbi_metric"] == 0).all()
    st = d.state(0)
    assert st.frames_decoded == 1000 and st.frames_perfect == 1000 and st.est_offset_hz == 1430.0
    no_ties(st, "configs[1]")
    d.close()


def test_64_streams_device_channel_round_trip(amd, oracle):
    """BASELINE configs[3] shape: 64 concurrent streams from the device channel tool (HBM-resident,
    zero-copy attach). Size-independent properties: every stream releases every frame, in order;
    noiseless streams decode every frame exactly; two sampled streams equal the oracle bit for bit."""
    import ctypes as C
    import torch
    F, S = 60, 64
    tx = amd.bert_frames(F)
    base = amd.modulate(tx)
    n = base.size // 2
    dev = torch.device("cuda", 0)
    d_base = torch.from_numpy(base).to(dev)
    d_iq = torch.empty((S, 2 * n), dtype=torch.int16, device=dev)
    d = amd.Demod(S, max_samples=n + 64, streaming=True)
    for k in range(S):
        sigma = 0.0 if k % 2 == 0 else 2005.0        # odd streams: 16 dB
        d.channel(d_base.data_ptr(), d_iq[k].data_ptr(), n, gain=2000.0 / 16383.0, f0_hz=-1500.0 + 3000.0 * k / 63,
                  sigma=sigma, seed=77 + k)
    d.sync()
    for k in range(S):
        d.attach(k, d_iq[k].data_ptr(), n, eof=True)
    d.process()
    d.sync()
    for k in range(S):
        fr, meta = d.pop_frames(k)
        assert len(fr) == F, k
        if k % 2 == 0:
            assert np.array_equal(fr, tx), k
        else:
            assert (fr == tx).all(axis=1).mean() > 0.95, k
        assert np.array_equal(meta["release_symbol"][1:] - meta["release_symbol"][:-1], np.full(F - 1, 2168)), k
        no_ties(d.state(k), f"stream {k}")
    for k in (5, 62):
        x = d_iq[k].cpu().numpy()
        exp = oracle.receive(x, streaming=True)
        d2 = amd.Demod(1, max_samples=n + 64, streaming=True)
        got = d2.receive([x])[0]
        check_stream(amd, got, exp, f"device-channel stream {k}")
        d2.close()
    d.close()


def test_long_stream_through_a_small_device_buffer(amd, oracle, iq100):
    """opv-modem keeps one demodulator alive for hours: a pushed stream may be far longer than the
    device buffers (opv_cfg.max_samples). 100 frames (8.7 M samples) through a 3-chunk buffer in
    16 KB pushes: consumed IQ / soft symbols are dropped on the fly, record rings wrap, and the
    frames, metrics, sync positions and tracker lines still equal the oracle's."""
    x = impair(iq100, amp=2500.0, f0_hz=-900.0, ebn0_db=13.0, seed=21)
    exp = oracle.receive(x, streaming=True)
    cap = 3 * 86720 + 8192
    d = amd.Demod(1, max_samples=cap, streaming=True)
    frames, metas, events = [], [], []
    step = 2 * 4096
    for o in range(0, x.size, step):
        d.push(0, x[o:o + step])
        d.process()
        f, m = d.pop_frames(0)
        frames.append(f)
        metas.append(m)
        events.append(d.pop_events(0))
    d.flush(0)
    d.process()
    f, m = d.pop_frames(0)
    frames.append(f)
    metas.append(m)
    events.append(d.pop_events(0))
    frames, metas, events = np.concatenate(frames), np.concatenate(metas), np.concatenate(events)
    assert len(frames) == len(exp["frames"]) > 90
    assert np.array_equal(frames, exp["frames"])
    assert np.array_equal(metas["viterbi_metric"], exp["metrics"])
    assert np.array_equal(metas["release_symbol"], exp["frame_sym"])
    events_match(amd, events, exp["events"])
    st = d.state(0)
    assert st.total_symbols == exp["n_soft"] and st.n_chunks == len(exp["chunks"])
    assert st.frames_decoded == len(exp["frames"])
    assert abs(st.freq_offset_hz - exp["final_freq_offset"]) < 1e-6
    tail = d.soft(0, first=exp["n_soft"] - 1000)
    a, _ = soft_err(tail, exp["soft"][-1000:])
    assert a < SOFT_TIGHT
    with pytest.raises(amd.OpvError):
        d.soft(0, first=0)                     # long gone
    d.close()
    # a push that cannot fit even after dropping everything consumed is refused loudly
    d = amd.Demod(1, max_samples=100000, streaming=True)
    with pytest.raises(amd.OpvError):
        d.push(0, x[: 2 * 150000])
    d.close()


def compaction_plan(chunks, total, sizes, cap):
    """What the pushes of one stream make of its device buffer, on the CPU: the oracle's chunk log gives the chunk origins (a
    call of 86720 samples that leaves 0 < leftover < 86720 behind advances by what it used), a round takes every whole chunk
    that has arrived, and a push that does not fit drops what lies in front of iq_keep(origin) = (origin - 16) & ~3 (csrc/opv_stream_rules.h).
    Returns per push (first, n, origin after its round, retained tail if the push compacted else None, iq_base after the push)."""
    origins = [0]
    for c in chunks:
        left = int(c[3])
        origins.append(origins[-1] + (86720 - left if 0 < left < 86720 else 86720))
    plan, pushed, base, origin, k, j = [], 0, 0, 0, 0, 0
    while pushed < total:
        n = min(sizes[j % len(sizes)], total - pushed)
        tail = None
        if pushed - base + n > cap:
            keep = ((origin - base - 16) & ~3) if origin - base >= 16 else 0
            base += keep
            tail = pushed - base
            assert keep and tail + n <= cap
        while k + 1 < len(origins) and origins[k] + 86720 <= pushed + n:
            k += 1
        origin = origins[k]
        plan.append((pushed, n, origin, tail, base))
        pushed += n
        j += 1
    return plan


def test_single_stream_compaction_at_every_tail_length(amd, oracle, iq100):
    """The compaction of ONE stream goes through the table-driven kernel too (a list of one: csrc/opv_push.hip, compact_streams).
    A capture through a 3-chunk buffer in pushes of 4097, 1, 86723 and 40001 samples with a round after each: the retained tail
    takes every length mod 4 (whole 16-byte moves + 0..3 samples) and once is shorter than 1024 samples (one slice), all of
    which is checked on the CPU first. It takes the 100-frame capture for that (267 pushes, 42 of them compacting, the
    shortest tail 72 samples): the 10-frame one compacts three times, with tails of 5718, 7322 and 4828 samples. Around every compacting push the last 64 samples read the same, the samples in front of
    the keep point are gone, and at the end frames, metrics, release symbols, events and every soft symbol are the oracle's.
    Stream 1 holds half a chunk and is never full: compaction leaves it alone."""
    x = iq100
    total = x.size // 2
    exp = oracle.receive(x, streaming=True)
    cap = 3 * 86720 + 8192
    plan = compaction_plan(exp["chunks"], total, (4097, 1, 86723, 40001), cap)
    tails = [t for _, _, _, t, _ in plan if t is not None]
    assert {t & 3 for t in tails} == {0, 1, 2, 3} and any(t < 1024 for t in tails) and any(t >= 1024 for t in tails), tails
    d = amd.Demod(2, max_samples=cap, streaming=True)
    other = np.ascontiguousarray(x[: 2 * 43360])
    d.push(1, other)
    frames, metas, events, softs, seen = [], [], [], [], 0
    for first, n, origin, tail, base in plan:
        before = d.iq(0, first=first - 64, cap=64) if tail is not None else None
        d.push(0, x[2 * first: 2 * (first + n)])
        if tail is not None:
            assert np.array_equal(before, x[2 * (first - 64): 2 * first]) and np.array_equal(d.iq(0, first=first - 64, cap=64), before), first
            assert d.iq(0, first=base - 1, cap=1).size == 0 and np.array_equal(d.iq(0, first=base, cap=1), x[2 * base: 2 * base + 2]), first
        d.process()
        assert d.state(0).chunk_origin == origin, (first, n)
        f, m = d.pop_frames(0)
        frames.append(f)
        metas.append(m)
        events.append(d.pop_events(0))
        softs.append(d.soft(0, first=seen))
        seen += len(softs[-1])
    d.flush(0)
    d.process()
    f, m = d.pop_frames(0)
    frames, metas, events = np.concatenate(frames + [f]), np.concatenate(metas + [m]), np.concatenate(events + [d.pop_events(0)])
    soft = np.concatenate(softs + [d.soft(0, first=seen)])
    assert len(frames) == len(exp["frames"]) == 100 and np.array_equal(frames, exp["frames"])
    assert np.array_equal(metas["viterbi_metric"], exp["metrics"])
    assert np.array_equal(metas["release_symbol"], exp["frame_sym"])
    events_match(amd, events, exp["events"])
    st = d.state(0)
    assert st.total_symbols == exp["n_soft"] == len(soft) and st.n_chunks == len(exp["chunks"])
    assert abs(st.freq_offset_hz - exp["final_freq_offset"]) < 1e-6
    a, _ = soft_err(soft, exp["soft"])
    assert a < SOFT_TIGHT
    assert d.state(1).chunk_origin == 0 and np.array_equal(d.iq(1, first=0), other)
    d.close()


def test_device_modulator_is_bit_identical_to_host_and_reference(amd, golden):
    """the TX chain writing straight into HBM. Same bytes as the host
    modulator, hence (sha256 pins) as the reference `opv-mod`."""
    import torch
    _, meta = golden
    pins = meta["opv_mod_bert_W5NYV"]
    d = amd.Demod(1, max_samples=1 << 20)
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(3)
    for frames, pin in ((amd.bert_frames(10), pins["10"]["sha256"]), (amd.bert_frames(100), pins["100"]["sha256"]),
                        (rng.integers(0, 256, (7, 134), dtype=np.uint8), None), (np.zeros((0, 134), np.uint8), None)):
        n = amd.lib().opv_tx_modulated_samples(len(frames))
        out = torch.empty(2 * n, dtype=torch.int16, device=dev)
        patched = d.modulate_device(frames, out.data_ptr())
        got = out.cpu().numpy()
        assert np.array_equal(got, amd.modulate(frames)), f"{len(frames)} frames, {patched} patched"
        if pin:
            assert hashlib.sha256(got.tobytes()).hexdigest() == pin
        print(len(frames), "frames: host-patched samples:", patched)
    d.close()


def test_device_transmit_chain_lengths_order_and_table_end(amd, golden):
    """The device transmit chain end to end (k_tx_encode -> k_tx_scan_frames -> k_tx_expand_phases -> k_tx_modulate):
    run lengths in ANY order on one context (the phase table grows and is re-used: 3, 1000, 40 frames; 1000 = BASELINE
    configs[1]'s capture, sha256 = `opv-mod -S W5NYV -B 1000`), adversarial payloads (all ones / all zeros / alternating: the
    differential sign and the tone choice at their extremes), and a run LONGER than the build-time NCO table (4096 frames), whose
    last checkpoints continue the recurrence on the host."""
    import torch
    _, meta = golden
    pins = meta["opv_mod_bert_W5NYV"]
    dev = torch.device("cuda", 0)
    d = amd.Demod(1, max_samples=1 << 20)
    for nfr in (3, 1000, 40):
        frames = amd.bert_frames(nfr)
        n = amd.lib().opv_tx_modulated_samples(nfr)
        out = torch.empty(2 * n, dtype=torch.int16, device=dev)
        d.modulate_device(frames, out.data_ptr())
        got = out.cpu().numpy()
        if nfr == 1000:
            assert hashlib.sha256(got.tobytes()).hexdigest() == pins["1000"]["sha256"]
        else:
            assert np.array_equal(got, amd.modulate(frames)), nfr
    pat = np.stack([np.full(134, 0xFF, np.uint8), np.zeros(134, np.uint8), np.full(134, 0xAA, np.uint8), np.full(134, 0x55, np.uint8),
                    np.arange(134, dtype=np.uint8)] * 3)
    n = amd.lib().opv_tx_modulated_samples(len(pat))
    out = torch.empty(2 * n, dtype=torch.int16, device=dev)
    d.modulate_device(pat, out.data_ptr())
    assert np.array_equal(out.cpu().numpy(), amd.modulate(pat))
    d.close()
    # past the end of the build-time NCO table (4096 frames): the checkpoints beyond it continue the recurrence on the host,
    # once per process. 4200 frames of random payloads on the device (1.46 GB of int16 IQ) against the host modulator run
    # through the same frames in pieces of 100 (its state carried from piece to piece), every piece compared sample for sample
    nfr = OPV_TX_TABLE_FRAMES + 104
    rng = np.random.default_rng(4096)
    frames = rng.integers(0, 256, (nfr, 134), dtype=np.uint8)
    n = amd.lib().opv_tx_modulated_samples(nfr)
    out = torch.empty(2 * n, dtype=torch.int16, device=dev)
    d = amd.Demod(1, max_samples=1 << 16)
    patched = d.modulate_device(frames, out.data_ptr())
    d.close()
    print(f"{nfr} frames on the device: {patched} samples re-evaluated on the host")
    tx = amd.TxStream()
    per = 2 * 2168 * 40
    for a in range(0, nfr, 100):
        b = min(a + 100, nfr)
        want = tx.frames(frames[a:b])
        assert np.array_equal(out[a * per: b * per].cpu().numpy(), want), f"frames {a}..{b} of {nfr} (table ends at {OPV_TX_TABLE_FRAMES})"
    tx.close()
    assert not out[nfr * per:].any()                  # the 100 trailing zero symbols (ref src/opv-mod.cpp:528-529)


def test_device_transmit_chain_past_the_flat_top_flip(amd):
    """Runs longer than 1563 frames: from there on glibc's sin / cos at the flat tops of the NCOs (one per symbol start and
    tone) is 1 - 2^-53, not 1.0, and 16383 x truncates to 16382 (k_tx_modulate.hip; round 3's first build flagged every such
    sample as ambiguous and gave up from ~1570 frames). One context, lengths in an order that grows and shrinks the cached
    zone bits; every run equals the host modulator (= opv-mod, by its sha256 pins) sample for sample, nothing patched."""
    import torch
    rng = np.random.default_rng(91)
    fr = rng.integers(0, 256, (2600, 134), dtype=np.uint8)
    d = amd.Demod(1, max_samples=1 << 16)
    for n in (1450, 2600, 1700, 900):
        ns = amd.lib().opv_tx_modulated_samples(n)
        out = torch.empty(2 * ns, dtype=torch.int16, device="cuda")
        assert d.modulate_device(fr[:n], out.data_ptr()) == 0, n
        assert np.array_equal(out.cpu().numpy(), amd.modulate(fr[:n])), n
        del out
    d.close()


def test_device_transmit_chain_with_a_distrusted_libm():
    """The flat-top zones are a statement about the process's libm; the library probes it once (opv_tx_libm_flat_tops_as_assumed,
    opv_tx_device.hip) and, if it answers differently, takes every symbol's flat-top bits from libm itself. That path, forced
    through OPV_TX_DISTRUST_LIBM in a child process (the probe's result is per process): runs shorter and longer than the
    1563-frame flip still equal the host modulator sample for sample."""
    import subprocess
    import sys
    code = (
        "import sys, numpy as np, torch\n"
        "sys.path.insert(0, %r)\n"
        "from amd_lib import load\n"
        "amd = load()\n"
        "fr = np.random.default_rng(92).integers(0, 256, (1800, 134), dtype=np.uint8)\n"
        "d = amd.Demod(1, max_samples=1 << 16)\n"
        "for n in (40, 1800, 1600):\n"
        "    ns = amd.lib().opv_tx_modulated_samples(n)\n"
        "    out = torch.empty(2 * ns, dtype=torch.int16, device='cuda')\n"
        "    assert d.modulate_device(fr[:n], out.data_ptr()) == 0, n\n"
        "    assert np.array_equal(out.cpu().numpy(), amd.modulate(fr[:n])), n\n"
        "d.close()\n"
        "print('distrusted-libm path ok')\n") % str(Path(__file__).resolve().parent)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, OPV_TX_DISTRUST_LIBM="1"), capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "distrusted-libm path ok" in p.stdout, p.stderr[-2000:]


def test_idle_process_on_the_zero_copy_path_launches_nothing(amd, iq10):
    """A caller that only uses opv_device_frames + opv_sync never refreshes the host mirror; an opv_process with nothing new
    must still be a no-op for it (the library reads 'a stream ended the round stalled' from a pinned word the last round's
    kernels wrote), not a whole round of launches: the timing events of the last real round are untouched."""
    import torch
    d = amd.Demod(2, max_samples=iq10.size // 2 + 64, streaming=True)
    t = torch.from_numpy(iq10.copy()).cuda()
    for k in range(2):
        d.attach(k, t.data_ptr(), iq10.size // 2, eof=True)
    d.enable_timing(True)
    d.process()
    d.sync()
    first = d.kernel_times()
    for _ in range(3):
        d.process()                                      # nothing new, nothing stalled
        d.sync()
    assert d.kernel_times() == first                     # (a relaunch re-records the events: the floats would differ)
    assert len(d.pop_frames(0)[0]) == 10 and len(d.pop_frames(1)[0]) == 10
    d.close()


def test_opv_mod_cli_on_the_gpu(amd, golden):
    """`bin/opv-mod -G 0`: the reference's modulator CLI with the transmit chain on the device - BERT and raw mode, the same
    bytes as the reference `opv-mod` (sha256 pins) / as the host chain."""
    import subprocess
    _, meta = golden
    pins = meta["opv_mod_bert_W5NYV"]
    exe = str(amd.PKG / "bin" / "opv-mod")
    out = subprocess.run([exe, "-S", "W5NYV", "-B", "100", "-G", "0"], capture_output=True, timeout=300)
    assert out.returncode == 0, out.stderr.decode()
    assert hashlib.sha256(out.stdout).hexdigest() == pins["100"]["sha256"]
    raw = np.random.default_rng(8).integers(0, 256, (5, 134), dtype=np.uint8)
    a = subprocess.run([exe, "-R", "-G", "0"], input=raw.tobytes(), capture_output=True, timeout=300)
    b = subprocess.run([exe, "-R"], input=raw.tobytes(), capture_output=True, timeout=300)
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and len(a.stdout) == (5 * 2168 + 100) * 40 * 4


def test_batch_mode_100_frames_noisy(amd, oracle, iq100):
    """Batch mode = ONE demodulate() over the whole capture (reference :1173): pos runs to 8.7e6
    (fp64 resolution of the sample position matters there) and there are no chunk artefacts."""
    x = impair(iq100, amp=3000.0, f0_hz=1100.0, ebn0_db=11.0, seed=9)
    d = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=False)
    got = d.receive([x])[0]
    check_stream(amd, got, oracle.receive(x, streaming=False), "batch 100 frames 11 dB")
    d.close()


def test_reset_and_reuse_and_two_contexts(amd, oracle, iq10):
    x = impair(iq10, amp=2000.0, f0_hz=300.0, ebn0_db=15.0, seed=4)
    exp = oracle.receive(x, streaming=True)
    a = amd.Demod(2, max_samples=x.size // 2 + 64, streaming=True)
    b = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=True)
    for rep in range(2):
        got = a.receive([x, iq10])
        check_stream(amd, got[0], exp, f"ctx a rep {rep}")
        gb = b.receive([x])[0]
        check_stream(amd, gb, exp, f"ctx b rep {rep}")
        a.reset()
        b.reset(0)
    a.close()
    b.close()


def test_growing_attached_capture(amd, oracle, iq10):
    """Zero-copy path fed incrementally: the caller's HBM buffer grows (eof=False), then ends."""
    import torch
    dev = torch.device("cuda", 0)
    d_x = torch.from_numpy(iq10).to(dev)
    n = iq10.size // 2
    d = amd.Demod(1, max_samples=n + 64, streaming=True)
    for upto in (50000, 86720, 300000, 300001, n - 7, n):
        d.attach(0, d_x.data_ptr(), upto, eof=(upto == n))
        d.process()
    d.sync()
    fr, meta = d.pop_frames(0)
    exp = oracle.receive(iq10, streaming=True)
    assert np.array_equal(fr, exp["frames"]) and np.array_equal(meta["release_symbol"], exp["frame_sym"])
    a, _ = soft_err(d.soft(0), exp["soft"])
    assert a < SOFT_TIGHT
    d.close()


@pytest.mark.parametrize("f0,ebn0", [(2000.0, 6.0), (-2000.0, 12.0)])
def test_config2_full_size_offset_awgn(amd, oracle, f0, ebn0):
    """BASELINE configs[2] at full size: 1000 frames, +/-2 kHz carrier offset (= the AFC clamp, outside
    the +/-1530 Hz search span) and AWGN (at 6 dB the reference decodes only flywheel garbage: parity
    there means identical threshold crossings and quantiser roundings). Everything
    the reference would print or write must match the oracle bit for bit over ~2.17 M symbols."""
    import torch
    tx = amd.bert_frames(1000)
    d = amd.Demod(1, max_samples=86724000 + 64, streaming=True)
    dev = torch.device("cuda", 0)
    n = amd.lib().opv_tx_modulated_samples(1000)
    clean = torch.empty(2 * n, dtype=torch.int16, device=dev)
    noisy = torch.empty(2 * n, dtype=torch.int16, device=dev)
    d.modulate_device(tx, clean.data_ptr())
    sigma = float(np.sqrt(80.0 * 2000.0 ** 2 / 10.0 ** (ebn0 / 10.0) / 2.0))
    d.channel(clean.data_ptr(), noisy.data_ptr(), n, gain=2000.0 / 16383.0, f0_hz=f0, sigma=sigma, seed=123)
    d.sync()
    x = noisy.cpu().numpy()
    d.attach(0, noisy.data_ptr(), n, eof=True)
    d.process()
    fr, meta = d.pop_frames(0)
    ev = d.pop_events(0)
    st = d.state(0)
    exp = oracle.receive(x, streaming=True)
    print(f"f0={f0} Eb/N0={ebn0}: {len(fr)} frames, {int((meta['viterbi_metric'] == 0).sum())} perfect, "
          f"{int((fr[:len(tx)] == tx[:len(fr)]).all(axis=1).sum()) if len(fr) <= len(tx) else 'n/a'} equal to the transmitted ones")
    assert np.array_equal(fr, exp["frames"])
    assert np.array_equal(meta["viterbi_metric"], exp["metrics"])
    assert np.array_equal(meta["release_symbol"], exp["frame_sym"])
    print("printed tracker lines differing in the last digit of raw=:", events_match(amd, ev, exp["events"]), "of", len(ev))
    assert st.total_symbols == exp["n_soft"] and st.est_offset_hz == exp["est_offset"]
    no_ties(st, "configs[2]")
    a, r = soft_err(d.soft(0), exp["soft"])
    print(f"soft max|d|/mean = {a:.2e}, max rel = {r:.2e}")
    assert a < SOFT_TIGHT and r < SOFT_RTOL
    d.close()


def test_frames_only_consumer_and_back_pressure(amd, oracle, iq100):
    """What opv-modem does with its child: it reads FRAMES and sends the tracker lines to /dev/null. A receiver
    that never calls opv_pop_events must run forever: the event log is lossy (most recent cap_events lines, the
    rest counted in events_dropped). Here 100 frames go through a 3-chunk staging buffer (7 frame slots, 92 event
    slots; 102 tracker lines), frames popped every round, events never - then the retained tail of the log must be the
    oracle's last lines. Second half: a consumer that stops popping FRAMES gets back-pressure, not data loss: the
    stream pauses (state.stalled), pushes are refused with OPV_ECAPACITY once the staging buffer is full, and
    after the pops it resumes where it stopped - every frame still equal to the oracle's."""
    x = iq100
    exp = oracle.receive(x, streaming=True)
    cap = 3 * 86720 + 8192
    n_slots = 4 * (cap // (2168 * 38) + 4) + 64          # opv_create: cap_events = 4 cap_frames + 64
    d = amd.Demod(1, max_samples=cap, streaming=True)
    frames = []
    step = 2 * 86720
    for o in range(0, x.size, step):
        d.push(0, x[o:o + step])
        d.process()
        frames.append(d.pop_frames(0)[0])
    d.flush(0)
    d.process()
    frames.append(d.pop_frames(0)[0])
    frames = np.concatenate(frames)
    assert np.array_equal(frames, exp["frames"]) and len(frames) == 100
    st = d.state(0)
    assert st.stalled == 0
    n_ev = len(exp["events"])
    assert n_ev > n_slots, (n_ev, n_slots)
    assert st.events_dropped == n_ev - n_slots, (st.events_dropped, n_ev)
    tail = d.pop_events(0)
    assert len(tail) == n_slots
    events_match(amd, tail, exp["events"][-n_slots:])
    assert d.state(0).events_dropped == n_ev - n_slots
    d.close()

    # back-pressure: frames are never dropped (this context holds 7 unpopped frames per stream)
    d = amd.Demod(1, max_samples=cap, streaming=True)
    got, refused, o = [], 0, 0
    stalled_seen = False
    while o < x.size:
        try:
            d.push(0, x[o:o + step])
            o += step
        except amd.OpvError as e:
            assert "-4" in str(e)                         # OPV_ECAPACITY: pop, then push again
            refused += 1
            stt = d.state(0)
            stalled_seen |= stt.stalled != 0
            f = d.pop_frames(0)[0]
            assert len(f) > 0, "a refused push must come with frames waiting to be popped"
            got.append(f)
            d.process()                                   # resumes the paused stream
            continue
        d.process()
    d.flush(0)
    for _ in range(40):
        d.process()
        f = d.pop_frames(0)[0]
        got.append(f)
        stt = d.state(0)
        if stt.flushed and stt.stalled == 0 and len(f) == 0:
            break
    got = np.concatenate(got)
    assert refused >= 3 and stalled_seen, (refused, stalled_seen)
    assert np.array_equal(got, exp["frames"]), (len(got), len(exp["frames"]))
    assert d.state(0).total_symbols == exp["n_soft"]
    d.close()


def test_rx_bridge_multi_stream_udp(amd, oracle, tmp_path):
    """the caller side of the boundary. Three IQ files -> opv-rx-bridge (one GPU
    context, 16 KB reads like opv-modem) -> 134-byte UDP datagrams on ports base+k; every stream's
    datagrams must be the oracle's frames, in order."""
    import socket
    import subprocess
    base = 40000 + (os.getpid() % 2000) * 4
    socks = []
    for k in range(3):
        so = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        so.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
        so.bind(("127.0.0.1", base + k))
        so.setblocking(False)
        socks.append(so)
    caps, exps = [], []
    for k in range(3):
        x = oracle.modulate(oracle.bert_frames(12 + 3 * k, f"K{k}XYZ", 0xBBAADD, 50 * k))
        if k == 2:
            x = impair(x, amp=2500.0, f0_hz=800.0, ebn0_db=14.0, seed=k)
        f = tmp_path / f"s{k}.iq"
        x.tofile(f)
        caps.append(str(f))
        exps.append(oracle.receive(x, streaming=True)["frames"])
    exe = str(amd.PKG / "bin" / "opv-rx-bridge")
    r = subprocess.run([exe, "-P", str(base)] + caps, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    for k in range(3):
        got = []
        while True:
            try:
                got.append(socks[k].recv(2048))
            except BlockingIOError:
                break
        assert all(len(g) == FRAME_BYTES for g in got)
        got = np.frombuffer(b"".join(got), np.uint8).reshape(-1, FRAME_BYTES)
        assert np.array_equal(got, exps[k]), f"stream {k}: {len(got)} datagrams vs {len(exps[k])} frames"
        socks[k].close()


def test_rx_bridge_shards_over_contexts_and_gathers_in_cxx(amd, oracle, tmp_path):
    """The C++ side of BASELINE configs[4] (north_star: "Host code stays C++ ... RCCL ... only to gather decoded frames"):
    `opv-rx-bridge --devices a,b` shards its inputs contiguously over one context per listed GPU (stream k -> context
    k / ceil(S / N)); on this one-GPU box the list is 0,0 - two independent contexts on the same device - and five inputs
    land 3 + 2. Every stream's datagrams must be the oracle's frames. `--devices 0 --gather` then runs the path's one
    collective from the stand-alone C++ process: opv_comm_init_all + opv_gather_frames_all (ncclGather through the
    SYSTEM's librccl, bound by dlopen), world 1 here, and checks the gathered counts against the local ones."""
    import socket
    import subprocess
    base = 42000 + (os.getpid() % 1500) * 5
    S = 5
    socks = []
    for k in range(S):
        so = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        so.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
        so.bind(("127.0.0.1", base + k))
        so.setblocking(False)
        socks.append(so)
    caps, exps = [], []
    for k in range(S):
        x = oracle.modulate(oracle.bert_frames(6 + 2 * k, f"D{k}", 0xBBAADD, 9 * k))
        if k % 2:
            x = impair(x, amp=3000.0, f0_hz=-500.0 + 300.0 * k, ebn0_db=15.0, seed=10 + k)
        f = tmp_path / f"d{k}.iq"
        x.tofile(f)
        caps.append(str(f))
        exps.append(oracle.receive(x, streaming=True)["frames"])
    exe = str(amd.PKG / "bin" / "opv-rx-bridge")

    def collect():
        out = []
        for k in range(S):
            got = []
            while True:
                try:
                    got.append(socks[k].recv(2048))
                except BlockingIOError:
                    break
            out.append(np.frombuffer(b"".join(got), np.uint8).reshape(-1, FRAME_BYTES))
        return out

    r = subprocess.run([exe, "-P", str(base), "--devices", "0,0"] + caps, capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    assert b"3 per context on 2 contexts" in r.stderr, r.stderr.decode()
    for k, got in enumerate(collect()):
        assert np.array_equal(got, exps[k]), f"--devices 0,0 stream {k}: {len(got)} datagrams vs {len(exps[k])} frames"
    r = subprocess.run([exe, "-P", str(base), "--devices", "0", "--gather"] + caps, capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    total = sum(len(e) for e in exps)
    assert f"gather: 1 rank(s) x {S} stream(s) -> GPU 0 over RCCL: {total} frames released in all, 0 stream(s) differ" in err, err
    for k, got in enumerate(collect()):
        assert np.array_equal(got, exps[k]), k
    for so in socks:
        so.close()


@pytest.mark.skipif(_visible_gpus() < 2, reason="needs >= 2 GPUs (armed for an N-GPU box): opv-rx-bridge --devices 0,1 --gather")
def test_rx_bridge_gathers_over_two_devices_in_cxx(amd, oracle, tmp_path):
    """ARMED FOR AN N-GPU BOX (skipped on the 1-GPU pool): the stand-alone C++ host on two real devices - `opv-rx-bridge --devices
    0,1 --gather`: five inputs land 3 + 2 on a context per GPU, and the path's one collective (opv_comm_init_all +
    opv_gather_frames_all: two ncclGathers in one RCCL group, into GPU 0's HBM) returns every context's frame counts. Datagrams
    equal the oracle's frames; the bridge's own comparison of gathered and local counts reports no difference."""
    import socket
    import subprocess
    base = 42000 + (os.getpid() % 1500) * 5
    S = 5
    socks = []
    for k in range(S):
        so = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        so.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
        so.bind(("127.0.0.1", base + k))
        so.setblocking(False)
        socks.append(so)
    caps, exps = [], []
    for k in range(S):
        x = oracle.modulate(oracle.bert_frames(6 + 2 * k, f"E{k}", 0xBBAADD, 7 * k))
        if k % 2:
            x = impair(x, amp=3000.0, f0_hz=-500.0 + 300.0 * k, ebn0_db=15.0, seed=20 + k)
        f = tmp_path / f"e{k}.iq"
        x.tofile(f)
        caps.append(str(f))
        exps.append(oracle.receive(x, streaming=True)["frames"])
    exe = str(amd.PKG / "bin" / "opv-rx-bridge")
    r = subprocess.run([exe, "-P", str(base), "--devices", "0,1", "--gather"] + caps, capture_output=True, timeout=300)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert "3 per context on 2 contexts" in err, err
    total = sum(len(e) for e in exps)
    assert f"gather: 2 rank(s) x 3 stream(s) -> GPU 0 over RCCL: {total} frames released in all, 0 stream(s) differ" in err, err
    for k in range(S):
        got = []
        while True:
            try:
                got.append(socks[k].recv(2048))
            except BlockingIOError:
                break
        got = np.frombuffer(b"".join(got), np.uint8).reshape(-1, FRAME_BYTES)
        assert np.array_equal(got, exps[k]), f"--devices 0,1 stream {k}: {len(got)} datagrams vs {len(exps[k])} frames"
        socks[k].close()


def test_rx_bridge_64_streams_from_pinned_buffers(amd, oracle, tmp_path):
    """the bridge at the width of one GPU's share of BASELINE configs[4]: 64 inputs (four distinct captures, each named sixteen
    times) -> one context -> 64 UDP ports. Its read buffers are pinned, so every poll round is ONE opv_push_iq_batch through the
    gather kernel; every stream's datagrams must be the oracle's frames of its capture, in order."""
    import socket
    import subprocess
    S = 64
    base = 43000 + (os.getpid() % 300) * 70
    socks = []
    for k in range(S):
        so = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        so.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 21)
        so.bind(("127.0.0.1", base + k))
        so.setblocking(False)
        socks.append(so)
    files, exps = [], []
    for j in range(4):
        x = oracle.modulate(oracle.bert_frames(5 + j, f"W{j}", 0xBBAADD, 11 * j))
        if j % 2:
            x = impair(x, amp=2800.0, f0_hz=350.0 * j - 600.0, ebn0_db=15.0, seed=30 + j)
        f = tmp_path / f"w{j}.iq"
        x.tofile(f)
        files.append(str(f))
        exps.append(oracle.receive(x, streaming=True)["frames"])
    exe = str(amd.PKG / "bin" / "opv-rx-bridge")
    r = subprocess.run([exe, "-q", "-P", str(base)] + [files[k % 4] for k in range(S)], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    for k in range(S):
        got = []
        while True:
            try:
                got.append(socks[k].recv(2048))
            except BlockingIOError:
                break
        got = np.frombuffer(b"".join(got), np.uint8).reshape(-1, FRAME_BYTES)
        assert np.array_equal(got, exps[k % 4]), f"stream {k}: {len(got)} datagrams vs {len(exps[k % 4])} frames"
        socks[k].close()


@pytest.mark.parametrize("pipelined", [False, True])
def test_live_capacity_tool_checks_what_it_times(amd, pipelined):
    """bin/opv-live-capacity (bench.py extras.live_capacity; a C++ caller of the C ABI like the bridge): 200 streams, 12 serving
    rounds - every stream listens to one long BERT run from its own frame on, each round pushes one 40 ms chunk per stream from
    pinned host memory, processes, pops. The tool compares every popped frame with what was sent: none wrong, all perfect, one frame
    per stream and round - in the serial loop and in the double-buffered one (opv_push_iq_batch_async / opv_push_wait)."""
    import json
    import subprocess
    exe = str(amd.PKG / "bin" / "opv-live-capacity")
    r = subprocess.run([exe, "200", "12", "3", "0"] + (["--pipelined"] if pipelined else []), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1000:]
    j = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert j["streams"] == 200 and j["pipelined"] is pipelined and j["rounds"] == 12
    assert j["frames_wrong"] == 0 and j["frames_imperfect"] == 0 and j["rounds_not_one_frame_per_stream"] == 0
    assert j["frames_released"] == 200 * 14                      # 15 rounds in all, the first one releases nothing
    assert 0.0 < j["round_ms_p50"] < 40.0


def test_rx_bridge_udp_and_stdin_sources(amd, oracle, tmp_path):
    """SURVEY.md §8f row 3, the source side: one stream from stdin ('-'), one from UDP datagrams (udp:PORT, ended by
    an empty datagram), one from a file - the three in one GPU context; every stream's output datagrams are the
    oracle's frames."""
    import socket
    import subprocess
    import threading
    import time
    base = 42000 + (os.getpid() % 1500) * 4
    in_port = base + 3
    socks = []
    for k in range(3):
        so = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        so.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
        so.bind(("127.0.0.1", base + k))
        so.setblocking(False)
        socks.append(so)
    caps = [oracle.modulate(oracle.bert_frames(6 + k, f"U{k}", 0xBBAADD, 9 * k)) for k in range(3)]
    caps[1] = impair(caps[1], amp=3000.0, f0_hz=-600.0, ebn0_db=15.0, seed=4)
    exps = [oracle.receive(x, streaming=True)["frames"] for x in caps]
    f2 = tmp_path / "s2.iq"
    caps[2].tofile(f2)
    exe = str(amd.PKG / "bin" / "opv-rx-bridge")
    p = subprocess.Popen([exe, "-q", "-P", str(base), "-", f"udp:{in_port}", str(f2)], stdin=subprocess.PIPE, stderr=subprocess.PIPE)

    def feed_udp():
        time.sleep(1.5)                                  # the bridge binds its socket before it creates the GPU context
        tx = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        raw = caps[1].tobytes()
        for o in range(0, len(raw), 8190):               # datagram sizes that are NOT a multiple of 4: samples straddle packets
            tx.sendto(raw[o:o + 8190], ("127.0.0.1", in_port))
            time.sleep(0.0004)                           # ~20 MB/s: well inside the 8 MB socket buffer
        tx.sendto(b"", ("127.0.0.1", in_port))
        tx.close()
    th = threading.Thread(target=feed_udp)
    th.start()
    p.stdin.write(caps[0].tobytes())
    p.stdin.close()
    th.join()
    assert p.wait(timeout=300) == 0, p.stderr.read().decode()
    for k in range(3):
        got = []
        while True:
            try:
                got.append(socks[k].recv(2048))
            except BlockingIOError:
                break
        got = np.frombuffer(b"".join(got), np.uint8).reshape(-1, FRAME_BYTES)
        assert np.array_equal(got, exps[k]), f"stream {k}: {len(got)} datagrams vs {len(exps[k])} frames"
        socks[k].close()


def test_config3_full_size_all_streams(amd):
    """BASELINE configs[3] at full size, ALL 64 streams: bench.py's own workload - SURVEY.md §8(d) C4 as written
    (workload.generate: device modulator, per-stream payload, f0 from -2000 to +2000 Hz across the 64 streams, 16 dB;
    64 x 86 724 000 samples in HBM) - through ONE opv_process, and every stream against the oracle run on its own bytes (a
    process pool over the job's host cores, a wave of streams in host memory at a time): frames, Viterbi metrics, release
    symbols, tracker events, symbol count, offset estimate, final AFC, no one-tap windows (ref src/opv-demod.cpp:1012-1113).
    The two edge streams (f0 = -/+2000 Hz: the AFC pinned at its clamp :303, the offset estimate saturating at the end of
    its +/-1530 Hz span :135,169) and two interior ones also have ALL their ~2.17 M soft symbols compared (< 1e-9 of the
    mean magnitude; contract 1e-5)."""
    import torch
    from concurrent.futures import ProcessPoolExecutor
    from __graft_entry__ import load_pkg_module
    from soak_inputs import host_workers, oracle_receive_job
    workload = load_pkg_module("workload")
    S, F = 64, 1000
    SOFT_STREAMS = (0, 21, 42, 63)
    assert [workload.stream_params(k, 16.0)[2] for k in (0, 63)] == [-2000.0, 2000.0]     # the recipe the bench line names
    dev = torch.device("cuda", 0)
    n = amd.lib().opv_tx_modulated_samples(F)
    d = amd.Demod(S, max_samples=n + 64, streaming=True)
    d_iq, tx, n = workload.generate(amd, d, torch, dev, range(S), F, 16.0)
    for k in range(S):
        d.attach(k, d_iq[k].data_ptr(), n, eof=True)
    d.process()
    d.sync()
    if not os.environ.get("OPV_FRONTEND"):                        # (dev switch: the whole suite on one mapping)
        assert d.frontend_kernel() == "k_msk_frontend_rb"        # the kernel the bench line's roofline is about
    W = host_workers()
    exact = total = 0
    per_stream = {}
    with ProcessPoolExecutor(W) as pool:
        for k0 in range(0, S, W):
            futs = {k: pool.submit(oracle_receive_job, d_iq[k].cpu().numpy(), k in SOFT_STREAMS) for k in range(k0, min(S, k0 + W))}
            for k, fut in futs.items():
                exp = fut.result()
                fr, meta = d.pop_frames(k)
                assert len(fr) == len(exp["frames"]) and np.array_equal(fr, exp["frames"]), k
                assert np.array_equal(meta["viterbi_metric"], exp["metrics"]), k
                assert np.array_equal(meta["release_symbol"], exp["frame_sym"]), k
                events_match(amd, d.pop_events(k), exp["events"])
                st = d.state(k)
                assert st.total_symbols == exp["n_soft"] and st.est_offset_hz == exp["est_offset"], k
                assert abs(st.freq_offset_hz - exp["final_freq_offset"]) < 1e-6, k
                no_ties(st, f"configs[3] stream {k}", offset_ties=None)
                if k in SOFT_STREAMS:
                    a, r = soft_err(d.soft(k), exp["soft"])
                    print(f"configs[3] stream {k} (f0 {workload.stream_params(k, 16.0)[2]:+.1f} Hz, estimate {st.est_offset_hz:+.1f}, "
                          f"final AFC {st.freq_offset_hz:+.2f}): {len(exp['soft'])} soft symbols, max|d|/mean = {a:.2e}, max rel = {r:.2e}")
                    assert a < SOFT_TIGHT and r < SOFT_RTOL, k
                ok = int((fr[:F] == tx[k][: len(fr)]).all(axis=1).sum()) if len(fr) <= F else 0
                per_stream[k] = (len(fr), ok, st.offset_ties)
                exact += ok
                total += len(fr)
    worst = sorted(per_stream.items(), key=lambda kv: kv[1][1])[:4]
    print("configs[3]: frames released", total, "equal to the transmitted ones", exact, "worst streams (released, exact, offset_ties)", worst)
    assert sum(v[2] for v in per_stream.values()) <= 2            # (the near-tie guard: rare on ordinary captures, no_ties)
    assert all(v[0] == F for v in per_stream.values()), {k: v for k, v in per_stream.items() if v[0] != F}
    assert total == S * F and exact >= 0.99 * total              # (the rest: channel errors at 16 dB, the same in the oracle)
    d.close()


def test_decoder_soak_slice(amd):
    """2000 payloads of scripts/experiments/decoder_soak.py's eight kinds (real coded frames at three noise levels, pure
    noise, few-level inputs full of trellis ties, scales around the drop threshold, huge scales, sparse zeros) through
    opv_decode_payloads: metric, quantised taps, deinterleaved taps, 1072 Viterbi bits and 134 bytes equal the oracle's
    FrameDecoder for every one (ref src/opv-demod.cpp:800-898; tie rule :829, first-minimum end state :835-837)."""
    from concurrent.futures import ProcessPoolExecutor
    from soak_inputs import decoder_payloads, host_workers, oracle_decode_chunk
    N = 2000
    soft = decoder_payloads(N, int(os.environ.get("OPV_FUZZ_BASE", "20261003")) % 1000 + 7)
    d = amd.Demod(1, max_samples=1 << 20)
    r = d.decode_payloads(soft, taps=True)
    d.close()
    W = host_workers()
    with ProcessPoolExecutor(W) as ex:
        exp = [e for part in ex.map(oracle_decode_chunk, np.array_split(soft, W * 4)) for e in part]
    dropped = 0
    for k, e in enumerate(exp):
        assert r["metrics"][k] == e["metric"], (k, k % 8)
        if e["metric"] < 0:
            dropped += 1
            continue
        assert np.array_equal(r["q"][k], e["q"]) and np.array_equal(r["deint"][k], e["deint"]), (k, k % 8)
        assert np.array_equal(r["bits"][k], e["bits"]) and np.array_equal(r["frames"][k], e["frame"]), (k, k % 8)
    assert 0 < dropped < N // 8                                  # the drop threshold was on both sides of some payloads


def test_offset_soak_slice(amd):
    """128 openings of scripts/experiments/offset_soak.py (random start, carrier offset in and beyond the search span, level,
    0 dB to clean, 3000..45000 samples, noise only, silence with a burst) in one batch-mode context: estimate_offset EQUAL to
    the oracle's for every one (ref src/opv-demod.cpp:131-202)."""
    from concurrent.futures import ProcessPoolExecutor
    from soak_inputs import host_workers, offset_openings, oracle_offset_chunk
    S = 128
    caps = offset_openings(int(os.environ.get("OPV_FUZZ_BASE", "20261003")) % 1000 + 11, S)
    d = amd.Demod(S, max_samples=46000, streaming=False)
    d.receive(caps)
    got = [d.state(k) for k in range(S)]
    d.close()
    W = host_workers()
    with ProcessPoolExecutor(W) as ex:
        res = list(ex.map(oracle_offset_chunk, [caps[i::W] for i in range(W)]))
    exp = [None] * S
    for i, part in enumerate(res):
        exp[i::W] = part
    for k in range(S):
        assert got[k].est_offset_hz == exp[k], (k, caps[k].size // 2, got[k].est_offset_hz, exp[k], got[k].offset_ties)


def test_pathological_inputs_match_the_oracle(amd, oracle, iq10):
    """Inputs nobody promised to be an OPV signal: full-scale noise (int16 clipping), DC, a constant
    carrier on one tone, alternating extremes, silence with a burst in the middle, a signal that
    stops and resumes. No faults, no hangs, and the same frames / events / soft symbols as the oracle."""
    caps = pathological_captures(iq10)          # (shared with tests/test_gpu_mapping_matrix.py)
    n = caps[0].size // 2
    assert len(caps) == 8 and n == 3 * 86720 + 12345
    d = amd.Demod(len(caps), max_samples=n + 64, streaming=True)
    got = d.receive(caps)
    d.close()
    for k, x in enumerate(caps):
        exp = oracle.receive(x, streaming=True)
        assert np.array_equal(got[k]["frames"], exp["frames"]), k
        assert np.array_equal(got[k]["meta"]["viterbi_metric"], exp["metrics"]), k
        events_match(amd, got[k]["events"], exp["events"])
        assert got[k]["state"].total_symbols == exp["n_soft"], k
        scale = np.mean(np.abs(exp["soft"])) + 1e-300
        assert np.max(np.abs(got[k]["soft"] - exp["soft"])) / scale < 1e-8, k
        e0, e1 = got[k]["state"].est_offset_hz, exp["est_offset"]
        assert e0 == e1, (k, e0, e1)
    # batch mode on two of them
    for k in (0, 4):
        d = amd.Demod(1, max_samples=n + 64, streaming=False)
        g = d.receive([caps[k]])[0]
        exp = oracle.receive(caps[k], streaming=False)
        assert np.array_equal(g["frames"], exp["frames"]) and g["state"].total_symbols == exp["n_soft"], k
        d.close()


@pytest.mark.gpu
def test_many_silence_gaps_signed_zero_rule(amd, oracle, iq10):
    """Hundreds of digital-silence gaps inside a capture that sits 1.2 kHz off tune: every gap edge
    makes the reference's phase detector take std::arg of an exact zero, whose value (0 or pi, a
    27 Hz step of the AFC) depends on the signs of zeros and so on the ABSOLUTE LO phase the
    reference carries (k_frontend's silence rule, rebuilt from the running sum of fo). One wrong
    decision shows up in the per-chunk AFC state and in every soft symbol after it.

    Not comparable, and kept out of the capture: a symbol whose window holds ONE non-zero tap next
    to silence. Both tone energies are then |s|^2 exactly, and the reference's `e1 > e2` is decided
    by the rounding of its own cos^2+sin^2 (the oracle shows soft = -/+2^-31 there); no
    implementation that does not replay the reference's LO bit for bit can follow that coin toss.
    In batch mode (another timing trajectory) the comparison stops at the first such symbol."""
    x, starts = _gapped_capture(oracle, iq10)
    assert len(starts) > 250
    for streaming in (True, False):
        exp = oracle.receive(x, streaming=streaming)
        amb = np.nonzero((exp["soft"] != 0) & (np.abs(exp["soft"]) < 1.0))[0]
        k_end = int(amb[0]) if amb.size else exp["n_soft"]
        covered = sum(1 for p in starts if p < 38 * k_end)
        assert covered > (250 if streaming else 20), (k_end, covered)
        d = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=streaming)
        g = d.receive([x])[0]
        d.close()
        assert g["state"].total_symbols == exp["n_soft"]
        assert g["chunks"].shape == exp["chunks"].shape
        scale = np.mean(np.abs(exp["soft"])) + 1e-300
        assert np.max(np.abs(g["soft"][:k_end] - exp["soft"][:k_end])) / scale < 1e-8
        # freq_offset, timing_freq, mu, leftover, symbols of every demodulate() call that ended before k_end
        done = np.nonzero(np.cumsum(exp["chunks"][:, 4]) <= k_end)[0]
        if streaming:
            assert done.size >= 10
        for c in done:
            assert np.allclose(g["chunks"][c], exp["chunks"][c], rtol=0, atol=1e-7), (c, g["chunks"][c], exp["chunks"][c])
        # one-tap windows whose two energies happen to round EQUAL in the reference (soft exactly 0, tone 2 by '>') are
        # invisible to the nudging above and harmless when the product rounds the same way - as the equal soft symbols and
        # chunk states just asserted show; the product still counts them (a handful in ~600 gap edges)
        print(f"streaming={streaming}: edge_ties counted on the nudged capture: {g['state'].edge_ties}")
        assert g["state"].edge_ties <= 12


def test_one_tap_windows_are_counted(amd, oracle, iq10):
    """The input class the product cannot follow bit for bit is REPORTED, not hidden: with the gap edges left
    where the random generator put them, some symbol windows hold exactly one non-zero tap (the oracle shows
    soft = -/+2^-31 there: the reference's tone choice is its own LO rounding). The product must (a) agree
    with the oracle on every soft symbol before the first such window, (b) count these windows in
    opv_stream_state.edge_ties - at least as many as the oracle shows up to the point where the two AFC
    trajectories may part - on all three stream-to-wave mappings (one, four and sixteen streams per wave)."""
    x, starts = _gapped_capture(oracle, iq10, nudge=False)
    exp = oracle.receive(x, streaming=True)
    amb = np.nonzero((exp["soft"] != 0) & (np.abs(exp["soft"]) < 1.0))[0]
    assert amb.size >= 1, "the un-nudged capture was expected to contain one-tap windows"
    k_end = int(amb[0])
    scale = np.mean(np.abs(exp["soft"])) + 1e-300
    for frontend in (1, 4, 16):
        d = amd.Demod(1, max_samples=x.size // 2 + 64, streaming=True)
        d.set_frontend(frontend)
        g = d.receive([x])[0]
        d.close()
        assert g["state"].total_symbols == exp["n_soft"]
        assert np.max(np.abs(g["soft"][:k_end] - exp["soft"][:k_end])) / scale < 1e-8
        ties = g["state"].edge_ties
        print(f"x{frontend}: oracle shows {amb.size} one-tap windows (first at symbol {k_end}), product counted {ties}")
        assert ties >= 1


def test_host_cli_process_contract(amd, golden, iq10):
    """bin/opv-demod is a drop-in for the reference binary on BASELINE configs[0]: same stdout bytes, same
    stderr TEXT (banner, offset line, tracker lines, frame boxes, summary), same exit status; `-s -c`
    only swaps the banner (reference :983-984, the -s path ignores -c); batch `-c` runs the Costas-loop kernel
    and prints the reference's extra line (prefix parity of its soft symbols: test_coherent_prefix_parity)."""
    import subprocess
    arrays, meta = golden
    exe = str(ROOT / "opv-cxx-demod_amd" / "bin" / "opv-demod")
    g = ROOT / "tests" / "golden"
    raw = iq10.tobytes()
    for args, frames_key, text in ((["-s", "-r"], "c1_stream_frames", "c1_stream_stderr.txt"),
                                   (["-r"], "c1_batch_frames", "c1_batch_stderr.txt"),
                                   (["-s", "-c", "-r"], "c1_stream_frames", "c1_stream_coherent_flag_stderr.txt")):
        p = subprocess.run([exe] + args, input=raw, capture_output=True, timeout=300)
        assert p.returncode == 0, p.stderr.decode()[-400:]
        assert p.stdout == arrays[frames_key].tobytes(), args
        assert p.stderr.decode("utf-8") == (g / text).read_text(), args
    p = subprocess.run([exe, "-s", "-r", "-q"], input=raw[: 4 * 50000], capture_output=True, timeout=300)
    assert p.returncode == 1 and p.stdout == b""                      # no frame decoded -> exit 1 (:1124)
    p = subprocess.run([exe, "-c", "-r", "-p", "50"], input=raw, capture_output=True, timeout=300)
    err = p.stderr.decode()
    assert p.returncode in (0, 1) and len(p.stdout) % FRAME_BYTES == 0
    assert (p.returncode == 0) == (len(p.stdout) > 0)                              # exit 0 iff a frame was decoded (ref :1216)
    assert "Costas Loop v1.0 (coherent)" in err and "Estimated carrier offset: 1430.0 Hz\nPLL bandwidth: 50.0 Hz\n" in err
    assert "Demodulated 21780 symbols, final AFC offset: " in err                  # the reference's count (:462, :1173)


def test_host_cli_on_a_capture_whose_offset_search_ties(amd, oracle, iq10):
    """The tie decision in a plain C++ process (no Python, no torch: bin/opv-demod's own HIP runtime runs the host function): a
    capture that opens with 40 000 REAL-valued samples - mirrored search candidates tie exactly, the reference keeps the first
    maximum by its libm's last places - followed by the ten-frame BERT capture. `-s` and batch mode: the `Estimated carrier
    offset` line equals what the oracle's estimate_offset says, and stdout + the whole stderr text equal the compiled reference
    binary's where that travelled with the snapshot (oracle/_ref)."""
    import subprocess
    from oracle_lib import ref_binary
    exe = str(ROOT / "opv-cxx-demod_amd" / "bin" / "opv-demod")
    head = np.zeros(2 * 40000, np.int16)
    head[0::2] = np.rint(12000 * np.cos(2 * np.pi * 36000.0 * np.arange(40000) / 2168000.0 + 0.3))
    x = np.concatenate([head, iq10])
    ref = ref_binary("opv-demod")
    for args, streaming in ((["-s", "-r"], True), (["-r"], False)):
        off = oracle.estimate_offset(x[: 2 * 86720] if streaming else x)
        assert off in (-1530.0, 1530.0)                                   # the tied edge pair, dragged out by the fine pass
        p = subprocess.run([exe] + args, input=x.tobytes(), capture_output=True, timeout=300)
        err = p.stderr.decode()
        assert f"Estimated carrier offset: {off:.1f} Hz\n" in err, err[:600]
        if ref is not None:
            q = subprocess.run([str(ref)] + args, input=x.tobytes(), capture_output=True, timeout=300)
            assert p.returncode == q.returncode and p.stdout == q.stdout, args
            mine, theirs = err.splitlines(), q.stderr.decode().splitlines()
            assert len(mine) == len(theirs), args
            for a, b in zip(mine, theirs):                                # (text equal but for the licensed last digit of raw=)
                assert a == b or (a.split("raw=")[0] == b.split("raw=")[0] and "raw=" in a), (a, b)


def test_host_cli_small_staging_buffer_and_a_backlog(amd, oracle, iq100):
    """bin/opv-demod takes up to eight chunks per round when stdin has a backlog - but never more than its staging buffer
    holds: with --capacity-sec 0.15 (3.75 chunks) and with 0.09 (2.2 chunks: no batching at all) a 30-frame capture read from
    a file still comes out whole, frame for frame the oracle's."""
    import subprocess
    dem = str(ROOT / "opv-cxx-demod_amd" / "bin" / "opv-demod")
    x = iq100[: 2 * 86720 * 30]
    exp = oracle.receive(x, streaming=True, want_soft=False)["frames"]
    for cap in ("0.15", "0.09", "2"):
        p = subprocess.run([dem, "-s", "-r", "-q", "--capacity-sec", cap], input=x.tobytes(), capture_output=True, timeout=300)
        assert p.returncode == 0, (cap, p.stderr[-300:])
        assert p.stdout == exp.tobytes(), cap


def test_reference_makefile_targets_with_our_binaries():
    """The reference's own (and only) tests, run on the drop-in binaries: `make test` (Makefile:23-25: opv-mod -S W5NYV
    -B 5 | opv-demod -s, grep Station|Token|Summary) and `make test-raw` (Makefile:28-33: three hand-built frames through
    opv-mod -R | opv-demod -s -r must come back byte for byte - the one byte-exact KAT the reference repo holds)."""
    import subprocess
    mod = str(ROOT / "opv-cxx-demod_amd" / "bin" / "opv-mod")
    dem = str(ROOT / "opv-cxx-demod_amd" / "bin" / "opv-demod")
    iq = subprocess.run([mod, "-S", "W5NYV", "-B", "5"], capture_output=True, timeout=120).stdout
    p = subprocess.run([dem, "-s"], input=iq, capture_output=True, timeout=300)
    err = p.stderr.decode()
    assert p.returncode == 0
    assert err.count("Station ID:  W5NYV") == 5 and err.count("Token:       0xBBAADD (default)") == 5
    assert "Summary: 5 frames (5 perfect, 0 errors)" in err
    frames = b"".join(bytes([0, 0, 3, 0x74, 0x26, 0x97, 0xBB, 0xAA, 0xDD] + [0] * 3 + [(i + j) & 0xFF for j in range(122)]) for i in range(3))
    iq = subprocess.run([mod, "-R"], input=frames, capture_output=True, timeout=120).stdout
    p = subprocess.run([dem, "-s", "-r"], input=iq, capture_output=True, timeout=300)
    assert p.returncode == 0 and p.stdout == frames, "raw mode: the three frames did not come back byte for byte"


@pytest.mark.parametrize("seed", [int(os.environ.get("OPV_FUZZ_BASE", "20261003")) + k for k in range(int(os.environ.get("OPV_FUZZ_SEEDS", "8")))])
def test_clock_rate_error_and_random_channels_fuzz(amd, oracle, iq10, iq100, seed):
    """Differential fuzz: 24 streams in one context, each with its own sample-clock error (the timing
    loop then drifts through integer sample boundaries, the chunk grid moves: leftovers from 18 to 50), carrier offset, level, Eb/N0 and a random truncation point; both -s and batch mode."""
    caps = fuzz_captures(seed, iq10, iq100)
    nmax = max(c.size // 2 for c in caps)
    for streaming in (True, False):
        d = amd.Demod(len(caps), max_samples=nmax + 64, streaming=streaming)
        got = d.receive(caps)
        kinds = set()
        guarded = 0
        for k, x in enumerate(caps):
            exp = oracle.receive(x, streaming=streaming)
            # the offset search's near-tie guard may fire on a random channel (seed 777017, stream 11: two candidates): that
            # path is reproduced - check_stream compares the estimate with the oracle's - so it is counted, not forbidden
            check_stream(amd, got[k], exp, f"fuzz {k} streaming={streaming}", offset_ties=None)
            guarded += got[k]["state"].offset_ties != 0
            if streaming:
                kinds.update(int(v) for v in exp["chunks"][:-1, 3])
        d.close()
        assert guarded <= 2, f"the near-tie guard fired on {guarded} of {len(caps)} streams"
        if streaming:
            assert len(kinds) >= 8, kinds        # the clock error really moved the chunk grid (leftovers 18..50)


def test_channel_accidents(amd, oracle):
    """Captures with the accidents of a live channel (tests/oracle_lib.py::accidents: dropped / repeated samples, noise
    bursts, deep fades, carrier steps, stretches without a signal) on top of offset and AWGN: the tracker goes through
    MISS, flywheel, lost lock and re-acquisition, the timing loop through jumps - everything still equals the oracle, in -s
    and batch mode. (scripts/experiments/stream_soak.py is the long form: 24 streams a round.)"""
    from oracle_lib import accidents
    rng = np.random.default_rng(20261004)
    caps = []
    for k in range(8):
        base = oracle.modulate(oracle.bert_frames(int(rng.integers(6, 12)), "A%d" % k, first=40 * k))
        amp = float(rng.uniform(400, 8000))
        x = impair(base, amp=amp, f0_hz=float(rng.uniform(-1800, 1800)), ebn0_db=float(rng.uniform(10, 22)), seed=900 + k)
        caps.append(accidents(x, rng, amp)[0])
    nmax = max(c.size // 2 for c in caps)
    kinds = set()
    for streaming in (True, False):
        d = amd.Demod(len(caps), max_samples=nmax + 64, streaming=streaming)
        got = d.receive(caps)
        d.close()
        for k, x in enumerate(caps):
            exp = oracle.receive(x, streaming=streaming)
            check_stream(amd, got[k], exp, f"accidents {k} streaming={streaming}", offset_ties=None)
            kinds.update(int(v) for v in exp["events"]["kind"])
    assert {1, 2, 3, 4, 5} <= kinds, kinds               # acquisitions, locks, sync OK, misses and a lost lock all occurred


@pytest.mark.parametrize("order", [[0, 4, 1, 16, 1, 0], [16, 0, 4, 1, 4, 16]])
def test_mapping_switched_between_rounds(amd, oracle, order):
    """opv_set_frontend between two opv_process calls of running streams: every mapping reads and leaves the same per-stream
    carry (OpvStream), so a context may change its mapping at any round boundary - six noisy streams pushed in six pieces, a
    different kernel for each piece, the result the oracle's."""
    rng = np.random.default_rng(3)
    caps = [impair(oracle.modulate(oracle.bert_frames(10, "M%d" % k, first=k)), amp=float(rng.uniform(800, 6000)),
                   f0_hz=float(rng.uniform(-1500, 1500)), ebn0_db=float(rng.uniform(12, 20)), seed=50 + k) for k in range(6)]
    n = caps[0].size // 2
    cuts = [0, n // 6, n // 3, n // 2, 2 * n // 3, 5 * n // 6, n]
    d = amd.Demod(6, max_samples=n + 64, streaming=True)
    for i, m in enumerate(order):
        d.set_frontend(m)
        for k in range(6):
            d.push(k, caps[k][2 * cuts[i]: 2 * cuts[i + 1]])
        if i == len(order) - 1:
            for k in range(6):
                d.flush(k)
        d.process()
        d.sync()
    for k in range(6):
        fr, meta = d.pop_frames(k)
        e = oracle.receive(caps[k], streaming=True)
        assert np.array_equal(fr, e["frames"]) and np.array_equal(meta["viterbi_metric"], e["metrics"]), k
        assert np.array_equal(meta["release_symbol"], e["frame_sym"]) and d.state(k).total_symbols == e["n_soft"], k
        a, _ = soft_err(d.soft(k), e["soft"])
        assert a < SOFT_TIGHT, (k, a)
    d.close()


@pytest.mark.parametrize("spw", [4, 16])
def test_several_streams_per_wave_mappings(amd, oracle, iq10, iq100, spw):
    """k_msk_frontend_x4_wg4 (four streams per wavefront, the mapping the shim picks from 2049 streams) and k_msk_frontend_x16 / _x16_wg4
    (sixteen per wavefront, one per DPP quad: from 8193 streams) on the cases that exercise their per-row machinery: rows with
    different chunk schedules (clock error, truncation), idle rows (stream count not a multiple of 4 / 16), the first-symbol
    early-gate clamp, the end-of-capture partial block, digital-silence gaps, batch mode, incremental pushes."""
    rng = np.random.default_rng(4)
    caps = [iq10, iq10[: 2 * 91022], iq100[: 2 * 86720 * 12]]
    for k in range(10):
        ppm = float(rng.choice([-300.0, -40.0, 0.0, 25.0, 180.0]))
        x = resample_clock(iq10, ppm) if ppm else iq10
        x = impair(x, amp=float(rng.uniform(400, 8000)), f0_hz=float(rng.uniform(-2100, 2100)),
                   ebn0_db=float(rng.uniform(9, 22)), seed=300 + k)
        caps.append(x[: 2 * int(rng.integers(x.size // 4, x.size // 2))] if k % 3 == 0 else x)
    gapped, _ = _gapped_capture(oracle, iq10)
    assert len(caps) % 4 == 1
    nmax = max(c.size // 2 for c in caps + [gapped])
    for streaming in (True, False):
        d = amd.Demod(len(caps), max_samples=nmax + 64, streaming=streaming)
        d.set_frontend(spw)
        got = d.receive(caps)
        assert d.frontend_kernel() == {4: "k_msk_frontend_x4_wg4", 16: "k_msk_frontend_x16"}[spw]   # 13 streams: sixteen per wave = ONE wave
        for k, x in enumerate(caps):
            check_stream(amd, got[k], oracle.receive(x, streaming=streaming), f"x{spw} stream {k} streaming={streaming}")
        d.close()
    # silence gaps (signed-zero rule of the phase detector), streaming
    exp = oracle.receive(gapped, streaming=True)
    d = amd.Demod(2, max_samples=nmax + 64, streaming=True)
    d.set_frontend(spw)
    g = d.receive([gapped, iq10])
    d.close()
    assert g[0]["state"].total_symbols == exp["n_soft"]
    scale = np.mean(np.abs(exp["soft"]))
    assert np.max(np.abs(g[0]["soft"] - exp["soft"])) / scale < 1e-8
    assert np.allclose(g[0]["chunks"], exp["chunks"], rtol=0, atol=1e-7)
    # every tail length mod 4 and mod 40 (partial 16-byte piece at the end of the capture)
    lens = list(range(91003, 91048))
    d = amd.Demod(len(lens), max_samples=100000, streaming=True)
    d.set_frontend(spw)
    got = d.receive([iq10[: 2 * n] for n in lens])
    assert d.frontend_kernel() == {4: "k_msk_frontend_x4_wg4", 16: "k_msk_frontend_x16_wg4"}[spw]  # 45 streams
    d.close()
    for n, g1 in zip(lens, got):
        e = oracle.receive(iq10[: 2 * n], streaming=True)
        assert g1["state"].total_symbols == e["n_soft"], n
        a, _ = soft_err(g1["soft"], e["soft"])
        assert a < SOFT_TIGHT and np.allclose(g1["chunks"], e["chunks"], rtol=0, atol=1e-9), (n, a)
    # incremental pushes (opv-modem's 16 KB reads) through the x4 mapping, 5 streams
    d = amd.Demod(5, max_samples=iq10.size // 2 + 64, streaming=True)
    d.set_frontend(spw)
    step = 4096
    for a0 in range(0, iq10.size // 2, step):
        for s in range(5):
            d.push(s, iq10[2 * a0: 2 * min(a0 + step, iq10.size // 2)])
        if (a0 // step) % 7 == 0:
            d.process()
    for s in range(5):
        d.flush(s)
    d.process(); d.sync()
    exp = oracle.receive(iq10, streaming=True)
    for s in range(5):
        fr, meta = d.pop_frames(s)
        assert np.array_equal(fr, exp["frames"]) and np.array_equal(meta["release_symbol"], exp["frame_sym"])
        a, _ = soft_err(d.soft(s), exp["soft"])
        assert a < SOFT_TIGHT
    d.close()


def test_push_batch_and_pooled_pops(amd, oracle, iq10):
    """A multi-stream server's round: opv_push_iq_batch (all copies enqueued, one wait) + pops served from
    the once-per-round host copy of the record pools; 12 streams, ragged block sizes, a pop every round."""
    caps = [impair(iq10, amp=2500.0, f0_hz=-1800.0 + 300.0 * k, ebn0_db=15.0, seed=40 + k) for k in range(11)] + [iq10]
    S = len(caps)
    d = amd.Demod(S, max_samples=iq10.size // 2 + 64, streaming=True)
    sizes = [30011, 86720, 4096, 123457]
    at = [0] * S
    frames = [[] for _ in range(S)]
    events = [[] for _ in range(S)]
    r = 0
    while any(a < c.size // 2 for a, c in zip(at, caps)):
        ids, blks = [], []
        for k in range(S):
            n = min(sizes[(r + k) % 4], caps[k].size // 2 - at[k])
            if n > 0:
                ids.append(k); blks.append(caps[k][2 * at[k]: 2 * (at[k] + n)]); at[k] += n
        d.push_batch(ids, blks)
        d.process()
        for k in range(S):
            fr, meta = d.pop_frames(k)
            frames[k].append((fr, meta))
            events[k].append(d.pop_events(k))
        r += 1
    for k in range(S):
        d.flush(k)
    d.process()
    for k in range(S):
        fr, meta = d.pop_frames(k)
        frames[k].append((fr, meta))
        events[k].append(d.pop_events(k))
        exp = oracle.receive(caps[k], streaming=True)
        got_fr = np.concatenate([f for f, _ in frames[k]])
        got_meta = np.concatenate([m for _, m in frames[k]])
        assert np.array_equal(got_fr, exp["frames"]), k
        assert np.array_equal(got_meta["viterbi_metric"], exp["metrics"]) and np.array_equal(got_meta["release_symbol"], exp["frame_sym"]), k
        events_match(amd, np.concatenate(events[k]), exp["events"])
        a, _ = soft_err(d.soft(k), exp["soft"])
        assert a < SOFT_TIGHT, (k, a)
    d.close()


@pytest.mark.parametrize("mode", ["gather", "copies", "async"])
def test_push_batch_from_pinned_memory_and_batched_compaction(amd, oracle, iq10, iq100, mode, monkeypatch):
    """The serving path's bulk moves (csrc/opv_push.hip: k_push_gather, k_compact). Blocks that lie in PINNED host memory cross
    PCIe through one gather kernel per opv_push_iq_batch (read through their device-visible addresses) instead of one copy per
    stream, and staging buffers that fill in the same round are compacted by one launch. 14 streams with a staging buffer of
    about three chunks (so every stream compacts every few rounds, most of them together), blocks of ragged sizes: 16-byte
    aligned ones, ones starting one, two or three samples into a quad (4-byte moves), lengths that are no multiple of four
    samples, a stream with two blocks in one batch, a block from PAGEABLE memory in the same batch (takes hipMemcpyAsync), and
    a stream whose second block of a batch forces its own compaction. mode "copies" (OPV_PUSH_NO_GATHER) runs the same rounds
    over the per-stream copies; mode "async" enqueues every batch with opv_push_iq_batch_async and calls opv_process BEFORE
    opv_push_wait (the kernels must queue behind the moves on the device). Every stream's frames, metrics, sync positions, tracker lines and soft symbols equal the oracle's."""
    import torch
    if mode == "copies":
        monkeypatch.setenv("OPV_PUSH_NO_GATHER", "1")
    caps = [impair(iq100[: 2 * 86720 * 30], amp=2500.0, f0_hz=-1500.0 + 230.0 * k, ebn0_db=15.0, seed=70 + k) for k in range(12)]
    caps += [iq100[: 2 * 86720 * 30].copy(), iq10.copy()]
    S = len(caps)
    pinned = []
    for k, x in enumerate(caps):                                   # every capture in its own pinned buffer, at a sample offset 0..3
        t = torch.empty(x.size + 8, dtype=torch.int16).pin_memory()
        v = t.numpy()[2 * (k % 4): 2 * (k % 4) + x.size]
        v[:] = x
        pinned.append((t, v))
    d = amd.Demod(S, max_samples=3 * 86720 + 20000, streaming=True)
    sizes = [86720, 40001, 86720, 130002, 86723, 4096]
    at = [0] * S
    frames = [[] for _ in range(S)]
    events = [[] for _ in range(S)]
    soft = [[] for _ in range(S)]
    r = 0
    while any(a < c.size // 2 for a, c in zip(at, caps)):
        ids, blks = [], []
        for k in range(S):
            for part in range(2 if k == 5 else 1):                 # stream 5: two blocks per batch
                n = min(sizes[(r + k + part) % len(sizes)] // (2 if k == 5 else 1), caps[k].size // 2 - at[k])
                if n > 0:
                    src = pinned[k][1] if not (k == 7 and r % 3 == 1) else caps[k]       # stream 7: every third round from pageable memory
                    ids.append(k); blks.append(src[2 * at[k]: 2 * (at[k] + n)]); at[k] += n
        if mode == "async":
            d.push_batch(ids, blks, wait=False)
            d.process()
            d.push_wait()
        else:
            d.push_batch(ids, blks)
            d.process()
        for k in range(S):
            fr, meta = d.pop_frames(k)
            frames[k].append((fr, meta))
            events[k].append(d.pop_events(k))
            st = d.state(k)
            done = sum(len(x) for x in soft[k])
            if st.total_symbols > done:
                soft[k].append(d.soft(k, first=done, cap=int(st.total_symbols - done)))
        r += 1
    for k in range(S):
        d.flush(k)
    d.process()
    for k in range(S):
        fr, meta = d.pop_frames(k)
        frames[k].append((fr, meta))
        events[k].append(d.pop_events(k))
        st = d.state(k)
        done = sum(len(x) for x in soft[k])
        if st.total_symbols > done:
            soft[k].append(d.soft(k, first=done, cap=int(st.total_symbols - done)))
        exp = oracle.receive(caps[k], streaming=True)
        got_fr = np.concatenate([f for f, _ in frames[k]])
        got_meta = np.concatenate([m for _, m in frames[k]])
        assert np.array_equal(got_fr, exp["frames"]), (k, len(got_fr), len(exp["frames"]))
        assert np.array_equal(got_meta["viterbi_metric"], exp["metrics"]) and np.array_equal(got_meta["release_symbol"], exp["frame_sym"]), k
        events_match(amd, np.concatenate(events[k]), exp["events"])
        assert st.total_symbols == exp["n_soft"], k
        a, _ = soft_err(np.concatenate(soft[k]), exp["soft"])
        assert a < SOFT_TIGHT, (k, a)
    d.close()


def test_push_batch_of_tiny_pinned_blocks(amd, oracle, iq10):
    """the gather route's slicing at its small end: two streams fed from pinned memory in batches whose LARGEST block is 1, 3, 17,
    255, 1000, 4097 ... samples (fewer bytes than one 16-byte move per lane of a block), then the rest; frames and soft symbols
    equal the oracle's"""
    import torch
    caps = [iq10.copy(), impair(iq10, amp=3000.0, f0_hz=400.0, ebn0_db=17.0, seed=5)]
    pinned = []
    for x in caps:
        t = torch.empty(x.size, dtype=torch.int16).pin_memory()
        t.numpy()[:] = x
        pinned.append(t)
    d = amd.Demod(2, max_samples=iq10.size // 2 + 64, streaming=True)
    at = 0
    n_all = iq10.size // 2
    for n in [1, 3, 17, 255, 1000, 4097, 86720, 5, 50000]:
        d.push_batch([0, 1], [pinned[k].numpy()[2 * at: 2 * (at + n)] for k in range(2)])
        d.process()
        at += n
    d.push_batch([0, 1], [pinned[k].numpy()[2 * at:] for k in range(2)])
    for k in range(2):
        d.flush(k)
    d.process()
    for k in range(2):
        exp = oracle.receive(caps[k], streaming=True)
        fr, meta = d.pop_frames(k)
        assert np.array_equal(fr, exp["frames"]) and np.array_equal(meta["viterbi_metric"], exp["metrics"]), k
        a, _ = soft_err(d.soft(k), exp["soft"])
        assert a < SOFT_TIGHT and d.state(k).total_symbols == exp["n_soft"], (k, a)
    d.close()


def test_device_clock_error_tool(amd, oracle, iq10):
    """the device channel chain with a sample-clock error. opv_resample_device is bit-identical
    to the numpy model the CPU-side tests use; modulate -> resample -> channel -> receive stays in HBM and the
    receiver's output on those captures equals the oracle's on the same bytes."""
    import torch
    dev = torch.device("cuda", 0)
    n = iq10.size // 2
    d_in = torch.from_numpy(iq10).to(dev)
    d = amd.Demod(4, max_samples=n + 4096, streaming=True)
    caps = []
    for ppm in (-350.0, -20.0, 45.0, 700.0):
        d_rs = torch.zeros(2 * (n + 2048), dtype=torch.int16, device=dev)
        n_out = d.resample(d_in.data_ptr(), n, d_rs.data_ptr(), n + 2048, ppm)
        d.sync()
        model = resample_clock(iq10, ppm)
        assert n_out == model.size // 2
        assert np.array_equal(d_rs[: 2 * n_out].cpu().numpy(), model), ppm     # same operations, same order
        n4 = n_out & ~3
        d_ch = torch.empty(2 * n4, dtype=torch.int16, device=dev)
        d.channel(d_rs.data_ptr(), d_ch.data_ptr(), n4, gain=0.2, f0_hz=123.0 * ppm / 45.0, sigma=300.0, seed=int(1000 + ppm))
        d.sync()
        caps.append(d_ch)
    for k, c in enumerate(caps):
        d.attach(k, c.data_ptr(), c.numel() // 2, eof=True)
    d.process()
    d.sync()
    for k, c in enumerate(caps):
        x = c.cpu().numpy()
        exp = oracle.receive(x, streaming=True)
        fr, meta = d.pop_frames(k)
        assert np.array_equal(fr, exp["frames"]) and len(fr) >= 9, k
        assert np.array_equal(meta["viterbi_metric"], exp["metrics"]) and np.array_equal(meta["release_symbol"], exp["frame_sym"]), k
        a, _ = soft_err(d.soft(k), exp["soft"])
        assert a < SOFT_TIGHT, (k, a)
    d.close()


def test_device_channel_matches_cpu_model(amd, iq10):
    """k_channel against its CPU model (tests/oracle_lib.py::channel_model), element by element.
    The hash and the uniforms are integer-exact; the int16 output may differ by ONE LSB where device logf /
    sincospif / sincospi and numpy's disagree in the last place and the value sits on a rounding boundary - counted,
    bounded, never more than 1. Plus the properties the BER curve rests on: sigma, sign of f0, whiteness."""
    import torch
    dev = torch.device("cuda", 0)
    n = (iq10.size // 2) & ~3
    x = iq10[: 2 * n]
    d_in = torch.from_numpy(x).to(dev)
    d_out = torch.empty_like(d_in)
    d = amd.Demod(1, max_samples=1 << 20)
    for gain, f0, sigma, seed in ((2000.0 / 16383.0, 700.0, 0.0, 1), (2000.0 / 16383.0, -1500.0, 634.0, 1000),
                                  (1.0, 0.0, 2518.0, 77), (0.3, 54200.0, 50.0, 2 ** 63 + 5), (2.5, 1999.5, 4000.0, 3)):
        d.channel(d_in.data_ptr(), d_out.data_ptr(), n, gain=gain, f0_hz=f0, sigma=sigma, seed=seed)
        d.sync()
        got = d_out.cpu().numpy().astype(np.int32)
        model = channel_model(x, gain=gain, f0_hz=f0, sigma=sigma, seed=seed).astype(np.int32)
        diff = np.abs(got - model)
        nd = int(np.count_nonzero(diff))
        print(f"k_channel gain={gain:.3f} f0={f0} sigma={sigma} seed={seed}: {nd} of {diff.size} int16 values differ from the CPU model (max {diff.max()})")
        assert diff.max() <= 1
        assert nd <= max(4, diff.size // 2000), "more than 0.05 % of the samples differ from the CPU model"
    # sigma and whiteness: noise-only output of a zero input
    d_zero = torch.zeros_like(d_in)
    d.channel(d_zero.data_ptr(), d_out.data_ptr(), n, gain=1.0, f0_hz=0.0, sigma=500.0, seed=9)
    d.sync()
    w = d_out.cpu().numpy().astype(np.float64)
    wi, wq = w[0::2], w[1::2]
    assert abs(wi.std() / 500.0 - 1.0) < 0.01 and abs(wq.std() / 500.0 - 1.0) < 0.01, (wi.std(), wq.std())
    assert abs(wi.mean()) < 3.0 and abs(wq.mean()) < 3.0
    assert abs(np.corrcoef(wi, wq)[0, 1]) < 0.01 and abs(np.corrcoef(wi[:-1], wi[1:])[0, 1]) < 0.01
    assert abs(np.mean(wi ** 4) / wi.var() ** 2 - 3.0) < 0.1                      # Gaussian kurtosis
    # sign of f0: a DC input comes out as a tone at +f0
    d_dc = torch.zeros_like(d_in)
    d_dc[0::2] = 8000
    d.channel(d_dc.data_ptr(), d_out.data_ptr(), n, gain=1.0, f0_hz=13550.0, sigma=0.0, seed=0)
    d.sync()
    y = d_out.cpu().numpy().astype(np.float64)
    z = (y[0::2] + 1j * y[1::2])[:65536]
    k = int(np.argmax(np.abs(np.fft.fft(z))))
    assert abs(k * 2168000.0 / 65536 - 13550.0) < 2168000.0 / 65536, k          # positive frequency bin
    d.close()


@pytest.mark.parametrize("frontend", [1, 4, 16])
def test_every_tiny_tail_and_tiny_capture(amd, oracle, iq10, frontend):
    """Tail calls of 0, 1, 2, 3 symbols (one full chunk + 0..130 samples) in -s mode, and whole captures of
    30..300 samples in batch mode (offset search over a handful of symbols): every length, one stream each."""
    x = impair(iq10, amp=4000.0, f0_hz=650.0, ebn0_db=20.0, seed=21)
    lens = [86720 + r for r in range(0, 131)]
    d = amd.Demod(len(lens), max_samples=88000, streaming=True)
    d.set_frontend(frontend)
    got = d.receive([x[: 2 * n] for n in lens])
    d.close()
    for n, g in zip(lens, got):
        e = oracle.receive(x[: 2 * n], streaming=True)
        assert g["state"].total_symbols == e["n_soft"], n
        assert g["chunks"].shape == e["chunks"].shape and np.allclose(g["chunks"], e["chunks"], rtol=0, atol=1e-9), n
        a, _ = soft_err(g["soft"], e["soft"])
        assert a < SOFT_TIGHT, (n, a)
    lens = list(range(30, 301, 3))
    d = amd.Demod(len(lens), max_samples=1024, streaming=False)
    d.set_frontend(frontend)
    got = d.receive([x[: 2 * n] for n in lens])
    d.close()
    for n, g in zip(lens, got):
        e = oracle.receive(x[: 2 * n], streaming=False)
        assert g["state"].total_symbols == e["n_soft"], n
        assert g["state"].est_offset_hz == e["est_offset"], (n, g["state"].est_offset_hz, e["est_offset"])
        if e["n_soft"]:
            a, _ = soft_err(g["soft"], e["soft"])
            assert a < SOFT_TIGHT, (n, a)


@pytest.mark.parametrize("seed", list(range(1, 1 + int(os.environ.get("OPV_FUZZ_SEEDS", "8")))))
def test_random_call_sequences(amd, oracle, iq10, seed):
    """Randomised use of the boundary: pushes of random sizes to random streams (singly or batched), opv_process
    at random moments, pops of random streams in between, a staging buffer small enough to be compacted every
    few chunks. Odd seeds feed from PINNED host memory - batches then go through the gather kernel, a third of them through
    opv_push_iq_batch_async with whatever call comes next (another push, opv_process, a pop, a reset) left to settle or order
    it. Whatever the interleaving, each stream's frames, metadata and tracker events are the oracle's."""
    rng = np.random.default_rng(seed)
    S = 6
    caps = [impair(iq10, amp=float(rng.uniform(800, 6000)), f0_hz=float(rng.uniform(-1900, 1900)),
                   ebn0_db=float(rng.uniform(11, 22)), seed=seed * 50 + k) for k in range(S)]
    src = caps
    if seed % 2 == 1:
        import torch
        keep = [torch.from_numpy(np.ascontiguousarray(c)).pin_memory() for c in caps]
        src = [t.numpy() for t in keep]
    d = amd.Demod(S, max_samples=3 * 86720 + 70000, streaming=True)
    if seed % 3 == 0 and not os.environ.get("OPV_NO_X4"):
        d.set_frontend(4 if seed % 2 else 16)
    at = [0] * S
    frames = [[] for _ in range(S)]
    metas = [[] for _ in range(S)]
    events = [[] for _ in range(S)]
    since = [0] * S          # samples pushed to a stream since the last process (must stay within the staging buffer)
    unpopped = [0] * S       # samples pushed to a stream since its last pop

    def pop(k):
        fr, meta = d.pop_frames(k)
        frames[k].append(fr); metas[k].append(meta); events[k].append(d.pop_events(k))

    while any(a < c.size // 2 for a, c in zip(at, caps)):
        act = rng.integers(0, 10)
        if act < 6:
            ks = [int(k) for k in rng.choice(S, size=int(rng.integers(1, 4)), replace=False) if at[k] < caps[k].size // 2]
            ks = [k for k in ks if since[k] < 60000]
            if not ks:
                act = 7
            else:
                blks = []
                for k in ks:
                    n = int(min(rng.integers(1, 50000), caps[k].size // 2 - at[k], 60000 - since[k]))
                    blks.append(src[k][2 * at[k]: 2 * (at[k] + n)]); at[k] += n; since[k] += n; unpopped[k] += n
                if len(ks) == 1 and rng.integers(0, 2):
                    d.push(ks[0], blks[0])
                elif src is not caps and rng.integers(0, 3) == 0:
                    d.push_batch(ks, blks, wait=False)
                else:
                    d.push_batch(ks, blks)
        if act in (6, 7):
            d.process()
            since = [0] * S
            for k in range(S):                           # the frame ring holds 8 unread frames here: a stream that
                if unpopped[k] > 4 * 86720:              # has been fed >4 frames' worth since its last pop is popped
                    pop(k); unpopped[k] = 0
        elif act >= 8:
            k = int(rng.integers(0, S))
            if rng.integers(0, 12) == 0 and at[k] < caps[k].size // 2:
                d.reset(k)                               # start this stream over (a caller re-tuning a channel)
                at[k] = 0; since[k] = 0; unpopped[k] = 0
                frames[k].clear(); metas[k].clear(); events[k].clear()
            else:
                pop(k); unpopped[k] = 0
    for k in range(S):
        d.flush(k)
    d.process()
    for k in range(S):
        pop(k)
        exp = oracle.receive(caps[k], streaming=True)
        fr = np.concatenate(frames[k]); meta = np.concatenate(metas[k])
        assert np.array_equal(fr, exp["frames"]), (seed, k)
        assert np.array_equal(meta["viterbi_metric"], exp["metrics"]) and np.array_equal(meta["release_symbol"], exp["frame_sym"]), (seed, k)
        events_match(amd, np.concatenate(events[k]), exp["events"])
        assert d.state(k).total_symbols == exp["n_soft"]
    d.close()


def test_contexts_in_concurrent_host_threads(amd, oracle, iq10):
    """'A ctx is not thread-safe, distinct ctxs are independent' (include/opv_demod.h): four host threads, one
    context each, running at the same time (ctypes drops the GIL in the calls)."""
    import threading
    caps = [impair(iq10, amp=2000.0 + 500 * k, f0_hz=-900.0 + 600 * k, ebn0_db=16.0, seed=60 + k) for k in range(4)]
    exps = [oracle.receive(x, streaming=True) for x in caps]
    out = [None] * 4

    def work(k):
        try:
            for rep in range(3):
                d = amd.Demod(2, max_samples=iq10.size // 2 + 64, streaming=True)
                d.set_frontend(4 if k == 3 else 1)
                out[k] = d.receive([caps[k], caps[(k + 1) % 4]])
                d.close()
        except Exception as e:           # surfaces in the main thread below
            out[k] = e

    th = [threading.Thread(target=work, args=(k,)) for k in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for k in range(4):
        assert not isinstance(out[k], Exception), out[k]
        check_stream(amd, out[k][0], exps[k], f"thread {k} stream 0")
        check_stream(amd, out[k][1], exps[(k + 1) % 4], f"thread {k} stream 1")


def test_host_cli_irregular_pipe_writes(amd, golden, iq10):
    """stdin delivered in pieces that split samples (1, 3, 5, 4097, 65537 ... bytes) and with a trailing partial
    sample: the reader carries the split sample over (reference :1022 reads 4 bytes at a time) and ignores the
    incomplete one at EOF; output identical to the one-shot run."""
    import subprocess
    import threading
    arrays, _ = golden
    exe = str(ROOT / "opv-cxx-demod_amd" / "bin" / "opv-demod")
    raw = iq10.tobytes() + b"\x12\x34\x56"           # 3 stray bytes: an incomplete last sample
    rng = np.random.default_rng(8)
    for args, key in ((["-s", "-r", "-q"], "c1_stream_frames"), (["-r", "-q"], "c1_batch_frames")):
        p = subprocess.Popen([exe] + args, stdin=subprocess.PIPE, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL)

        def feed():
            pos = 0
            sizes = [1, 3, 5, 2, 4097, 65537, 7, 1048579, 13]
            i = 0
            while pos < len(raw):
                n = sizes[i % len(sizes)] if i < 40 else int(rng.integers(1, 300000))
                p.stdin.write(raw[pos: pos + n]); p.stdin.flush()
                pos += n; i += 1
            p.stdin.close()

        t = threading.Thread(target=feed)
        t.start()
        out = p.stdout.read()
        t.join()
        assert p.wait(timeout=120) == 0
        assert out == arrays[key].tobytes(), args
