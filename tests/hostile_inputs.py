"""Input recipes that more than one test module is built on, CPU only: the hostile capture set of tests/test_gpu_mapping_matrix.py
(with what makes it hostile, said by the oracle alone) and the captures and flag values of single tests of tests/test_gpu_parity.py.
The GPU modules hold the product to the ORACLE on these inputs; tests/test_oracle_pinned_live.py holds the oracle to the compiled
reference on the same ones. Nothing here needs a device, and one definition serves both sides. Test infrastructure: everything
comes from the CPU oracle's transmit chain and the numpy channel model (tests/oracle_lib.py)."""
from concurrent.futures import ProcessPoolExecutor
from functools import partial

import numpy as np

from oracle_lib import CHUNK_SAMPLES as CHUNK, accidents, format_events, impair, resample_clock
from soak_inputs import host_workers, oracle_receive_job, pathological_captures

LONG = "clamp+2600"     # the 30-frame capture of the hostile set: the one that keeps a push test running for >= 12 rounds


def gapped_capture(oracle, iq10, nudge=True):
    """10 frames, 1.2 kHz off tune, ~300 gaps of exact zeros. With nudge=True, gap edges that would leave a
    symbol window with ONE non-zero tap are moved until the oracle sees none (test_gpu_parity.py:
    test_many_silence_gaps_signed_zero_rule, test_one_tap_windows_are_counted)."""
    base = impair(iq10, amp=6000.0, f0_hz=1200.0).reshape(-1, 2)
    rng = np.random.default_rng(5)
    pos, gaps = 3000, []
    while pos + 400 < base.shape[0]:
        glen = int(rng.integers(105, 260))          # >= one whole 60-sample correlation window of zeros
        gaps.append([pos, glen])
        pos += glen + int(rng.integers(1500, 4000))

    def build():
        z = base.copy()
        for p, n in gaps:
            z[p:p + n] = 0
        return z.reshape(-1)

    if not nudge:
        return build(), [g[0] for g in gaps]
    for _ in range(200):
        x = build()
        soft = oracle.receive(x, streaming=True)["soft"]
        amb = np.nonzero((soft != 0) & (np.abs(soft) < 1.0))[0]            # energies are ~1e10
        if amb.size == 0:
            return x, [g[0] for g in gaps]
        at = 40 * int(amb[0])                                                # roughly the sample position
        j = int(np.argmin([min(abs(p - at), abs(p + n - at)) for p, n in gaps]))
        if abs(gaps[j][0] - at) < abs(gaps[j][0] + gaps[j][1] - at):
            gaps[j][0] -= 3; gaps[j][1] += 3                                 # leading edge 3 samples earlier
        else:
            gaps[j][1] += 3                                                  # trailing edge 3 samples later
    raise AssertionError("could not remove the tie symbols")


# ------------------------------------------------------------------ the hostile set (tests/test_gpu_mapping_matrix.py)
def slip_capture(iq10, ppm):
    """the 10-frame capture as an ADC `ppm` parts per million fast took it, 300 Hz low, 20 dB (test_timing_loop_slipping's recipe)"""
    return impair(resample_clock(iq10, ppm), amp=5000.0, f0_hz=-300.0, ebn0_db=20.0, seed=9)


def hostile_captures(oracle):
    """[(name, class, int16 IQ)]; class: "full" (check_stream), "patho" / "gap" (1e-8 + chunk log), "tie" (un-nudged gaps)"""
    iq10 = oracle.modulate(oracle.bert_frames(10))
    caps = [(f"patho{k}", "patho", x) for k, x in enumerate(pathological_captures(iq10))]
    for ppm in (-25000.0, -3000.0, 3000.0, 25000.0):                         # test_timing_loop_slipping's recipe
        caps.append((f"slip{ppm:+.0f}", "full", slip_capture(iq10, ppm)))
    rng = np.random.default_rng(20261004)                                     # test_channel_accidents' recipe (its captures 0, 5, 6, 7)
    for k in range(8):
        base = oracle.modulate(oracle.bert_frames(int(rng.integers(6, 12)), "A%d" % k, first=40 * k))
        amp = float(rng.uniform(400, 8000))
        x = impair(base, amp=amp, f0_hz=float(rng.uniform(-1800, 1800)), ebn0_db=float(rng.uniform(10, 22)), seed=900 + k)
        x = accidents(x, rng, amp)[0]
        if k in (0, 5, 6, 7):
            caps.append((f"accident{k}", "full", x))
    caps.append(("gaps_nudged", "gap", gapped_capture(oracle, iq10)[0]))
    caps.append(("gaps_as_drawn", "tie", gapped_capture(oracle, iq10, nudge=False)[0]))
    caps.append((LONG, "full", impair(oracle.modulate(oracle.bert_frames(30, "CLAMP", first=7)), amp=3000.0, f0_hz=2600.0, ebn0_db=14.0, seed=41)))
    caps.append(("edge-1990", "full", impair(oracle.modulate(oracle.bert_frames(6, "EDGE", first=3)), amp=1500.0, f0_hz=-1990.0, ebn0_db=6.0, seed=42)))
    lsb = oracle.modulate(oracle.bert_frames(3, "LSB", first=11))
    caps.append(("lsb_2_chunks", "patho", (lsb[: 2 * 2 * CHUNK] // 4000).astype(np.int16)))      # 3-4 LSB, exactly two chunks
    caps.append(("short", "full", impair(iq10[: 2 * 900], amp=4000.0, f0_hz=250.0, ebn0_db=16.0, seed=43)))     # 22 symbols
    # ordinary 16 dB captures: (frames, f0, amplitude, cut in samples or None)
    for k, (F, f0, amp, cut) in enumerate([(1, 700.0, 2000.0, 50000), (5, -1100.0, 900.0, 4 * CHUNK), (3, 1500.0, 6000.0, None),
                                           (5, -250.0, 12000.0, None), (8, 1900.0, 2500.0, None), (12, 40.0, 4000.0, None),
                                           (4, -1400.0, 700.0, None), (7, 900.0, 3000.0, 6 * CHUNK + 33333), (2, -1800.0, 8000.0, None),
                                           (9, -600.0, 5000.0, 3 * CHUNK - 1)]):
        x = impair(oracle.modulate(oracle.bert_frames(F, "H%d" % k, first=500 + 17 * k)), amp=amp, f0_hz=f0, ebn0_db=16.0, seed=600 + k)
        caps.append((f"ord{k}_{F}f", "full", x if cut is None else x[: 2 * cut]))
    return caps


def ambiguous(soft):
    """one-tap windows as the oracle shows them: soft = -/+2^-31 against energies of ~1e10"""
    return np.nonzero((soft != 0) & (np.abs(soft) < 1.0))[0]


def oracle_over(caps, streaming):
    with ProcessPoolExecutor(host_workers()) as pool:
        return list(pool.map(partial(oracle_receive_job, want_soft=True, streaming=streaming), caps))


def receive_pair_job(job):
    """job = (int16 IQ, keyword arguments of receive): one capture through the oracle AND the compiled reference (one object of
    each per worker process) -> (Oracle.receive's result, Reference.receive's)"""
    global _RECEIVE_PAIR
    try:
        o, r = _RECEIVE_PAIR
    except NameError:
        from oracle_lib import Oracle, Reference
        o, r = _RECEIVE_PAIR = Oracle(), Reference()
    x, kw = job
    return o.receive(x, **kw), r.receive(x, **kw)


def receive_pairs(jobs):
    """receive_pair_job over worker processes: the reference's tracker is driven symbol by symbol from Python, which is what a
    comparison of many captures waits for"""
    with ProcessPoolExecutor(host_workers()) as pool:
        return list(pool.map(receive_pair_job, jobs))


# ------------------------------------------------------------------ the oracle == the compiled reference (tests/test_oracle_pinned_live.py, tests/test_coherent_host.py)
def bits(x):
    return np.ascontiguousarray(x, np.float64).view(np.uint64)


def same_float(a, b):
    return bits(np.float64(a).reshape(1))[0] == bits(np.float64(b).reshape(1))[0]


def assert_same_receive(a, b, tag=""):
    """a: Oracle.receive (or soak_inputs.oracle_receive_job), b: Reference.receive of the same input - everything =="""
    assert a["soft"].shape == b["soft"].shape, f"{tag}: {a['soft'].shape[0]} soft symbols, the reference {b['soft'].shape[0]}"
    d = np.nonzero(bits(a["soft"]) != bits(b["soft"]))[0]
    assert d.size == 0, f"{tag}: {d.size} soft symbols differ, the first at {d[0]}: {a['soft'][d[0]]!r} vs {b['soft'][d[0]]!r}"
    assert np.array_equal(a["frames"], b["frames"]), f"{tag}: decoded bytes differ"
    assert np.array_equal(a["metrics"], b["metrics"]), f"{tag}: Viterbi metrics differ"
    assert np.array_equal(a["frame_sym"], b["frame_sym"]), f"{tag}: release symbols differ"
    assert format_events(a["events"]) == [ln for ln in b["log"].split("\n") if ln.startswith("[")], f"{tag}: tracker lines differ"
    ca, cb = a["chunks"][:, [0, 1, 3, 4]], b["chunks"][:, [0, 1, 3, 4]]          # (column 2, mu, is NaN on the reference side)
    assert ca.shape == cb.shape and np.array_equal(bits(ca), bits(cb)), f"{tag}: chunk log differs:\n{ca}\n{cb}"
    e0, e1 = a["est_offset"], b["est_offset"]
    assert (np.isnan(e0) and np.isnan(e1)) or e0 == e1, f"{tag}: offset estimate {e0} vs {e1}"
    assert same_float(a["final_freq_offset"], b["final_freq_offset"]), f"{tag}: {a['final_freq_offset']!r} vs {b['final_freq_offset']!r}"
    assert a["final_state"] == b["final_state"], tag


def assert_set_is_hostile(names, classes, caps, exp_s, exp_b):
    """what the set is FOR, said by the oracle alone before the product has seen an input"""
    n = [c.size // 2 for c in caps]
    assert 28 <= len(caps) <= 32 and min(n) < 24 * 40 and any(v < CHUNK for v in n) and any(v >= 12 * CHUNK for v in n)
    assert any(v % CHUNK == 0 for v in n), "an exact multiple of the chunk length belongs to the set"
    assert len(set(n)) >= 20, "mixed lengths"
    kinds = set(int(v) for e in exp_s for v in e["events"]["kind"])
    assert {1, 2, 3, 4, 5} <= kinds, kinds
    clamp = [(names[j], int(np.sum(np.abs(e["chunks"][:, 0]) == 2000.0))) for j, e in enumerate(exp_s)]
    assert any(c for _, c in clamp), "no demodulate() call ended with the AFC on its clamp"
    left = set(int(v) for e in exp_s for v in e["chunks"][:-1, 3])
    assert len(left) >= 8, left
    tie, gap = names.index("gaps_as_drawn"), names.index("gaps_nudged")
    assert ambiguous(exp_s[tie]["soft"]).size >= 1 and ambiguous(exp_s[gap]["soft"]).size == 0
    per = [len(e["frames"]) for e in exp_s]
    assert min(per) == 0 and max(per) >= 10, per
    for e in exp_s + exp_b:
        assert e["n_soft"] == len(e["soft"])
    tf = max(float(np.max(np.abs(e["chunks"][:, 1]))) for e in exp_s + exp_b if len(e["chunks"]))
    print(f"hostile set: {len(caps)} captures, {min(n)} .. {max(n)} samples; -s frames {sum(per)}; event kinds {sorted(kinds)}; calls ending on the "
          f"AFC clamp {[c for c in clamp if c[1]]}; leftovers {sorted(left)}; one-tap windows in the un-nudged capture "
          f"{ambiguous(exp_s[tie]['soft']).size}; largest |timing_freq| at a call boundary {tf:.1e}")


# ------------------------------------------------------------------ recipes of single tests of tests/test_gpu_parity.py
# test_extreme_flag_values: -o beyond the AFC clamp and -a so large that the loop slams into its clamp every symbol
EXTREME_FLAGS = [(6000.0, 0.001), (-2600.0, 0.001), (150000.0, 0.001), (300.0, 0.08), (0.0, 1.0), (-700.0, 0.0), (100.0, -0.01)]
AFC_ALPHA_FLAG = 0.01   # test_afc_alpha_flag, on the clean 10-frame capture


def extreme_flags_capture(iq10):
    return impair(iq10, amp=3000.0, f0_hz=400.0, ebn0_db=18.0, seed=77)


def near_tie_captures(iq10):
    """test_offset_search_near_tie_guard's eight one-chunk captures: real-valued ones whose mirrored offset candidates tie
    exactly, and two controls whose landscape peaks at 0"""
    rng = np.random.default_rng(2024)
    caps = []
    t = np.arange(86720)
    # real tones well outside the +/-13.55 kHz pair: two window main lobes 2 x 20..33 kHz apart add up to a landscape
    # that is convex at o = 0, so its maximum is the tied pair of edge candidates -1500 / +1500
    for f_hz, amp in ((33550.0, 9000.0), (36000.0, 20000.0), (42000.0, 3000.0), (47000.0, 12000.0)):
        x = np.zeros(2 * 86720, np.int16); x[0::2] = np.rint(amp * np.cos(2 * np.pi * f_hz * t / 2168000.0 + 0.3)); caps.append(x)
    x = np.zeros(2 * 86720, np.int16); x[0::2] = np.rint(8000 * np.cos(2 * np.pi * 33550.0 * t / 2168000.0) + 300 * rng.standard_normal(86720)); caps.append(x)
    x = np.zeros(2 * 86720, np.int16); x[0::2] = np.clip(np.rint(rng.standard_normal(86720) * 50), -32768, 32767); caps.append(x)   # real noise
    x = iq10[: 2 * 86720].copy(); x[1::2] = 0; caps.append(x)                       # I branch of the MSK capture: peak at 0, no tie
    x = np.zeros(2 * 86720, np.int16); x[0::2] = 12345; caps.append(x)              # DC: peak at 0, no tie
    return caps


def staged_ties_capture(n=4000):
    """test_more_ties_in_one_round_than_the_host_passes_stage's short real-valued capture: a convex, exactly symmetric landscape"""
    x = np.zeros(2 * n, np.int16)
    x[0::2] = np.rint(9000 * np.cos(2 * np.pi * 36000.0 * np.arange(n) / 2168000.0 + 0.3))
    return x


def fuzz_captures(seed, iq10, iq100):
    """test_clock_rate_error_and_random_channels_fuzz's 24 captures of one seed: each with its own sample-clock error, carrier
    offset, level, Eb/N0 and, one in four, a random truncation point"""
    rng = np.random.default_rng(seed)
    caps = []
    for k in range(24):
        base = iq100[: 2 * 86720 * 14] if k % 3 == 0 else iq10
        ppm = float(rng.choice([-400.0, -120.0, -35.0, 0.0, 7.0, 60.0, 250.0, 900.0]))
        x = resample_clock(base, ppm) if ppm else base
        x = impair(x, amp=float(rng.uniform(300, 9000)), f0_hz=float(rng.uniform(-2100, 2100)),
                   ebn0_db=float(rng.uniform(9, 24)), seed=seed % 1000 + k)
        cut = int(rng.integers(x.size // 4, x.size // 2)) if k % 4 == 1 else x.size // 2
        caps.append(x[: 2 * cut])
    return caps
