"""GPU: the wideband front door (opv_wb_*, csrc/k_wideband.hip + csrc/opv_wideband.hip). k_wb_ddc is integer-exact, so its outputs
are held to the numpy int64 model of tests/wideband_models.py with == on every sample (read back through opv_tap_iq), for any
split of a capture into pushes and any mix of pinned, pageable and device sources; and the streams it feeds are held to the ORACLE
run on the model's output, like every other pushed stream of the suite (stream_checks.check_stream: frames, metrics, release
symbols, tracker lines, chunk log ==, soft symbols < 1e-9).

The end-to-end plan (wideband_device.PLAN_D4) was chosen on the CPU so that the reference algorithm by itself decodes every transmitted frame
of the clean channels AND of the 12 dB channel from the model's output - the precondition the fixture asserts before the product
sees a sample:
  D = 4 (wide rate 8.672 MS/s), K = 4 slots at -1.1, 0.0, +1.6 and +2.7 MHz. A channel repeated by D (zero-order hold) has images at
  multiples of 2.168 MHz from its centre; these four centres keep every image >= 532 kHz from every other slot.
  Slots 0 and 2 carry clean channels (amplitude 3000, carrier offsets +1700 / -1900 Hz), slot 1 a channel at Eb/N0 = 12 dB through
  oracle_lib.impair (amplitude 1000, +600 Hz), slot 3 is left empty.
  Taps: 321-tap Hamming-windowed sinc, cut-off 200 kHz, scaled to sum 2^15; out_shift = 30 (the LO contributes 32767): unity gain.
  321 because the filter's delay, (L - 1) / 2 = 160 wide samples, is then exactly one symbol (40 samples at the stream's rate): the
  reference's timing loop starts on a symbol boundary, as it does on a capture of its own. With 143 taps (17.75 samples late, close
  to half a symbol: the loop's unstable point) it needs two clean frames to pull in and never does at 12 dB - the reference alone
  then released nothing on that slot within 2 frames, although it decodes the same channel directly.
The channels are made by the product's own transmit chain (amd.bert_frames / amd.modulate)."""
import numpy as np
import pytest

from fixtures import amd, torch_dev  # noqa: F401
from stream_checks import SOFT_TIGHT, events_match
from stream_runs import CHUNK
from wideband_device import (PLAN_D4, Sources, assert_exactness_preconditions, check_plan_streams_d4, exactness_inputs, make_plan_capture_d4,
                             plan_wideband_d4)
from wideband_models import WIDE_RATE, halved_taps, wb_model, wb_model_inc

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = -1, -4, -6


@pytest.fixture(scope="module")
def e2e(amd, oracle):
    return make_plan_capture_d4(amd, oracle, 2)


# ------------------------------------------------------------------ 1. exactness
CASES = {
    # name: (D, L, K, S, first_sample, n_wide, input)
    "D1_L1_K1_S0": (1, 1, 1, 0, 0, 1000, "small"),                       # S = 0: no rounding term; products of small inputs, unclamped
    "D3_L2_K5_wrap32": (3, 2, 5, 21, (1 << 32) - 1000, 3 * 700 + 1, "random"),   # the phase product wraps inside the capture
    "D4_L143_K33_wrap40": (4, 143, 33, 33, (1 << 40) + 7, 4 * 600 + 3, "random"),
    "D16_L1024_K5": (16, 1024, 5, 36, 0, 16 * 450 + 5, "random"),
    "D1_L143_K5_clamps": (1, 143, 5, 34, (1 << 32) - 1000, 2000, "fullscale"),   # full-scale input, tap gain 4: both clamps fire
    "D4_L2_K1_halfway": (4, 2, 1, 3, 0, 4 * 300, "halfway"),               # accumulators at negative half-way points
}


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_integer_model_on_every_sample(amd, torch_dev, case):
    """opv_wb_push_device in two pieces (the second starts inside a decimation period and needs the carry) into a scratch context that
    never runs opv_process; every stream's IQ read back with opv_tap_iq == the model, sample for sample."""
    D, L, K, S, first, N, kind = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T = amd.wb_lo_table()
    (wide,), taps, centres = exactness_inputs(kind, rng, "rx", D * WIDE_RATE, K, N, L, 1, halfway_taps=(1, 0))      # (one phase: the cap is on all taps)
    inc = amd.wb_plan(D, centres, taps, S, first)
    assert np.array_equal(inc, wb_model_inc(D, centres))
    exp = wb_model(T, wide, D, inc, taps, S, first)
    n_out = amd.wb_outputs(D, N)
    assert exp.shape == (K, 2 * n_out) and n_out > 256, "more than one workgroup of outputs"
    # halfway: channel 0 sits at centre 0: acc = 32767 x I. With S = 3 an accumulator is half-way when acc = 4 (mod 8), i.e. I = 4 (mod 8): I = -4
    assert_exactness_preconditions(kind, exp, halfway=(32767 * wide[0::2][::D].astype(np.int64), exp[0, 0::2]))
    if "wrap32" in case:
        assert first < (1 << 32) <= first + N
    d = amd.Demod(K, max_samples=n_out + 64, streaming=True)
    wb = amd.Wideband(d, D, list(range(K)), centres, taps, S, first)
    try:
        src = Sources(torch_dev, wide)
        cut = (N // 2) | 1 if D > 1 else N // 2
        assert D == 1 or cut % D
        src.push(wb, "device", 0, cut)
        src.push(wb, "device", cut, N)
        for k in range(K):
            got = d.iq(k)
            assert got.size == exp[k].size, (k, got.size, exp[k].size)
            bad = np.nonzero(got != exp[k])[0]
            assert bad.size == 0, f"{case}: channel {k}: {bad.size} of {got.size} values differ, first at {bad[0]}: {got[bad[0]]} vs {exp[k][bad[0]]}"
    finally:
        wb.close()
        d.close()


# ------------------------------------------------------------------ 2. any split equals one shot
def test_any_split_and_any_source_equals_one_shot(amd, torch_dev, e2e):
    """the plan's capture whole (pinned), and in pieces of 1, D - 1, D + 1, L - 2 and 40 001 wide samples taken in turn from pinned,
    pageable and device memory (5 sizes x 3 sources: every pair occurs): the streams' IQ == the model in both runs, and the frames,
    metrics, symbols and tracker lines of both == the oracle on the model's output"""
    D, L = PLAN_D4["D"], PLAN_D4["L"]
    wide = e2e["wide"]
    N = wide.size // 2
    src = Sources(torch_dev, wide)
    n_out = amd.wb_outputs(D, N)
    pieces, kinds = [1, D - 1, D + 1, L - 2, 40001], ["pinned", "pageable", "device"]
    for split in (False, True):
        d = amd.Demod(len(PLAN_D4["centres"]), max_samples=n_out + 64, streaming=True)
        wb = plan_wideband_d4(amd, d)
        try:
            if not split:
                src.push(wb, "pinned", 0, N)
            else:
                at = j = 0
                seen = set()
                while at < N:
                    m = min(pieces[j % 5], N - at)
                    src.push(wb, kinds[j % 3], at, at + m)
                    seen.add((pieces[j % 5], kinds[j % 3]))
                    at, j = at + m, j + 1
                assert len(seen) == 15 and j > 45
            for k in range(len(PLAN_D4["centres"])):
                assert np.array_equal(d.iq(k), e2e["model"][k]), (split, k)
            wb.flush()
            d.process()
            d.sync()
            check_plan_streams_d4(amd, d, e2e, "split" if split else "one shot")
        finally:
            wb.close()
            d.close()


# ------------------------------------------------------------------ 3. + 4. end to end against the oracle, on every mapping
@pytest.mark.parametrize("streams_per_wave", [0, 1, 4, 16])
def test_end_to_end_against_the_oracle_on_every_mapping(amd, e2e, streams_per_wave):
    """K channels modulated with the product's transmit chain, offsets within +/-2 kHz, one at
    12 dB, one slot empty; each stream's frames, metrics, release symbols, tracker lines and chunk log == Oracle().receive(model
    output), soft symbols < 1e-9 - with the context on its automatic mapping and forced to 1, 4 and 16 streams per wave."""
    N = e2e["wide"].size // 2
    d = amd.Demod(len(PLAN_D4["centres"]), max_samples=amd.wb_outputs(PLAN_D4["D"], N) + 64, streaming=True)
    wb = plan_wideband_d4(amd, d)
    try:
        if streams_per_wave:
            d.set_frontend(streams_per_wave)
        wb.push(e2e["wide"])
        wb.flush()
        d.process()
        d.sync()
        check_plan_streams_d4(amd, d, e2e, f"mapping {streams_per_wave}")
        for k in PLAN_D4["channels"]:
            fr = d.pop_frames(k)[0]
            assert len(fr) == 0                                              # (check_plan_streams_d4 popped them: == the oracle's == tx)
    finally:
        wb.close()
        d.close()


# ------------------------------------------------------------------ 5. long run through small buffers
def test_long_run_through_small_buffers(amd, oracle, torch_dev):
    """12 frames per channel through a context whose buffers hold 3 chunks + one push: a push, opv_process and a pop per round, so that
    every stream's buffer is compacted several times (seen through opv_tap_iq: the samples in front of the keep point are gone). The
    IQ that is still retained == the model at its absolute indices after every round, and at the end everything == the oracle, the
    whole chunk log (read round by round) included."""
    cap = make_plan_capture_d4(amd, oracle, 12, empty_is_silent=False)      # (over 12 frames of leaked noise the reference's tracker false-alarms on the empty slot: the product must too)
    D, K = PLAN_D4["D"], len(PLAN_D4["centres"])
    N = cap["wide"].size // 2
    push_out = 30000
    src = Sources(torch_dev, cap["wide"])
    d = amd.Demod(K, max_samples=3 * CHUNK + push_out, streaming=True)
    wb = plan_wideband_d4(amd, d)
    try:
        frames = [[] for _ in range(K)]
        metas = [[] for _ in range(K)]
        events = [[] for _ in range(K)]
        chunks = [[] for _ in range(K)]
        base, compactions = [0] * K, [0] * K
        at = r = 0
        while at < N:
            m = min(push_out * D - (7 if r % 2 else 0), N - at)
            origin = [d.state(k).chunk_origin for k in range(K)]
            src.push(wb, ("pinned", "device", "pageable")[r % 3], at, at + m)
            at += m
            have = amd.wb_outputs(D, at)
            for k in range(K):
                if d.iq(k, first=base[k], cap=1).size == 0:                  # the sample at the old keep point is gone: compacted
                    compactions[k] += 1
                    base[k] = (origin[k] - 16) & ~3
                got = d.iq(k, first=base[k])
                assert np.array_equal(got, cap["model"][k][2 * base[k]: 2 * have]), (r, k, base[k], got.size // 2, have)
            if at == N:
                wb.flush()
            d.process()
            d.sync()
            for k in range(K):
                f, mt = d.pop_frames(k)
                frames[k].append(f)
                metas[k].append(mt)
                events[k].append(d.pop_events(k))
                chunks[k].append(d.chunks(k, first=sum(map(len, chunks[k]))))   # (the log is a ring: read what each round added)
            r += 1
        assert min(compactions) >= 3, compactions
        for k in PLAN_D4["channels"]:                                           # (the 12 dB slot included: the fixture holds the oracle to tx)
            assert len(cap["exp"][k]["frames"]) == 12
        for k, exp in enumerate(cap["exp"]):
            st = d.state(k)
            fr, meta, ev = np.concatenate(frames[k]), np.concatenate(metas[k]), np.concatenate(events[k])
            assert st.stalled == 0 and st.total_symbols == exp["n_soft"], (k, st.total_symbols, exp["n_soft"])
            assert np.array_equal(fr, exp["frames"]) and np.array_equal(meta["viterbi_metric"], exp["metrics"]), k
            assert np.array_equal(meta["release_symbol"], exp["frame_sym"]), k
            events_match(amd, ev, exp["events"])
            assert abs(st.freq_offset_hz - exp["final_freq_offset"]) < 1e-6 and st.sync_state == exp["final_state"], k
            log = np.concatenate(chunks[k])
            assert st.n_chunks == len(exp["chunks"]) == len(log) >= 12, k
            assert np.array_equal(log[:, 3:], exp["chunks"][:, 3:]), k          # leftover, symbols per call
            assert np.allclose(log[:, :3], exp["chunks"][:, :3], rtol=0, atol=1e-7), k
            tail = d.soft(k, first=exp["n_soft"] - 2000)                      # (the ring keeps the recent soft symbols only)
            assert tail.size == 2000 and np.max(np.abs(tail - exp["soft"][-2000:])) < SOFT_TIGHT * np.mean(np.abs(exp["soft"])), k
    finally:
        wb.close()
        d.close()


# ------------------------------------------------------------------ 6. refusals are atomic
def test_refused_pushes_change_nothing(amd, torch_dev):
    """a push that one stream cannot take - flushed, attached, without room - is refused with the documented code and has changed no
    stream and not the object: total_samples and the retained IQ of every stream are what they were, the same block pushed again
    after the cause is gone is accepted, and all outputs still == the model. A stream named by two objects is OPV_EINVAL."""
    torch, dev = torch_dev
    rng = np.random.default_rng(66)
    D, L, S, K = 2, 5, 17, 3
    streams, centres = [4, 0, 2], [300000.0, -700000.0, 0.0]
    taps = halved_taps(rng, L, 1 << 17)
    piece, n_pieces = 2000, 4
    wide = rng.integers(-20000, 20000, 2 * piece * n_pieces).astype(np.int16)
    exp = wb_model(amd.wb_lo_table(), wide, D, wb_model_inc(D, centres), taps, S)
    per = piece // D
    d = amd.Demod(5, max_samples=3 * per + 10, streaming=True)
    wb = amd.Wideband(d, D, streams, centres, taps, S)
    src = Sources(torch_dev, wide)
    scratch = torch.zeros(64, dtype=torch.int16, device=dev)
    try:
        for bad in ([4, 0, 7], [4, 0, -1], [1, 3, 1], [1, 2, 3], [3, 1, 4]):      # out of range, named twice, owned by the live object
            with pytest.raises(amd.OpvError) as e:
                amd.Wideband(d, D, bad, centres, taps, S)
            assert f"opv error {EINVAL}:" in str(e.value), (bad, e.value)
        other = amd.Wideband(d, D, [1, 3], centres[:2], taps, S)            # the free streams may be fed by a second object
        other.close()

        def snapshot():
            return [(d.state(k).total_samples, d.iq(k).tobytes()) for k in range(5)]

        def refused(code, lo, hi, kind="pageable"):
            before = snapshot()
            with pytest.raises(amd.OpvError) as e:
                src.push(wb, kind, lo, hi)
            assert f"opv error {code}:" in str(e.value), e.value
            assert snapshot() == before
        src.push(wb, "pinned", 0, piece)
        # one stream flushed
        d.flush(0)
        refused(ESTATE, piece, 2 * piece)
        refused(ESTATE, piece, 2 * piece, "device")
        d.reset(0)                                                           # (allowed: the object goes on feeding the stream, from here on)
        src.push(wb, "pageable", piece, 2 * piece)
        # one stream attached
        d.reset(2)
        d.attach(2, scratch.data_ptr(), 16, eof=False)
        refused(ESTATE, 2 * piece, 3 * piece, "pinned")
        d.reset(2)
        src.push(wb, "device", 2 * piece, 3 * piece)
        # one stream left without room: stream 4 holds 3 pushes, the others less
        assert d.iq(4).size // 2 == 3 * per and d.iq(0).size // 2 == 2 * per and d.iq(2).size // 2 == per
        refused(ECAPACITY, 3 * piece, 4 * piece)
        refused(ECAPACITY, 3 * piece, 4 * piece, "pinned")
        assert np.array_equal(d.iq(4), exp[0][: 2 * 3 * per])
        d.reset(4)
        src.push(wb, "pinned", 3 * piece, 4 * piece)
        # the object went on as if the refused calls had never been made: every stream holds the model from its last reset on
        held = {4: exp[0][2 * 3 * per:], 0: exp[1][2 * per:], 2: exp[2][2 * 2 * per:]}
        for k, x in held.items():
            assert x.size and np.array_equal(d.iq(k), x), k
        assert d.iq(1).size == 0 and d.iq(3).size == 0
        # ... and a later round sees exactly those samples: the same state as a context that was handed them by opv_push_iq
        wb.flush()
        d.process()
        d.sync()
        d2 = amd.Demod(5, max_samples=3 * per + 10, streaming=True)
        try:
            for k, x in held.items():
                d2.push(k, x)
                d2.flush(k)
            d2.process()
            d2.sync()
            for k in range(5):
                a, b = d.state(k), d2.state(k)
                for f in ("total_samples", "total_symbols", "chunk_origin", "n_chunks", "flushed", "frames_released", "sync_state", "stalled"):
                    assert getattr(a, f) == getattr(b, f), (k, f, getattr(a, f), getattr(b, f))
                assert np.array_equal(d.soft(k), d2.soft(k)), k
            assert d.state(4).total_symbols > 0
        finally:
            d2.close()
    finally:
        wb.close()
        d.close()


# ------------------------------------------------------------------ 7. ordering
def test_async_pushes_between_rounds_equal_the_synchronous_run(amd, torch_dev, e2e):
    """push_async -> process -> push_async -> sync for several rounds (the next block crosses PCIe while the kernels of the round in
    hand run; nothing waits on the host between a push and the opv_process behind it): same results as the synchronous run, i.e.
    the oracle's, and the same IQ in the buffers."""
    D = PLAN_D4["D"]
    wide = e2e["wide"]
    N = wide.size // 2
    src = Sources(torch_dev, wide)
    block = 100003
    cuts = list(range(0, N, block)) + [N]
    assert len(cuts) >= 7
    d = amd.Demod(len(PLAN_D4["centres"]), max_samples=amd.wb_outputs(D, N) + 64, streaming=True)
    wb = plan_wideband_d4(amd, d)
    try:
        wb.push_async(src.pinned[2 * cuts[0]: 2 * cuts[1]])
        for r in range(1, len(cuts)):
            if r == len(cuts) - 1:
                d.push_wait()
                wb.flush()
            d.process()
            if r < len(cuts) - 1:
                wb.push_async(src.pinned[2 * cuts[r]: 2 * cuts[r + 1]])
            d.sync()
        d.push_wait()
        for k in range(len(PLAN_D4["centres"])):
            assert np.array_equal(d.iq(k), e2e["model"][k]), k
        d.process()
        d.sync()
        check_plan_streams_d4(amd, d, e2e, "async rounds")
    finally:
        wb.close()
        d.close()


# ------------------------------------------------------------------ 8. lifetimes
def test_several_async_pushes_of_copied_blocks_and_an_object_that_outlives_its_context(amd):
    """(a) three opv_wb_push_async in flight before one push_wait, from inputs the binding has to copy (not contiguous, not int16):
    every copy stays referenced until the wait, and the streams hold the model. (b) a wideband object whose context is destroyed
    first is detached: push and flush answer OPV_ESTATE, closing it frees its own memory only."""
    rng = np.random.default_rng(8)
    D, L, S, centres = 2, 9, 18, [250000.0, -400000.0]
    taps = halved_taps(rng, L, 1 << 18)
    N = 3 * 5000
    wide = rng.integers(-20000, 20000, 2 * N).astype(np.int16)
    exp = wb_model(amd.wb_lo_table(), wide, D, wb_model_inc(D, centres), taps, S)
    d = amd.Demod(2, max_samples=N // D + 64, streaming=True)
    wb = amd.Wideband(d, D, [0, 1], centres, taps, S)
    try:
        spread = np.zeros((N, 4), np.int16)
        spread[:, :2] = wide.reshape(N, 2)
        wb.push_async(spread[:5000, :2])                                     # a strided view: copied
        wb.push_async(wide[2 * 5000: 2 * 10000].astype(np.int32))            # another type: copied
        wb.push_async(spread[10000:, :2])
        assert len(wb._inflight) == 3
        d.push_wait()
        assert len(wb._inflight) == 0
        for k in range(2):
            assert np.array_equal(d.iq(k), exp[k]), k
        d.close()
        for call in (lambda: wb.push(wide[:200]), wb.flush):
            with pytest.raises(amd.OpvError) as e:
                call()
            assert f"opv error {ESTATE}:" in str(e.value), e.value
    finally:
        wb.close()
        d.close()
