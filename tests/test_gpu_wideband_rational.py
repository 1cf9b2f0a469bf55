"""GPU: the rational wideband front door (opv_wb_create_rational, csrc/k_wideband_rational.hip + csrc/opv_wideband.hip): a capture
at 2 168 000 x down / up S/s. k_wbr_ddc is integer-exact, so its outputs are held to the numpy int64 model of
tests/wideband_models.py with == on every sample (read back through opv_tap_iq), for any split of a capture into pushes
and any mix of pinned, pageable and device sources; with up = 1 it must deliver the bytes of the integer door; and the streams it
feeds are held to the ORACLE run on the model's output like every other pushed stream (stream_checks.check_stream).

The end-to-end plan (wideband_device.PLAN_10M) is a 10 MS/s capture (down / up = 1250 / 271) with the channels of PLAN_D4 at
-3.1, 0.0 and +1.7 MHz and an empty slot at +3.9 MHz; the middle channel is at Eb/N0 = 14 dB (at 12 dB the reference alone loses
bits behind this door, so that is no precondition to build on). Each channel is brought from 2.168 to 10 MS/s by FFT zero-padding.
Prototype filter: 26 016 taps (J = 96 per phase) at 271 x 10 MS/s, Hamming-windowed sinc with a 200 kHz cut-off, every phase's sum
close to 2^15, out_shift = 30. The fixture asserts, from the oracle alone, that every transmitted frame is decoded and none on the
empty slot before the product sees a sample."""
import numpy as np
import pytest

from fixtures import amd, torch_dev  # noqa: F401
from stream_checks import SOFT_TIGHT, events_match
from stream_runs import CHUNK
from wideband_device import (PLAN_10M, Sources, assert_exactness_preconditions, check_plan_streams_10m, check_up_to_the_first_window,
                             exactness_inputs, first_one_tap_window, make_channel_10m, make_plan_capture_10m, plan_taps_10m, plan_wideband_10m,
                             to_wide)
from wideband_models import WIDE_RATE, halved_taps, per_phase_taps, wb_model, wb_model_inc, wbr_model, wbr_model_inc, wbr_outputs

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = -1, -4, -6


@pytest.fixture(scope="module")
def e2e(amd, oracle):
    return make_plan_capture_10m(amd, oracle, 2)


def plan_demod(amd, e2e):
    return amd.Demod(len(PLAN_10M["centres"]), max_samples=e2e["model"].shape[1] // 2 + 64, streaming=True)


# ------------------------------------------------------------------ 1. exactness
CASES = {
    # name: (down, up, L, K, S, first_sample, n_wide, input)
    "3_2_L1_empty_phase": (3, 2, 1, 1, 0, 0, 1000, "small"),              # J = 1, phase 1 holds no tap: every odd output is exactly 0
    "625_542_ragged_wrap32": (625, 542, 542 * 3 + 17, 5, 21, (1 << 32) - 1000, 1500, "random"),   # ragged last tap row; the phase product wraps
    "1250_271_K33_wrap40": (1250, 271, 271 * 37, 33, 33, (1 << 40) + 7, 3000, "random"),
    "7680_271_J64": (7680, 271, 271 * 64, 5, 36, 0, 17000, "random"),       # M / U = 28.3
    "32_1_J1024": (32, 1, 1024, 5, 36, 0, 32 * 300 + 5, "random"),          # largest ratio, largest J: the span at its limit
    "1025_1024_all_rows": (1025, 1024, 4096, 3, 34, 0, 1500, "random"),     # the phase walks through all 1024 rows one by one
    "1_1_L143_K5_clamps": (1, 1, 143, 5, 34, (1 << 32) - 1000, 2000, "fullscale"),   # the integer door's clamp case
    "3_2_L2_halfway": (3, 2, 2, 1, 3, 0, 1200, "halfway"),                  # accumulators at negative half-way points
}


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_integer_model_on_every_sample(amd, torch_dev, case):
    """opv_wb_push_device in two pieces (the cut at an odd sample inside a resampling period: the second needs the carry and starts
    at a phase other than 0) into a scratch context that never runs opv_process; every stream's IQ read back with opv_tap_iq == the
    model, sample for sample."""
    M, U, L, K, S, first, N, kind = CASES[case]
    # (the clamp case draws the centres, input and taps of test_gpu_wideband's D1_L143_K5_clamps: its seed, its order of draws)
    rng = np.random.default_rng(sum(map(ord, "D1_L143_K5_clamps" if kind == "fullscale" else case)))
    T = amd.wb_lo_table()
    (wide,), taps, centres = exactness_inputs(kind, rng, "rx", M * WIDE_RATE / U, K, N, L, U, halfway_taps=(1, 1))  # (phase 0 and phase 1: one tap of 1 each)
    inc = amd.wbr_plan(M, U, centres, taps, S, first)
    assert np.array_equal(inc, wbr_model_inc(M, U, centres))
    exp = wbr_model(T, wide, M, U, inc, taps, S, first)
    n_out = amd.wbr_outputs(M, U, N)
    assert n_out == wbr_outputs(M, U, N) and exp.shape == (K, 2 * n_out) and n_out > 256, "more than one workgroup of outputs"
    if kind == "small":
        assert not exp[0, 2::4].any() and not exp[0, 3::4].any() and exp[0, 0::4].any()        # odd outputs: the empty phase
    # halfway: channel 0 sits at centre 0 and every phase holds the single tap 1: acc[r] = 32767 x I[n_r]. With S = 3 an accumulator is
    # half-way when acc = 4 (mod 8), i.e. I = 4 (mod 8): I = -4
    n_r = (np.arange(n_out, dtype=np.int64) * M) // U
    assert_exactness_preconditions(kind, exp, halfway=(32767 * wide[0::2].astype(np.int64)[n_r], exp[0, 0::2]))
    if "wrap32" in case:
        assert first < (1 << 32) <= first + N
    d = amd.Demod(K, max_samples=n_out + 64, streaming=True)
    wb = amd.Wideband.rational(d, M, U, list(range(K)), centres, taps, S, first)
    try:
        src = Sources(torch_dev, wide)
        cut = (N // 2) | 1
        while M > 1 and (cut * U) % M == 0:                                 # an odd sample INSIDE a resampling period
            cut += 2
        assert cut < N and cut % 2 and (M == 1 or (cut * U) % M)
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


# ------------------------------------------------------------------ 2. up = 1 is the present door
def test_up_1_delivers_the_bytes_of_the_integer_door(amd, torch_dev):
    """a rational object (down = 4, up = 1) and an opv_wb_create object (decim = 4) fed the same random capture in the same pieces:
    the same IQ in every stream, == both models"""
    rng = np.random.default_rng(41)
    D, L, K, S, first, N = 4, 143, 5, 33, (1 << 32) - 1000, 4 * 600 + 3
    centres = list(rng.uniform(-D * WIDE_RATE / 2, D * WIDE_RATE / 2, K))
    wide, taps = rng.integers(-32768, 32768, 2 * N).astype(np.int16), halved_taps(rng, L)
    T = amd.wb_lo_table()
    inc = amd.wbr_plan(D, 1, centres, taps, S, first)
    assert np.array_equal(inc, amd.wb_plan(D, centres, taps, S, first)) and np.array_equal(inc, wb_model_inc(D, centres))
    exp = wb_model(T, wide, D, inc, taps, S, first)
    assert np.array_equal(exp, wbr_model(T, wide, D, 1, inc, taps, S, first))
    assert amd.wbr_outputs(D, 1, N) == amd.wb_outputs(D, N) > 256
    d = amd.Demod(2 * K, max_samples=exp.shape[1] // 2 + 64, streaming=True)
    a = amd.Wideband.rational(d, D, 1, list(range(K)), centres, taps, S, first)
    b = amd.Wideband(d, D, list(range(K, 2 * K)), centres, taps, S, first)
    try:
        src = Sources(torch_dev, wide)
        cuts = [0, 1, 6, (N // 2) | 1, N - 2, N]
        for lo, hi in zip(cuts, cuts[1:]):
            for wb in (a, b):
                src.push(wb, "device", lo, hi)
        for k in range(K):
            x, y = d.iq(k), d.iq(K + k)
            assert np.array_equal(x, y), k
            assert np.array_equal(x, exp[k]), k
    finally:
        a.close()
        b.close()
        d.close()


# ------------------------------------------------------------------ 3. any split equals one shot
def test_any_split_and_any_source_equals_one_shot(amd, torch_dev, e2e):
    """the plan's capture whole (pinned), and in pieces of 1, 2, 5, J - 2 and 40 001 wide samples taken in turn from pinned, pageable
    and device memory (5 sizes x 3 sources: every pair occurs): the streams' IQ == the model in both runs, and the frames, metrics,
    symbols, tracker lines and chunk log of both == the oracle on the model's output"""
    wide = e2e["wide"]
    N = wide.size // 2
    src = Sources(torch_dev, wide)
    pieces, kinds = [1, 2, 5, PLAN_10M["J"] - 2, 40001], ["pinned", "pageable", "device"]
    for split in (False, True):
        d = plan_demod(amd, e2e)
        wb = plan_wideband_10m(amd, d)
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
            for k in range(len(PLAN_10M["centres"])):
                assert np.array_equal(d.iq(k), e2e["model"][k]), (split, k)
            wb.flush()
            d.process()
            d.sync()
            check_plan_streams_10m(amd, d, e2e, "split" if split else "one shot")
        finally:
            wb.close()
            d.close()


# ------------------------------------------------------------------ 4. end to end against the oracle
@pytest.mark.parametrize("streams_per_wave", [0, 4])
def test_end_to_end_against_the_oracle(amd, e2e, streams_per_wave):
    """each stream's frames, metrics, release symbols, tracker lines and chunk log == Oracle().receive(model output), soft symbols
    < 1e-9 - with the context on its automatic mapping and forced to 4 streams per wave"""
    d = plan_demod(amd, e2e)
    wb = plan_wideband_10m(amd, d)
    try:
        if streams_per_wave:
            d.set_frontend(streams_per_wave)
        wb.push(e2e["wide"])
        wb.flush()
        d.process()
        d.sync()
        check_plan_streams_10m(amd, d, e2e, f"mapping {streams_per_wave}")
    finally:
        wb.close()
        d.close()


def test_async_pushes_between_rounds_equal_the_synchronous_run(amd, torch_dev, e2e):
    """push_async -> process -> push_async -> sync for several rounds, then push_wait: the oracle's results and the model's IQ"""
    wide = e2e["wide"]
    N = wide.size // 2
    src = Sources(torch_dev, wide)
    block = 100003
    cuts = list(range(0, N, block)) + [N]
    assert len(cuts) >= 7
    d = plan_demod(amd, e2e)
    wb = plan_wideband_10m(amd, d)
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
        for k in range(len(PLAN_10M["centres"])):
            assert np.array_equal(d.iq(k), e2e["model"][k]), k
        d.process()
        d.sync()
        check_plan_streams_10m(amd, d, e2e, "async rounds")
    finally:
        wb.close()
        d.close()


# ------------------------------------------------------------------ 5. refusals are atomic
def test_refused_pushes_change_nothing(amd, torch_dev):
    """a push that one stream cannot take - flushed (OPV_ESTATE), without room (OPV_ECAPACITY) - has changed no stream and not the
    object: every stream's IQ is what it was, and what the object delivers afterwards == the model and == a second object's run in
    which the refused pushes were never made - so its N and its history (J - 1 = 4 samples, pieces that end inside a resampling
    period) did not move."""
    rng = np.random.default_rng(67)
    M, U, L, S = 3, 2, 9, 17
    streams, centres = [4, 0, 2], [300000.0, -700000.0, 0.0]
    taps = per_phase_taps(rng, L, U, 1 << 17)
    piece, n_pieces = 3001, 4
    wide = rng.integers(-20000, 20000, 2 * piece * n_pieces).astype(np.int16)
    exp = wbr_model(amd.wb_lo_table(), wide, M, U, wbr_model_inc(M, U, centres), taps, S)
    cum = [wbr_outputs(M, U, i * piece) for i in range(n_pieces + 1)]
    assert (piece * U) % M and len({b - a for a, b in zip(cum, cum[1:])}) == 2       # pieces end inside a period; their output counts differ
    src = Sources(torch_dev, wide)
    runs = []
    for with_refusals in (True, False):
        d = amd.Demod(5, max_samples=cum[3] + 10, streaming=True)
        wb = amd.Wideband.rational(d, M, U, streams, centres, taps, S)
        try:
            def snapshot():
                return [(d.state(k).total_samples, d.iq(k).tobytes()) for k in range(5)]

            def refused(code, lo, hi, kind):
                if not with_refusals:
                    return
                before = snapshot()
                with pytest.raises(amd.OpvError) as e:
                    src.push(wb, kind, lo, hi)
                assert f"opv error {code}:" in str(e.value), e.value
                assert snapshot() == before
            src.push(wb, "pinned", 0, piece)
            if with_refusals:
                d.flush(0)                                                   # one stream flushed
            refused(ESTATE, piece, 2 * piece, "pageable")
            refused(ESTATE, piece, 2 * piece, "device")
            d.reset(0)
            src.push(wb, "pageable", piece, 2 * piece)
            d.reset(2)
            src.push(wb, "device", 2 * piece, 3 * piece)
            # one stream left without room: stream 4 holds 3 pushes, the others less
            assert d.iq(4).size // 2 == cum[3] and d.iq(0).size // 2 == cum[3] - cum[1] and d.iq(2).size // 2 == cum[3] - cum[2]
            refused(ECAPACITY, 3 * piece, 4 * piece, "pageable")
            refused(ECAPACITY, 3 * piece, 4 * piece, "pinned")
            assert np.array_equal(d.iq(4), exp[0][: 2 * cum[3]])
            d.reset(4)
            src.push(wb, "pinned", 3 * piece, 4 * piece)
            held = {4: exp[0][2 * cum[3]:], 0: exp[1][2 * cum[1]:], 2: exp[2][2 * cum[2]:]}
            for k, x in held.items():
                assert x.size and np.array_equal(d.iq(k), x), (with_refusals, k)
            assert d.iq(1).size == 0 and d.iq(3).size == 0
            runs.append(snapshot())
        finally:
            wb.close()
            d.close()
    assert runs[0] == runs[1]


# ------------------------------------------------------------------ 6. long run through small buffers
def test_long_run_through_small_buffers(amd, oracle, torch_dev):
    """12 frames of one channel at 10 MS/s in pushes of 50 001 wide samples through a context whose buffer holds 3 chunks + one
    push: a push, opv_process and a pop per round. Outputs per push take both floor and ceil of 50 001 x 271 / 1250; the IQ still
    retained == the model after every push, and at the end everything == the oracle on the model's output."""
    M, U, J, S, centre, push = PLAN_10M["down"], PLAN_10M["up"], 24, PLAN_10M["out_shift"], 1700000.0, 50001
    tx, z = make_channel_10m(amd, 2, 12)
    fw = M * WIDE_RATE / U
    wide = to_wide(z * np.exp(2j * np.pi * centre / fw * np.arange(z.size, dtype=np.float64)))
    taps = plan_taps_10m(J)
    model = wbr_model(amd.wb_lo_table(), wide, M, U, wbr_model_inc(M, U, [centre]), taps, S)[0]
    exp = oracle.receive(model, streaming=True)
    assert np.array_equal(exp["frames"], tx) and len(tx) == 12              # (the reference alone decodes the channel behind this door)
    assert first_one_tap_window(exp)[0] >= 12 * 2168                        # (and shows no one-tap window inside the frames)
    N = wide.size // 2
    src = Sources(torch_dev, wide)
    d = amd.Demod(1, max_samples=3 * CHUNK + wbr_outputs(M, U, push) + 1, streaming=True)
    wb = amd.Wideband.rational(d, M, U, [0], [centre], taps, S)
    try:
        frames, metas, events, chunks, per_push = [], [], [], [], set()
        base = compactions = at = r = 0
        while at < N:
            m = min(push, N - at)
            origin = d.state(0).chunk_origin
            src.push(wb, ("pinned", "device", "pageable")[r % 3], at, at + m)
            if m == push:
                per_push.add(amd.wbr_outputs(M, U, at + m) - amd.wbr_outputs(M, U, at))
            at += m
            have = amd.wbr_outputs(M, U, at)
            if d.iq(0, first=base, cap=1).size == 0:                        # the sample at the old keep point is gone: compacted
                compactions += 1
                base = (origin - 16) & ~3
            got = d.iq(0, first=base)
            assert np.array_equal(got, model[2 * base: 2 * have]), (r, base, got.size // 2, have)
            if at == N:
                wb.flush()
            d.process()
            d.sync()
            f, mt = d.pop_frames(0)
            frames.append(f)
            metas.append(mt)
            events.append(d.pop_events(0))
            chunks.append(d.chunks(0, first=sum(map(len, chunks))))
            r += 1
        assert per_push == {push * U // M, push * U // M + 1}, per_push
        assert compactions >= 3, compactions
        st = d.state(0)
        fr, meta, ev, log = np.concatenate(frames), np.concatenate(metas), np.concatenate(events), np.concatenate(chunks)
        assert st.n_chunks == len(exp["chunks"]) == len(log) >= 12
        if first_one_tap_window(exp)[1]:                                     # (in the tail of zeros behind the 12 frames: asserted above)
            check_up_to_the_first_window(amd, st, fr, meta, ev, log, exp, "long run")
        else:
            assert st.stalled == 0 and st.edge_ties == 0 and st.total_symbols == exp["n_soft"], (st.total_symbols, exp["n_soft"])
            assert np.array_equal(fr, exp["frames"]) and np.array_equal(meta["viterbi_metric"], exp["metrics"])
            assert np.array_equal(meta["release_symbol"], exp["frame_sym"])
            events_match(amd, ev, exp["events"])
            assert abs(st.freq_offset_hz - exp["final_freq_offset"]) < 1e-6 and st.sync_state == exp["final_state"]
            assert np.array_equal(log[:, 3:], exp["chunks"][:, 3:])
            assert np.allclose(log[:, :3], exp["chunks"][:, :3], rtol=0, atol=1e-7)
        tail = d.soft(0, first=exp["n_soft"] - 2000)                        # (the ring keeps the recent soft symbols only)
        assert tail.size == 2000 and exp["n_soft"] - 200 <= 12 * 2168        # ... of which the last 200 lie in or next to the tail of zeros
        assert np.max(np.abs(tail[:1800] - exp["soft"][-2000:-200])) < SOFT_TIGHT * np.mean(np.abs(exp["soft"]))
    finally:
        wb.close()
        d.close()
