"""GPU: the wideband scan (opv_scan_*, csrc/k_scan.hip + csrc/opv_scan.hip). k_scan_probe is integer-exact, so the rows an object
delivers are held to the numpy int64 model of tests/scan_model.py with == on every value, for any split of a capture into pushes
and any mix of pinned, pageable and device sources, at the smallest shapes at which the kernel can go wrong: every P that fills
lanes differently (1, 3, 65, 257, 1024), windows of 1, 7, 1024 and 4096 taps, hops below, at and above the window, blocks of 1, 3
and 64 segments, both kinds of wide rate, phases and sample indices that cross 2^32, both clamps (CASES: every push of these is
launched with one segment per workgroup), and every launch shape of k_scan_probe (SHAPES: several segments per workgroup, a shorter
last run, a block that is not cut at all), each asserted from the launch rule before the device runs.

The end-to-end case (tests/scan_inputs.py, SCAN_PLAN): three BERT channels of the D = 4 plan whose carriers sit +7 300, -4 100 and
+15 250 Hz off their nominal centres under wideband noise (the weakest at Eb/N0 = 12 dB). The device's rows, summed, give carriers
within 1500 Hz of the truth (the half-range of the reference's coarse search; the CPU model alone stays within 1000 Hz: the
precondition); a Wideband created at the found centres decodes every transmitted frame, every stream == the oracle on wb_model at
those centres; and the control, on the oracle alone: fed wb_model at the NOMINAL centres it releases no frame on the +15 250 Hz
channel. (The issue's +11 250 Hz was not far enough: there, and at +13 250 Hz, the oracle at the nominal centre still released two
frames - wrong ones; +15 250 Hz is the first 2 kHz step at which it releases none.)"""
import numpy as np
import pytest

from fixtures import amd, torch_dev  # noqa: F401
from scan_inputs import (SCAN_PLAN, door_streams_on_the_cpu, make_scan_capture, scan_plan_carriers, scan_plan_probes, scan_plan_rows_model)
from scan_model import hann_window, scan_blocks, scan_keep, scan_model, scan_segment_sums, scan_shape
from stream_checks import check_stream
from stream_runs import collect
from wideband_device import PLAN_D4, Sources, plan_taps_d4
from wideband_models import WIDE_RATE, halved_taps, wb_model, wb_model_inc, wbr_model_inc

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = -1, -4, -6


def assert_rows(got, exp, tag):
    assert got.shape == exp.shape and got.dtype == exp.dtype == np.uint64, (tag, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{tag}: {len(bad)} of {got.size} values differ, first at block {bad[0][0]} probe {bad[0][1]}: {got[tuple(bad[0])]} vs {exp[tuple(bad[0])]}"


# ------------------------------------------------------------------ 1. exactness
CASES = {
    # name: (down, up, P, Lw, H, A, S, first_sample, n_wide, input)
    "P1_Lw1_H1_A1_S0": (1, 1, 1, 1, 1, 1, 0, 0, 3000, "tiny"),                    # S = 0: no rounding term; a block per sample
    "P3_Lw7_H20_A3_wrap32": (3, 1, 3, 7, 20, 3, 25, (1 << 32) - 1000, 20001, "random"),    # H > Lw; a and a x inc cross 2^32 inside the capture
    "P65_Lw7_H5_A64": (4, 1, 65, 7, 5, 64, 25, 12345, 20003, "random"),          # 62 blocks of 64 segments (31 per push: 64 runs of one)
    "P65_Lw1024_H1024_A3_10M": (1250, 271, 65, 1024, 1024, 3, 31, (1 << 40) + 7, 20000, "random"),   # H = Lw, the rational rate, runs of one segment
    "P257_Lw1024_H512_A3": (4, 1, 257, 1024, 512, 3, 31, 0, 20011, "random"),    # H < Lw, two probe groups, the second one lane wide
    "P1024_Lw1024_H512_A1": (7680, 271, 1024, 1024, 512, 1, 31, 77, 4000, "random"),
    "P3_Lw4096_H2048_A3": (4, 1, 3, 4096, 2048, 3, 33, (1 << 32) - 9000, 20000, "random"),
    "P3_Lw64_S40_fullscale": (4, 1, 3, 64, 64, 3, 40, 1 << 29, 20000, "fullscale"),
    "P3_Lw64_S27_clamps": (4, 1, 3, 64, 64, 3, 27, 1 << 29, 20000, "fullscale"),    # |z| reaches 2^51.5 of the 2^52 bound; both clamps fire
}


def case_inputs(case):
    down, up, P, Lw, H, A, S, first, N, kind = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    fw = down * WIDE_RATE / up
    probes = list(rng.uniform(-fw / 2, fw / 2, P))
    if kind == "tiny":
        wide, window, probes = rng.integers(-9, 10, 2 * N).astype(np.int16), np.array([3], np.int16), [0.0]
    elif kind == "random":
        wide, window = rng.integers(-32768, 32768, 2 * N).astype(np.int16), halved_taps(rng, Lw, 1 << 21)
    else:
        # a window at the gain cap (64 x -32768 = 2^21 exactly) against full scale: probe 0 has inc = 1 and first_sample = 2^29, so its
        # LO stands at 45 degrees (c = s = 23170) and |I c + Q s| = 2 x 32768 x 23170 over the two constant stretches at the start
        wide = rng.choice(np.array([-32768, 32767], np.int16), 2 * N)
        wide[: 2 * 3 * Lw], wide[2 * 3 * Lw: 2 * 6 * Lw] = -32768, 32767
        window = np.full(Lw, -32768, np.int16)
        probes[0], probes[1] = fw / 4294967296.0, 0.0
    return wide, window, probes


@pytest.mark.parametrize("case", list(CASES))
def test_rows_equal_the_integer_model_on_every_value(amd, torch_dev, case):
    """one capture in two device pushes from a pointer that is only 4-byte aligned (the second starts inside a segment and needs
    the carry); every row popped == the model"""
    down, up, P, Lw, H, A, S, first, N, kind = CASES[case]
    wide, window, probes = case_inputs(case)
    T = amd.wb_lo_table()
    inc = amd.scan_plan(down, up, probes, window, H, A, S, first_sample=first)
    assert np.array_equal(inc, wbr_model_inc(down, up, probes))
    exp = scan_model(T, wide, inc, window, H, A, S, first)
    blocks = amd.scan_blocks(Lw, H, A, N, down, up)
    assert exp.shape == (blocks, P) and blocks == scan_blocks(Lw, H, A, N) and blocks >= 2
    if "wrap32" in case:
        assert first < (1 << 32) <= first + N
    if kind == "fullscale":                                                  # the preconditions, on the MODEL
        zr, zi = scan_segment_sums(T, wide, inc, window, H, first)
        top = max(int(np.max(np.abs(zr))), int(np.max(np.abs(zi))))
        assert (1 << 51) < top < (1 << 52) and inc[0] == 1 and inc[1] == 0
        if S == 27:
            y = np.concatenate([(zr + (1 << 26)) >> 27, (zi + (1 << 26)) >> 27]).ravel()
            assert (y > (1 << 24) - 1).any() and (y < -(1 << 24)).any() and (np.abs(y) < (1 << 23)).any()
            # probe 0 over the constant stretches: zi = 0, zr at the upper clamp in block 0 and at the lower one in block 1
            assert int(exp[0, 0]) == 3 * ((1 << 24) - 1) ** 2 and int(exp[1, 0]) == 3 * (1 << 48)
        else:
            assert top >> 40 < 1 << 12 and exp.max() > 0
    if kind == "tiny":
        assert 0 < exp.max() <= 2 * (3 * 9 * 32767) ** 2
    d = amd.Demod(1, max_samples=1 << 16, streaming=True)
    sc = amd.Scan(d, down, up, probes, window, H, A, S, ring_blocks=blocks, first_sample=first)
    try:
        src = Sources(torch_dev, np.concatenate([np.zeros(2, np.int16), wide]))       # the capture starts at sample 1 of the buffer
        assert (src.dev_t.data_ptr() + 4) % 16 == 4
        cut = (N // 2) | 1
        src.push(sc, "device", 1, 1 + cut)
        src.push(sc, "device", 1 + cut, 1 + N)
        got, first_block = sc.pop()
        assert first_block == 0
        assert_rows(got, exp, case)
        assert sc.pop()[0].shape == (0, P)
    finally:
        sc.close()
        d.close()


# ------------------------------------------------------------------ 1b. every launch shape
SHAPES = {
    # name: (P, Lw, H, A, S, n_wide, cuts, (run_len, runs, pgroups) of the push that completes the most blocks, segments of its last run)
    "two_per_run": (65, 7, 5, 64, 25, 20003, [], (2, 32, 1), 2),                      # 62 blocks in ONE push
    "four_per_run_last_three": (257, 7, 5, 67, 25, 20003, [], (4, 17, 2), 3),        # 59 blocks, A % run_len != 0: the last run is shorter
    "two_per_run_full_window": (3, 1024, 16, 64, 31, 40000, [], (2, 32, 1), 2),      # 38 blocks: LDS reused by a second segment of 1024 taps
    "uncut_blocks": (3, 3, 2, 3, 20, 12300, [], (3, 1, 1), 3),                       # 2049 blocks in one push: run_len = A
    "eight_per_run_after_a_carry": (1024, 7, 5, 67, 25, 20433, [333], (8, 9, 4), 3),   # 60 blocks behind a carry of 333 samples, four probe groups
}


@pytest.mark.parametrize("case", list(SHAPES))
def test_rows_equal_the_model_on_every_launch_shape(amd, torch_dev, case):
    """a push that completes so many blocks that a workgroup takes several segments of one (it reuses its LDS behind a barrier and adds
    the segments' powers), with a shorter last run, or a whole block; the shape is computed from the launch rule (scan_model.scan_shape,
    held to the C rule on the CPU) and asserted first"""
    P, Lw, H, A, S, N, cuts, shape, last = SHAPES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    wide, window = rng.integers(-32768, 32768, 2 * N).astype(np.int16), halved_taps(rng, Lw, 1 << 21)
    probes = list(rng.uniform(-4e6, 4e6, P))
    cuts = [0] + cuts + [N]
    per_push = [scan_blocks(Lw, H, A, hi) - scan_blocks(Lw, H, A, lo) for lo, hi in zip(cuts, cuts[1:])]
    got_shape = scan_shape(P, A, max(per_push))
    assert got_shape == shape and A - (shape[1] - 1) * shape[0] == last and shape[0] > 1, (got_shape, per_push)
    exp = scan_model(amd.wb_lo_table(), wide, wbr_model_inc(4, 1, probes), window, H, A, S, 7)
    assert len(exp) == sum(per_push) <= 4096
    src = Sources(torch_dev, wide)
    d = amd.Demod(1, max_samples=1 << 16, streaming=True)
    sc = amd.Scan(d, 4, 1, probes, window, H, A, S, ring_blocks=len(exp), first_sample=7)
    try:
        for lo, hi in zip(cuts, cuts[1:]):
            src.push(sc, "device", lo, hi)
        assert_rows(sc.pop()[0], exp, case)
    finally:
        sc.close()
        d.close()


def test_pushes_that_end_in_the_gap_between_blocks(amd, torch_dev):
    """H > Lw: a block's last sample comes before the next block's first, so a push can end where nothing is carried (keep = 0) and
    the next push's leading samples belong to no segment and are skipped. Pushes that end on a block's last sample, inside the gap,
    one sample before the next block and one sample into it, from every kind of source: rows == the model."""
    rng = np.random.default_rng(44)
    P, Lw, H, A, S, N = 5, 7, 20, 3, 25, 4000
    span, stride = (A - 1) * H + Lw, A * H
    assert span == 47 and stride == 60
    wide, window = rng.integers(-32768, 32768, 2 * N).astype(np.int16), halved_taps(rng, Lw, 1 << 21)
    probes = list(rng.uniform(-4e6, 4e6, P))
    exp = scan_model(amd.wb_lo_table(), wide, wbr_model_inc(4, 1, probes), window, H, A, S, (1 << 32) - 500)
    cuts = [0, 5 * stride + span, 9 * stride + 50, 10 * stride - 1, 10 * stride + 1, 20 * stride + 59, 21 * stride + 58, 21 * stride + 59, 40 * stride + 30, N]
    keeps = [scan_keep(Lw, H, A, c) for c in cuts]
    assert keeps[1] == 0 and keeps[2] == 0 and keeps[3] == 0 and keeps[4] == 1 and keeps[5] == 0 and keeps[6] == 0 and keeps[7] == 0 and keeps[8] == 30
    src = Sources(torch_dev, wide)
    d = amd.Demod(1, max_samples=1 << 16, streaming=True)
    sc = amd.Scan(d, 4, 1, probes, window, H, A, S, ring_blocks=len(exp), first_sample=(1 << 32) - 500)
    try:
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            src.push(sc, ("device", "pinned", "pageable")[j % 3], lo, hi)
        assert_rows(sc.pop()[0], exp, "gap")
    finally:
        sc.close()
        d.close()


# ------------------------------------------------------------------ 2. any split, any source
def test_any_split_and_any_source_equals_one_push(amd, torch_dev):
    """one capture in one pinned push, and in pieces taken in turn from pinned, pageable and device memory: shorter than the carry,
    ending exactly on a block's last sample, empty, completing several blocks at once; rows popped now and then. All == the model,
    and the blocks are numbered through."""
    rng = np.random.default_rng(5)
    down, up, P, Lw, H, A, S, first, N = 4, 1, 70, 100, 37, 4, 27, 999, 20000
    span, stride = (A - 1) * H + Lw, A * H
    wide, window = rng.integers(-32768, 32768, 2 * N).astype(np.int16), halved_taps(rng, Lw, 1 << 21)
    probes = list(rng.uniform(-4e6, 4e6, P))
    exp = scan_model(amd.wb_lo_table(), wide, wbr_model_inc(down, up, probes), window, H, A, S, first)
    blocks = len(exp)
    src = Sources(torch_dev, wide)
    d = amd.Demod(1, max_samples=1 << 16, streaming=True)
    try:
        sc = amd.Scan(d, down, up, probes, window, H, A, S, ring_blocks=blocks, first_sample=first)
        src.push(sc, "pinned", 0, N)
        got, b0 = sc.pop()
        assert b0 == 0
        assert_rows(got, exp, "one push")
        sc.close()
        # cuts: inside the first segment, one sample before / exactly on / one behind a block's last sample, an empty push, tiny pieces
        # (all shorter than the carry), then 11 blocks at once, then odd pieces to the end
        cuts = [0, 5, span - 1, span, span, span + 1, span + 2, span + 3, stride + span, 2 * stride + span - 1, 13 * stride + span + 9]
        while cuts[-1] < N:
            cuts.append(min(N, cuts[-1] + int(rng.integers(1, 3 * span))))
        assert span > 40 and cuts[3] == cuts[4]
        sc = amd.Scan(d, down, up, probes, window, H, A, S, ring_blocks=blocks, first_sample=first)
        rows, at_block, kinds = [], 0, ["pinned", "pageable", "device"]
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            src.push(sc, kinds[j % 3], lo, hi)
            if j % 4 == 3 or hi == N:
                got, b0 = sc.pop()
                assert b0 == at_block and at_block + len(got) == scan_blocks(Lw, H, A, hi), (j, b0, at_block, len(got))
                at_block += len(got)
                rows.append(got)
        assert_rows(np.concatenate(rows), exp, "pieces")
        sc.close()
    finally:
        d.close()


# ------------------------------------------------------------------ 3. the ring, reset, lifetimes
def test_full_ring_refuses_and_changes_nothing_reset_and_detachment(amd, torch_dev):
    rng = np.random.default_rng(6)
    down, up, P, Lw, H, A, S, N = 1250, 271, 5, 16, 16, 2, 20, 32 * 7 + 5
    wide, window = rng.integers(-32768, 32768, 2 * N).astype(np.int16), halved_taps(rng, Lw, 1 << 20)
    probes = [0.0, 1e6, -2e6, 3.3e6, -4.9e6]
    T, inc = amd.wb_lo_table(), wbr_model_inc(down, up, probes)
    exp = scan_model(T, wide, inc, window, H, A, S, 11)
    assert len(exp) == 7
    src = Sources(torch_dev, wide)
    d = amd.Demod(1, max_samples=1 << 16, streaming=True)
    sc = amd.Scan(d, down, up, probes, window, H, A, S, ring_blocks=3, first_sample=11)
    try:
        src.push(sc, "pinned", 0, 32 * 3 + 7)                                # three blocks and seven samples of the fourth: the ring is full
        for kind in ("pinned", "pageable", "device"):
            with pytest.raises(amd.OpvError) as e:
                src.push(sc, kind, 32 * 3 + 7, 32 * 4)                       # completes the fourth
            assert f"opv error {ECAPACITY}:" in str(e.value), e.value
        src.push(sc, "device", 32 * 3 + 7, 32 * 4 - 1)                       # one sample short of it: accepted, the carry grows
        with pytest.raises(amd.OpvError):
            src.push(sc, "device", 32 * 4 - 1, 32 * 4)
        got, b0 = sc.pop(2)                                                  # frees two rows
        assert b0 == 0
        assert_rows(got, exp[:2], "first two")
        src.push(sc, "pageable", 32 * 4 - 1, 32 * 5 + 3)                     # the same push now succeeds, and one block more: full again
        with pytest.raises(amd.OpvError):
            src.push(sc, "pinned", 32 * 5 + 3, N)
        got, b0 = sc.pop()
        assert b0 == 2
        assert_rows(got, exp[2:5], "around the wrap")                        # rows 2, 3, 4 lie at ring rows 2, 0, 1
        src.push(sc, "pinned", 32 * 5 + 3, N)
        got, b0 = sc.pop()
        assert b0 == 5
        assert_rows(got, exp[5:], "the rest")
        # reset in the middle of a block, then another first_sample: the carry is gone and blocks count from 0
        src.push(sc, "device", 0, 19)
        sc.reset((1 << 32) - 50)
        src.push(sc, "device", 10, 10 + 32 * 3 + 5)
        got, b0 = sc.pop()
        assert b0 == 0
        assert_rows(got, scan_model(T, wide[20: 20 + 2 * (32 * 3 + 5)], inc, window, H, A, S, (1 << 32) - 50), "after reset")
        # refusals of the create call, and an object that outlives its context
        with pytest.raises(amd.OpvError) as e:
            amd.Scan(d, 6, 4, probes, window, H, A, S)
        assert f"opv error {EINVAL}:" in str(e.value)
        d.close()
        for call in (lambda: sc.push(wide[:64]), sc.pop, sc.reset):
            with pytest.raises(amd.OpvError) as e:
                call()
            assert f"opv error {ESTATE}:" in str(e.value), e.value
    finally:
        sc.close()
        d.close()


# ------------------------------------------------------------------ 4. beside a door, on the same device block
def test_a_scan_and_a_door_of_one_context_fed_the_same_device_block(amd, torch_dev):
    rng = np.random.default_rng(7)
    D, L, S, N = 4, 33, 20, 20000
    wide, taps, centres = rng.integers(-20000, 20000, 2 * N).astype(np.int16), halved_taps(rng, L, 1 << 18), [300000.0, -1700000.0]
    probes, window = list(rng.uniform(-4e6, 4e6, 40)), hann_window(256)
    T = amd.wb_lo_table()
    exp_rows = scan_model(T, wide, wbr_model_inc(D, 1, probes), window, 128, 8, 24, 5)
    exp_iq = wb_model(T, wide, D, wb_model_inc(D, centres), taps, S, 5)
    src = Sources(torch_dev, wide)
    d = amd.Demod(2, max_samples=N // D + 64, streaming=True)
    sc = amd.Scan(d, D, 1, probes, window, 128, 8, 24, ring_blocks=len(exp_rows), first_sample=5)
    wb = amd.Wideband(d, D, [0, 1], centres, taps, S, 5)
    try:
        for lo, hi in ((0, 7001), (7001, 7002), (7002, N)):
            src.push(sc, "device", lo, hi)
            src.push(wb, "device", lo, hi)
        assert_rows(sc.pop()[0], exp_rows, "scan beside a door")
        for k in range(2):
            assert np.array_equal(d.iq(k), exp_iq[k]), k
    finally:
        wb.close()
        sc.close()
        d.close()


# ------------------------------------------------------------------ 5. end to end
@pytest.fixture(scope="module")
def e2e(amd, oracle):
    cap = make_scan_capture(amd)
    cap["rows"] = scan_plan_rows_model(amd, cap["wide"])
    return cap


def test_end_to_end_scan_find_tune_decode(amd, oracle, e2e):
    """see the module's docstring. The control's carrier sits +15 250 Hz off its nominal centre: at the issue's +11 250 Hz, and at
    +13 250 Hz, the oracle fed the nominal centre still released two (wrong) frames. Measured on the MI355X: the device's rows ==
    the model's, so the found centres are the model's, -19, +404 and -487 Hz from the truth."""
    p, true_hz = SCAN_PLAN, e2e["true_hz"]
    # the precondition, on the CPU alone
    model_found = scan_plan_carriers(e2e["rows"])
    assert len(model_found) == 3 and max(abs(f[0] - t) for f, t in zip(model_found, true_hz)) < 1000.0, (model_found, true_hz)
    _, _, probes = scan_plan_probes()
    K = 3
    d = amd.Demod(K, max_samples=amd.wb_outputs(PLAN_D4["D"], e2e["wide"].size // 2) + 64, streaming=True)
    sc = amd.Scan(d, PLAN_D4["D"], 1, probes, hann_window(p["n_window"]), p["hop"], p["n_avg"], p["out_shift"], ring_blocks=16)
    wb = None
    try:
        # 1. the device scan, 2. the carriers
        sc.push(e2e["wide"][: 2 * p["scan_samples"]])
        rows, _ = sc.pop()
        assert_rows(rows, e2e["rows"], "plan rows")
        found = scan_plan_carriers(rows, amd.scan_carriers)
        print("found", [f[0] for f in found], "errors", [f[0] - t for f, t in zip(found, true_hz)])
        assert len(found) == 3
        for f, t in zip(found, true_hz):
            assert abs(f[0] - t) < 1500.0, (f, t)
        centres = [f[0] for f in found]
        # 3. a door at the found centres, 4. decode: every stream == the oracle on the model at those centres, the frames are the transmitted ones
        model, exp = door_streams_on_the_cpu(amd, oracle, e2e["wide"], centres)
        wb = amd.Wideband(d, PLAN_D4["D"], list(range(K)), centres, plan_taps_d4(), PLAN_D4["out_shift"])
        wb.push(e2e["wide"])
        for k in range(K):
            assert np.array_equal(d.iq(k), model[k]), k
        wb.flush()
        d.process()
        d.sync()
        for k in range(K):
            got = collect(d, k)
            assert got["state"].stalled == 0
            check_stream(amd, got, exp[k], f"scan plan slot {k}", edge_ties=0, offset_ties=None)
            assert np.array_equal(got["frames"], e2e["tx"][k]) and len(got["frames"]) == p["frames"], k
        # the control, on the oracle alone: at the nominal centres the far channel is lost
        _, ctl = door_streams_on_the_cpu(amd, oracle, e2e["wide"], p["centres"])
        assert len(ctl[2]["frames"]) == 0
    finally:
        if wb is not None:
            wb.close()
        sc.close()
        d.close()
