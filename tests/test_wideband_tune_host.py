"""CPU-only: the LO schedule of the four wideband converters (include/opv_demod.h, "per-channel retune and Doppler ramps"; the
rules are csrc/opv_wb_rules.cpp) against tests/wideband_tune_model.py: opv_wb_seg_phase and opv_wb_seg_next against the model in
Python integers, the four scheduled models against the four models of tests/wideband_models.py and against each other, and the
rules - every refusal and that it changes nothing, pruning on the receive and the transmit rule, the per-push device table against
the absolute formula - as a stand-alone program under ASan + UBSan (tests/san_tune/)."""
import subprocess

import numpy as np
import pytest

from amd_lib import ROOT
from fixtures_built import amd  # noqa: F401
from struct_layout import check_ctypes_layout
from wideband_models import (WIDE_RATE, per_phase_taps, tx_phase_taps, wb_model, wb_model_inc, wbr_model, wbr_model_inc, wbtx_model,
                             wbtxr_model)
from wideband_tune_model import (M64, TUNE_GAP, creation, lo_index, model_inc32, model_ramp, schedule, seg_next, seg_phase, tri,
                                 wb_tuned_model, wbr_tuned_model, wbtx_tuned_model, wbtxr_tuned_model)

EINVAL = -1
D_EDGES = [0, 1, (1 << 31) - 1, (1 << 31) + 1, (1 << 32) - 1, (1 << 32) + 1, 1 << 63, (1 << 64) - 1]


def test_struct_layouts_and_constants(amd, tmp_path):
    check_ctypes_layout(tmp_path, amd.WbSeg, "opv_wb_seg", 32, ["start", "phase", "inc", "ramp"])
    check_ctypes_layout(tmp_path, amd.WbTune, "opv_wb_tune", 40, ["channel", "phase_given", "at", "centre_hz", "rate_hz_s", "phase"])
    text = (ROOT / "include" / "opv_demod.h").read_text()
    for name, value in (("OPV_WB_TUNE_GAP", "4096"), ("OPV_WB_TUNE_SEGS", "16"), ("OPV_WB_TUNE_MAX_RATE", "1.0e7")):
        assert f"#define {name}" in text and text.split(f"#define {name}")[1].split()[0] == value
    assert (amd.WB_TUNE_GAP, amd.WB_TUNE_SEGS, amd.WB_TUNE_MAX_RATE) == (4096, 16, 1.0e7)


# ------------------------------------------------------------------ opv_wb_seg_phase
def test_seg_phase_equals_the_model(amd):
    """d at the edges of 31, 32, 63 and 64 bits and random d of every width, ramps of both signs, an increment with the top bit set"""
    rng = np.random.default_rng(1)
    assert [tri(d) for d in (0, 1, 2, 3, 4, 5)] == [0, 0, 1, 3, 6, 10] and tri((1 << 64) - 1) == ((1 << 64) - 1) * ((1 << 63) - 1) % (1 << 64)
    for ramp in (38912345678901, -38912345678901, 1, -1, 0, (1 << 63) - 1, -(1 << 63)):
        for inc in (0xF000000100000000, 0x0000000100000000, M64):
            seg = (12345, 0x0123456789ABCDEF, inc, ramp)
            ds = D_EDGES + [int(rng.integers(0, 1 << 62)) >> int(rng.integers(0, 62)) for _ in range(8)]
            for d in ds:
                a = (seg[0] + d) & M64
                assert amd.wb_seg_phase(seg, a) == seg_phase(seg, a), (seg, d)
    # phi64(a + 1) - phi64(a) = inc + ramp x d: a frequency that moves linearly
    seg = (7, 99, 5 << 32, -3)
    for d in (0, 1, 1000, 1 << 33):
        assert (amd.wb_seg_phase(seg, 7 + d + 1) - amd.wb_seg_phase(seg, 7 + d)) & M64 == (seg[2] + seg[3] * d) & M64


# ------------------------------------------------------------------ opv_wb_seg_next
@pytest.mark.parametrize("down,up", [(4, 1), (1, 1), (16, 1), (1250, 271), (7680, 271), (625, 542)])
def test_seg_next_equals_the_model_and_the_plans_increment(amd, down, up):
    rng = np.random.default_rng(down + up)
    fw = down * WIDE_RATE / up
    taps = np.array([1], np.int16)
    prev = (0, 0, 0x12345678 << 32, 0)
    for _ in range(30):
        at = int(rng.integers(0, 1 << 45))
        f = float(rng.uniform(-fw / 2, fw / 2))
        r = float(rng.uniform(-1.0e7, 1.0e7)) if _ % 3 else 0.0
        got = amd.wb_seg_next(prev, down, up, at, f, r)
        assert got.astuple() == seg_next(prev, down, up, at, f, r), (at, f, r)
        assert got.inc >> 32 == int(amd.wbr_plan(down, up, [f], taps, 0)[0]) == int(wbr_model_inc(down, up, [f])[0]) and got.inc & 0xFFFFFFFF == 0
        if up == 1:
            assert got.inc >> 32 == int(amd.wb_plan(down, [f], taps, 0)[0]) == int(amd.wbtx_plan(down, [f], taps, 0)[0])
        assert got.phase == amd.wb_seg_phase(prev, at)                      # continuity
        prev = got.astuple()
    for rate in (1.0e7, -1.0e7):                                            # the largest ramp: what it is, and that it fits
        assert amd.wb_seg_next(prev, down, up, 0, 0.0, rate).ramp == model_ramp(down, up, rate)
    assert abs(model_ramp(1, 1, 1.0e7)) < 1 << 46
    for bad in (dict(f=np.nan), dict(f=np.inf), dict(r=np.nan), dict(r=-np.inf), dict(r=1.0000001e7), dict(r=-1.0000001e7), dict(down=0), dict(up=0)):
        with pytest.raises(amd.OpvError, match="opv error -1: opv_wb_seg_next"):
            amd.wb_seg_next(prev, bad.get("down", down), bad.get("up", up), 5, bad.get("f", 0.0), bad.get("r", 0.0))


def test_a_ramp_is_the_frequency_the_header_says():
    """from `at` on the channel sits at centre_hz + rate_hz_s x (a - at) / fw: the phase step of the model, in Hz, d samples in"""
    down, up, f, r = 1250, 271, 1.7e6, -4.0e5
    fw = down * WIDE_RATE / up
    seg = seg_next((0, 0, 0, 0), down, up, 1000, f, r)
    for d in (0, 10000, 3000000):
        step = (seg_phase(seg, 1000 + d + 1) - seg_phase(seg, 1000 + d)) & M64
        assert abs(step / 2.0 ** 64 * fw - (f + r * d / fw)) < 0.01


# ------------------------------------------------------------------ the scheduled models
def test_lo_index_in_uint64_equals_python_integers():
    segs = schedule(0xF2345678, 4, 1, [(3000, -1.1e6, 9.0e6), (3000 + TUNE_GAP, 2.0e6, -1.0e7)])
    for a0 in (0, 2999, (1 << 32) - 3000):
        segs_at = segs if a0 < 3000 else [segs[0]] + [seg_next(segs[0], 4, 1, a0 + 5, 1e5, -1e7), ]
        assert np.array_equal(lo_index(segs_at, a0, 9000), lo_index(segs_at, a0, 9000, exact=True))
    far = [(5, 1 << 63, (1 << 64) - (1 << 32), -(1 << 45))]
    assert np.array_equal(lo_index(far, (1 << 40) + 12345, 5000), lo_index(far, (1 << 40) + 12345, 5000, exact=True))
    assert lo_index(far, (1 << 40), 3)[1] == seg_phase(far[0], (1 << 40) + 1) >> 52


@pytest.mark.parametrize("first", [0, (1 << 32) - 700, (1 << 40) + 12345])
def test_creation_schedules_give_the_unscheduled_models(amd, first):
    """the new rule contains the old one: ((a inc << 32) mod 2^64) >> 52 == ((a inc) mod 2^32) >> 20, through all four models; and with
    up = 1 the two derivations of each side agree behind a schedule that moves"""
    rng = np.random.default_rng(3)
    T = amd.wb_lo_table()
    K, N = 3, 1500
    wide = rng.integers(-32768, 32768, 2 * N).astype(np.int16)
    chans = [rng.integers(-32768, 32768, 2 * 400).astype(np.int16) for _ in range(K)]
    # receive
    D, taps = 4, per_phase_taps(rng, 37, 1)
    inc = wb_model_inc(D, rng.uniform(-4e6, 4e6, K))
    assert np.array_equal(wb_tuned_model(T, wide, D, creation(inc), taps, 21, first), wb_model(T, wide, D, inc, taps, 21, first))
    M, U, rtaps = 7, 3, per_phase_taps(rng, 50, 3)
    inc_r = wbr_model_inc(M, U, rng.uniform(-2e6, 2e6, K))
    assert np.array_equal(wbr_tuned_model(T, wide, M, U, creation(inc_r), rtaps, 21, first), wbr_model(T, wide, M, U, inc_r, rtaps, 21, first))
    moving = [schedule(w, D, 1, [(first + 100 + 30 * k, 1e5 * (k - 1), (-1) ** k * 9.9e6), (first + 100 + TUNE_GAP, -7e5, 0.0)]) for k, w in enumerate(inc)]
    a, b = wb_tuned_model(T, wide, D, moving, taps, 21, first), wbr_tuned_model(T, wide, D, 1, moving, taps, 21, first)
    assert np.array_equal(a, b) and not np.array_equal(a, wb_model(T, wide, D, inc, taps, 21, first))
    # transmit
    ttaps = tx_phase_taps(rng, 37, D)
    assert np.array_equal(wbtx_tuned_model(T, chans, D, creation(inc), ttaps, 31, first), wbtx_model(T, chans, D, inc, ttaps, 31, first))
    rt = tx_phase_taps(rng, 50, M)
    assert np.array_equal(wbtxr_tuned_model(T, chans, M, U, creation(inc_r), rt, 31, first), wbtxr_model(T, chans, M, U, inc_r, rt, 31, first))
    a, b = wbtx_tuned_model(T, chans, D, moving, ttaps, 31, first), wbtxr_tuned_model(T, chans, D, 1, moving, ttaps, 31, first)
    assert np.array_equal(a, b) and not np.array_equal(a, wbtx_model(T, chans, D, inc, ttaps, 31, first))


# ------------------------------------------------------------------ the rules under ASan + UBSan, as a stand-alone program
def parse_segs(line):
    tag, n, *rest = line.split()
    segs = [tuple(int(v) for v in s.split(":")) for s in rest]
    assert len(segs) == int(n)
    return segs


def test_tune_rules_under_sanitizers(tmp_path):
    """tests/san_tune/: csrc/opv_wb_rules.cpp linked into a program with its own main, once with -fsanitize=address,undefined and once
    plain. By itself it holds a segment's phase to 128-bit arithmetic, walks every refusal of opv_wb_seg_next and of a retune
    (OPV_EINVAL for a channel out of range, a centre or rate that is not finite, a rate above the limit, two entries of a channel
    inside the gap or out of order, a null pointer, count < 0; OPV_ESTATE for the past; OPV_ECAPACITY for the 17th segment) and
    asserts that the lists are what they were, prunes by the receive and by the transmit rule, and holds the per-push device table,
    evaluated as the kernels evaluate it, to the absolute formula (origins in front of sample 0, across 2^32, on and beside
    every boundary). The sanitized build reports nothing, exits 0 and prints what the plain build prints; the phases and segments it
    prints are the model's."""
    out_dir = tmp_path / "san_tune"
    p = subprocess.run(["make", "-C", str(ROOT / "tests" / "san_tune"), f"OUT={out_dir}"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    env = dict(ASAN_OPTIONS="exitcode=99:detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")
    outs = []
    for exe in ("tune_rules_san", "tune_rules_plain"):
        r = subprocess.run([str(out_dir / exe)], capture_output=True, text=True, env=env)
        assert r.returncode == 0 and not r.stderr, (exe, r.returncode, r.stdout[-2000:], r.stderr[-3000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1]
    lines = outs[0].splitlines()
    assert lines[-1] == "failures 0" and not any(ln.startswith("MISS") for ln in lines)
    # ---- what it printed against the model
    phases = [ln.split() for ln in lines if ln.startswith("phase ")]
    assert len(phases) == 2 * len(D_EDGES)
    for _, sign, d, got in phases:
        seg = (12345, 0x0123456789ABCDEF, 0xF000000100000000, int(sign) * 38912345678901)
        assert int(got) == seg_phase(seg, (12345 + int(d)) & M64), (sign, d)
    nxt = [ln.split() for ln in lines if ln.startswith("next ")][0]
    assert tuple(int(v) for v in nxt[1:]) == seg_next((0, 0, 0x12345678 << 32, 0), 1250, 271, 100000, -3.1e6, -2.5e5)[1:]
    A, inc = (1 << 32) - 3000, [0x10000000, 0xF0000000]
    named = {ln.split()[0]: parse_segs(ln) for ln in lines if ln.split()[0] in ("segs0", "segs1", "rx1", "tx1")}
    ch0 = schedule(inc[0], 4, 1, [(A, -2.2e6, -3e5)])
    assert named["segs0"] == ch0[1:]                                        # the tune at the object's first sample replaced the creation segment
    ch1 = schedule(inc[1], 4, 1, [(A + 777, 1.5e6, 4e5), (A + 777 + TUNE_GAP, 1.4e6, 0.0), (A + 777 + 2 * TUNE_GAP, -1.4e6, -1e7)])
    assert named["segs1"] == ch1
    assert named["rx1"] == ch1[2:] and named["tx1"] == ch1[2:]
    assert ch1[1][2] >> 32 == model_inc32(4, 1, 1.5e6)
