"""CPU-only: the host half of the wideband scan (include/opv_demod.h, opv_scan_plan / opv_scan_blocks / opv_scan_carriers; the
rules are csrc/opv_scan_rules.cpp) against tests/scan_model.py, the model against a literal restatement of the header's arithmetic,
the same rules as a stand-alone program under ASan + UBSan (tests/san_scan/), and the CPU half of the end-to-end plan of
tests/test_gpu_scan.py (tests/scan_inputs.py): its preconditions, asserted on the models and the oracle alone."""
import ctypes as C
import subprocess

import numpy as np
import pytest

from amd_lib import ROOT
from fixtures_built import amd  # noqa: F401
from scan_inputs import (SCAN_PLAN, carrier_cases, door_streams_on_the_cpu, make_scan_capture, scan_plan_carriers, scan_plan_rows_model)
from scan_model import carriers_model, hann_window, scan_blocks, scan_model, scan_shape
from struct_layout import check_ctypes_layout
from wideband_models import WIDE_RATE, wb_model_inc, wbr_model_inc

EINVAL = -1


# ------------------------------------------------------------------ the model against a literal restatement
@pytest.mark.parametrize("Lw,H,A,S", [(5, 3, 2, 4), (4, 4, 1, 0), (3, 7, 3, 24)])
def test_model_agrees_with_a_literal_restatement(amd, Lw, H, A, S):
    """mix, window, sum, shift, clamp, square, add: in python integers, one product at a time"""
    rng = np.random.default_rng(10 * Lw + H)
    T = amd.wb_lo_table()
    first, N = (1 << 32) - 11, 61
    wide = rng.integers(-32768, 32768, 2 * N).astype(np.int16)
    window = rng.integers(-3000, 3000, Lw).astype(np.int16)
    inc = wbr_model_inc(7, 4, [250000.0, -1234567.0, 0.0])
    got = scan_model(T, wide, inc, window, H, A, S, first)
    segs = (N - Lw) // H + 1
    assert got.shape == (segs // A, 3) and got.dtype == np.uint64 and segs // A >= 2
    clamped = 0
    for p, w in enumerate(inc):
        for b in range(segs // A):
            total = 0
            for sg in range(b * A, b * A + A):
                z = [0, 0]
                for t in range(Lw):
                    n = sg * H + t
                    i = (((first + n) * int(w)) & 0xFFFFFFFF) >> 20
                    c, s = int(T[i]), int(T[(i - 1024) & 4095])
                    x, y = int(wide[2 * n]), int(wide[2 * n + 1])
                    z[0] += int(window[t]) * (x * c + y * s)
                    z[1] += int(window[t]) * (y * c - x * s)
                y2 = [min(max((v + ((1 << (S - 1)) if S else 0)) // (1 << S), -(1 << 24)), (1 << 24) - 1) for v in z]   # python's // is floor
                clamped += sum(abs(v) >= (1 << 24) - 1 for v in y2)
                total += y2[0] ** 2 + y2[1] ** 2
            assert int(got[b, p]) == total, (p, b)
    assert (clamped > 0) == (S < 24)                                        # (|z| < 3 x 3000 x 2^31: S = 24 keeps it inside 25 bits)


# ------------------------------------------------------------------ opv_scan_plan
def plan_rc(amd, cfg=None, probes=(1000.0, -1000.0), window=None, inc=True, **kw):
    a = dict(down=7, up=4, n_probes=len(probes) if probes is not None else 1, n_window=9, hop=5, n_avg=3, out_shift=5, ring_blocks=2, first_sample=0)
    a.update(kw)
    c = amd.ScanCfg(**a)
    if not isinstance(window, str):                                         # ("null": no window at all)
        window = np.ones(max(a["n_window"], 1), np.int16) if window is None else np.ascontiguousarray(window, np.int16)
    probes = None if probes is None else np.ascontiguousarray(probes, np.float64)
    out = np.zeros(1100, np.uint32)
    return amd.lib().opv_scan_plan(None if cfg == "null" else C.byref(c), None if probes is None else probes.ctypes.data,
                                   None if isinstance(window, str) else window.ctypes.data, out.ctypes.data if inc else None)


@pytest.mark.parametrize("M,U", [(1, 1), (4, 1), (16, 1), (32, 1), (625, 542), (1250, 271), (7680, 271), (1025, 1024)])
def test_plan_increments_equal_the_rational_doors(amd, M, U):
    fw = M * WIDE_RATE / U
    probes = [100000.0, 1.0, 54200.0 * 7, -100000.0, -1.0, -fw / 4, 0.0, -0.0, 1e5 / 3, 12345.678901, np.pi * 1e4,
              fw / 2, -fw / 2, 0.75 * fw, -0.75 * fw, 3 * fw + 5000.0, -7 * fw - 5000.0, fw, 1e12]
    got = amd.scan_plan(M, U, probes, [1, 2, 3], 2, 1, 0)
    assert got.dtype == np.uint32 and np.array_equal(got, wbr_model_inc(M, U, probes))
    assert np.array_equal(got, amd.wbr_plan(M, U, probes, [1, 2, 3], 0))
    if U == 1:
        assert np.array_equal(got, wb_model_inc(M, probes))
        if M <= 16:
            assert np.array_equal(got, amd.wb_plan(M, probes, [1, 2, 3], 0))
    grid = -fw / 2 + fw / 1024 * np.arange(1024)                            # a full bank
    assert np.array_equal(amd.scan_plan(M, U, grid, hann_window(1024), 1024, 1, 22), wbr_model_inc(M, U, grid))


def test_plan_refuses_one_step_outside_every_limit_and_accepts_the_edge(amd):
    def rc(**kw):
        return plan_rc(amd, **kw)
    assert rc() == 0
    # down and up: opv_wbr_plan's
    assert rc(up=0, down=1) == EINVAL and rc(up=1025, down=1026) == EINVAL and rc(up=1024, down=1025) == 0 and rc(up=1, down=1) == 0
    assert rc(down=2, up=3) == EINVAL and rc(down=33, up=1) == EINVAL and rc(down=32, up=1) == 0 and rc(down=0, up=1) == EINVAL
    assert rc(down=6, up=4) == EINVAL and rc(down=542, up=271) == EINVAL
    # P
    assert rc(probes=np.zeros(1024)) == 0 and rc(probes=np.zeros(1025)) == EINVAL and rc(probes=[5.0]) == 0
    assert rc(probes=[5.0], n_probes=0) == EINVAL and rc(probes=[5.0], n_probes=-1) == EINVAL
    # Lw, H, A
    assert rc(n_window=0) == EINVAL and rc(n_window=1) == 0 and rc(n_window=4096) == 0 and rc(n_window=4097) == EINVAL
    assert rc(hop=0) == EINVAL and rc(hop=1) == 0 and rc(hop=65536, n_avg=1) == 0 and rc(hop=65537, n_avg=1) == EINVAL
    assert rc(n_avg=0) == EINVAL and rc(n_avg=1) == 0 and rc(n_avg=4096, hop=1) == 0 and rc(n_avg=4097, hop=1) == EINVAL
    # the block span (A - 1) H + Lw: exactly 2^20 and one more
    assert rc(n_avg=1025, hop=1023, n_window=1024) == 0 and 1024 * 1023 + 1024 == 1 << 20
    assert rc(n_avg=1025, hop=1023, n_window=1025) == EINVAL
    assert rc(n_avg=17, hop=65536, n_window=1) == EINVAL and rc(n_avg=16, hop=65536, n_window=4096) == 0
    assert rc(n_avg=4096, hop=256, n_window=256) == 0 and rc(n_avg=4096, hop=256, n_window=257) == EINVAL
    # S, the ring
    assert rc(out_shift=-1) == EINVAL and rc(out_shift=0) == 0 and rc(out_shift=40) == 0 and rc(out_shift=41) == EINVAL
    assert rc(ring_blocks=0) == EINVAL and rc(ring_blocks=1) == 0 and rc(ring_blocks=4096) == 0 and rc(ring_blocks=4097) == EINVAL
    # the window's gain: exactly 2^21 and one more
    full = np.full(64, -32768, np.int16)
    assert np.abs(full.astype(np.int64)).sum() == 1 << 21 and rc(n_window=64, window=full) == 0
    assert rc(n_window=65, window=np.concatenate([full, [1]])) == EINVAL and rc(n_window=65, window=np.concatenate([full, [-1]])) == EINVAL
    assert rc(n_window=65, window=np.concatenate([full, [0]])) == 0
    # the probes, the pointers
    for bad in (np.nan, np.inf, -np.inf):
        assert rc(probes=[1000.0, bad]) == EINVAL, bad
    assert rc(probes=None) == EINVAL and rc(window="null") == EINVAL and rc(inc=False) == EINVAL and rc(cfg="null") == EINVAL
    assert b"opv_scan" in amd.lib().opv_last_error()
    with pytest.raises(amd.OpvError):
        amd.scan_plan(6, 4, [0.0], [1], 1, 1, 0)


def test_struct_layouts_match_the_header(amd, tmp_path):
    offsets = check_ctypes_layout(tmp_path, amd.ScanCfg, "opv_scan_cfg", 40,
                                  ["down", "up", "n_probes", "n_window", "hop", "n_avg", "out_shift", "ring_blocks", "first_sample"])
    assert offsets["first_sample"] == 32
    offsets = check_ctypes_layout(tmp_path, amd.ScanCarrier, "opv_scan_carrier", 24, ["centre_hz", "excess", "probe", "reserved"])
    assert offsets["probe"] == 16


# ------------------------------------------------------------------ opv_scan_blocks
BLOCK_SHAPES = [(1024, 1024, 64), (1024, 512, 3), (7, 2000, 3), (7, 2000, 1), (4096, 1, 4096), (1, 1, 1), (1, 65536, 16), (300, 299, 5)]   # (Lw, H, A)


def blocks_edge_counts(Lw, H, A):
    """N around every boundary: the first segment, every block's last sample (+/- 1), far out and near 2^63"""
    span, stride = (A - 1) * H + Lw, A * H
    ns = {0, 1, Lw - 1, Lw, Lw + 1, Lw + H - 1, Lw + H}
    for b in (0, 1, 2, 7, 1 << 20):
        ns |= {b * stride + span - 1, b * stride + span, b * stride + span + 1}
    for far in ((1 << 31), (1 << 32) + 1, (1 << 62) + 12345, (1 << 63) - 1, 1 << 63):
        ns |= {far, far - far % stride + span - 1, far - far % stride + span}
    return sorted(n for n in ns if n >= 0)


@pytest.mark.parametrize("Lw,H,A", BLOCK_SHAPES)
def test_blocks_equal_the_model_around_every_boundary(amd, Lw, H, A):
    span, stride = (A - 1) * H + Lw, A * H
    for N in blocks_edge_counts(Lw, H, A):
        assert amd.scan_blocks(Lw, H, A, N) == scan_blocks(Lw, H, A, N), N
    for b in (0, 1, 5):                                                     # a block exists exactly from its last sample on
        assert amd.scan_blocks(Lw, H, A, b * stride + span - 1) == b and amd.scan_blocks(Lw, H, A, b * stride + span) == b + 1
    L = amd.lib()
    assert L.opv_scan_blocks(None, 5000) == 0
    for bad in (amd.ScanCfg(6, 4, 1, 4, 4, 1, 0, 1, 0), amd.ScanCfg(1, 1, 1, 0, 4, 1, 0, 1, 0), amd.ScanCfg(1, 1, 1, 4, 0, 1, 0, 1, 0), amd.ScanCfg(1, 1, 1, 4, 4, 0, 0, 1, 0)):
        assert L.opv_scan_blocks(C.byref(bad), 5000) == 0


# ------------------------------------------------------------------ opv_scan_carriers
CASES = {c[0]: c for c in carrier_cases()}


@pytest.mark.parametrize("name", list(CASES))
def test_carriers_equal_the_model_bit_for_bit(amd, name):
    _, row, f0, step, hw, ratio, cap = CASES[name]
    got, exp = amd.scan_carriers(row, f0, step, hw, ratio, cap), carriers_model(row, f0, step, hw, ratio, cap)
    assert len(got) == len(exp) <= cap
    for g, e in zip(got, exp):
        assert g[1] == e[1] and g[0].hex() == e[0].hex() and g[2].hex() == e[2].hex(), (g, e)
    # what each made row is there for. (Every box that holds a whole peak ties with its neighbours that do: `probe` is the lowest
    # such index, not the peak's, and the centroid finds the peak from there.)
    probes, at = [e[1] for e in exp], [(e[0] - f0) / step for e in exp]
    if name == "tie_in_box":
        assert probes == [20, 70] and abs(at[0] - 21) < 1e-9 and abs(at[1] - 71) < 1e-9 and exp[0][2] == exp[1][2]     # equal boxes: the lower index first
    if name == "both_ends":
        assert [round(x) for x in at[:2]] == [63, 0]
    if name == "flat_strict":
        assert exp == []
    if name == "flat_loose":
        assert probes == [3, 10, 17, 24, 31] and all(e[2] == 0.0 and e[0] == f0 + e[1] * step for e in exp)      # the first whole box, then every 2 W + 1
    if name == "floor_zero":
        assert sorted(row)[len(row) // 2] == 0 and round(at[0]) == 11 and abs(at[1] - 150.5) < 1e-9
    if name == "floor_zero_all":
        assert len(exp) == 3 and round(at[2]) == 199                        # every probe with power in reach is a candidate; 2 W apart
    if name in ("ratio_256", "ratio_0"):
        assert round(at[0]) == 40 and len(exp) > 1
    if name == "closer_than_2w":
        assert len(exp) == 2 and 50 < at[0] < 55 and round(at[1]) == 90    # the two share a box: one carrier between them
    if name == "cap_1":
        assert len(exp) == 1
    if name == "cap_0":
        assert exp == []
    if name == "near_2_61":
        assert min(row) > 1 << 60 and len(exp) >= 1
    if name == "w_beyond_row":
        assert len(exp) == 1 and probes == [0]


def test_carriers_refuses_bad_arguments(amd):
    L = amd.lib()
    row = np.arange(10, dtype=np.uint64)
    out = (amd.ScanCarrier * 4)()

    def rc(P=10, f0=0.0, step=10.0, hw=20.0, r=row.ctypes.data, o=out, cap=4):
        return L.opv_scan_carriers(r, P, f0, step, hw, 300, o, cap)
    assert rc() >= 0
    assert rc(P=0) == EINVAL and rc(P=-1) == EINVAL and rc(P=1025) == EINVAL
    for bad in (0.0, -1.0, np.nan, np.inf):
        assert rc(step=bad) == EINVAL, bad
    for bad in (-1.0, np.nan, np.inf):
        assert rc(hw=bad) == EINVAL, bad
    assert rc(f0=np.nan) == EINVAL and rc(r=None) == EINVAL and rc(o=None) == EINVAL and rc(o=None, cap=0) == 0
    assert b"opv_scan_carriers" in L.opv_last_error()


# ------------------------------------------------------------------ the same rules under ASan + UBSan, as a stand-alone program
def test_scan_rules_under_sanitizers(tmp_path):
    """tests/san_scan/: csrc/opv_scan_rules.cpp and csrc/opv_wb_rules.cpp linked into a program with its own main, once with
    -fsanitize=address,undefined and once plain. It walks the limits of the plan at and one step outside every edge, the block
    count and a push's plan over the shapes and counts of this module (and over every split of short captures: the blocks of the
    pieces add up, the carry is what the next block needs and stays below the span), the launch shape, and opv_scan_carriers over
    this module's rows, read from a file, and it prints the launch shape for a grid of (P, A, blocks), which is held to scan_model.scan_shape. The sanitized build reports nothing, exits 0 and prints what the plain build prints;
    the carriers it prints are carriers_model's, bit for bit."""
    out_dir = tmp_path / "san_scan"
    p = subprocess.run(["make", "-C", str(ROOT / "tests" / "san_scan"), f"OUT={out_dir}"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    rows = tmp_path / "rows.txt"
    with open(rows, "w") as f:
        for name, row, f0, step, hw, ratio, cap in CASES.values():
            f.write(" ".join([name, float(f0).hex(), float(step).hex(), float(hw).hex(), str(ratio), str(cap), str(len(row))] + [str(int(v)) for v in row]) + "\n")
    shapes = tmp_path / "shapes.txt"
    with open(shapes, "w") as f:
        for Lw, H, A in BLOCK_SHAPES:
            f.write(" ".join(map(str, [Lw, H, A] + blocks_edge_counts(Lw, H, A))) + "\n")
    env = dict(ASAN_OPTIONS="exitcode=99:detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")
    outs = []
    for exe in ("scan_rules_san", "scan_rules_plain"):
        q = subprocess.run([str(out_dir / exe), str(rows), str(shapes)], capture_output=True, text=True, env=env, timeout=300)
        assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (exe, q.returncode, q.stderr[-3000:])
        outs.append(q.stdout.splitlines())
    assert outs[0] == outs[1]
    lines = {ln.split()[0]: ln.split()[1:] for ln in outs[0]}
    for name, row, f0, step, hw, ratio, cap in CASES.values():
        exp = carriers_model(row, f0, step, hw, ratio, cap)
        tok = lines["carriers:" + name]
        assert tok[0] == str(len(exp)) and len(tok) == 1 + 3 * len(exp), name
        for k, e in enumerate(exp):                                         # (printf's %a and float.hex spell the same double differently)
            assert tok[1 + 3 * k] == str(e[1]) and float.fromhex(tok[2 + 3 * k]).hex() == e[0].hex() and float.fromhex(tok[3 + 3 * k]).hex() == e[2].hex(), (name, k)
    for Lw, H, A in BLOCK_SHAPES:
        assert lines[f"blocks:{Lw}:{H}:{A}"] == [str(scan_blocks(Lw, H, A, N)) for N in blocks_edge_counts(Lw, H, A)]
    assert int(lines["plans"][0]) >= 39 and int(lines["splits"][0]) > 10000
    # the launch shape as the GPU cases' preconditions restate it
    shapes = {k: v for k, v in lines.items() if k.startswith("shape:")}
    assert len(shapes) == 7 * 9 * 13
    for k, v in shapes.items():
        _, P, A, blocks = k.split(":")
        assert tuple(map(int, v)) == scan_shape(int(P), int(A), int(blocks)), k


# ------------------------------------------------------------------ the end-to-end plan's CPU half
def test_end_to_end_plan_holds_on_the_cpu_alone(amd, oracle):
    """the preconditions of test_gpu_scan.py's end-to-end case, from the models and the oracle alone: carriers_model on scan_model's
    rows finds all three carriers within 1000 Hz; the oracle on wb_model at the found centres decodes every transmitted frame;
    and the control - the oracle on wb_model at the NOMINAL centres releases no frame on the channel whose carrier sits 15 250 Hz
    off (at +11 250 and +13 250 Hz it still released frames, wrong ones: the offset search saturates at its edge and the tracker
    false-alarms; 15 250 Hz is the first 2 kHz step at which it releases none)."""
    cap = make_scan_capture(amd)
    found = scan_plan_carriers(scan_plan_rows_model(amd, cap["wide"]))
    assert len(found) == 3
    errs = [f[0] - t for f, t in zip(found, cap["true_hz"])]
    assert max(map(abs, errs)) < 1000.0, errs
    assert max(abs(o) for o in SCAN_PLAN["off_hz"]) > 1500.0
    _, exp = door_streams_on_the_cpu(amd, oracle, cap["wide"], [f[0] for f in found])
    for k in range(3):
        assert np.array_equal(exp[k]["frames"], cap["tx"][k]) and len(exp[k]["frames"]) == SCAN_PLAN["frames"], k
    _, ctl = door_streams_on_the_cpu(amd, oracle, cap["wide"], SCAN_PLAN["centres"])
    assert len(ctl[2]["frames"]) == 0
