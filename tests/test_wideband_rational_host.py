"""CPU-only: the host half of the rational wideband front door (include/opv_demod.h, opv_wbr_plan / opv_wbr_outputs /
opv_wb_create_rational; the rules are csrc/opv_wb_rules.cpp) against a numpy int64 restatement of the header's arithmetic. The
model is tests/wideband_models.py (wbr_model_inc, wbr_outputs, wbr_model), and tests/test_gpu_wideband_rational.py holds the device
to the same functions with ==."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

from fixtures_built import amd  # noqa: F401
from struct_layout import check_ctypes_layout
from wideband_models import WIDE_RATE, per_phase_taps, wb_model, wb_model_inc, wbr_model, wbr_model_inc

EINVAL = -1


# ------------------------------------------------------------------ the model against a literal restatement, and against the integer door's
@pytest.mark.parametrize("M,U,L", [(3, 2, 5), (7, 4, 9), (5, 1, 4)])
def test_model_agrees_with_a_literal_zero_stuff_filter_decimate(amd, M, U, L):
    """zero-stuff m by U, the full FIR with `taps`, keep every M-th: in python integers, one product at a time"""
    rng = np.random.default_rng(100 * M + U)
    T = amd.wb_lo_table()
    S, first, N = 4, (1 << 32) - 7, 37
    wide = rng.integers(-32768, 32768, 2 * N).astype(np.int16)
    taps = rng.integers(-20000, 20000, L).astype(np.int16)
    inc = wbr_model_inc(M, U, [250000.0, -1234567.0])
    got = wbr_model(T, wide, M, U, inc, taps, S, first)
    n_out = -(-N * U // M)
    assert got.shape == (2, 2 * n_out)
    for k, w in enumerate(inc):
        z = [(0, 0)] * (N * U)
        for n in range(N):
            phi = ((first + n) * int(w)) & 0xFFFFFFFF
            i = phi >> 20
            c, s = int(T[i]), int(T[(i - 1024) & 4095])
            x, y = int(wide[2 * n]), int(wide[2 * n + 1])
            z[n * U] = (x * c + y * s, y * c - x * s)
        for r in range(n_out):
            assert r * M < N * U
            for comp in (0, 1):
                acc = sum(int(taps[t]) * z[r * M - t][comp] for t in range(L) if r * M - t >= 0)
                v = (acc + (1 << (S - 1))) // (1 << S)                      # python's // is floor
                assert got[k, 2 * r + comp] == min(max(v, -32768), 32767), (k, r, comp)
    assert (got == 32767).any() and (got == -32768).any()


@pytest.mark.parametrize("D,L,S,N", [(4, 143, 33, 2403), (3, 2, 21, 2101), (16, 1024, 36, 7205), (1, 1, 0, 500)])
def test_up_1_is_the_integer_doors_model(amd, D, L, S, N):
    rng = np.random.default_rng(D * 1000 + L)
    T = amd.wb_lo_table()
    first = (1 << 32) - 1000
    centres = list(rng.uniform(-D * WIDE_RATE / 2, D * WIDE_RATE / 2, 3))
    inc = wbr_model_inc(D, 1, centres)
    assert np.array_equal(inc, wb_model_inc(D, centres))
    wide = rng.integers(-32768, 32768, 2 * N).astype(np.int16)
    taps = per_phase_taps(rng, L, 1) if L > 1 else np.array([3], np.int16)
    if S == 0:
        wide = rng.integers(-9, 10, 2 * N).astype(np.int16)
    a, b = wbr_model(T, wide, D, 1, inc, taps, S, first), wb_model(T, wide, D, inc, taps, S, first)
    assert a.shape == b.shape and np.array_equal(a, b)
    assert (np.abs(a.astype(np.int32)) < 32767).any()


# ------------------------------------------------------------------ opv_wbr_plan
def plan_rc(amd, down, up, K, L, S, centre, taps, reserved=0, inc=True, cfg=True, out=None):
    c = amd.WbrCfg(down, up, K, L, S, reserved, 0)
    centre = None if centre is None else np.ascontiguousarray(centre, np.float64)
    taps = None if taps is None else np.ascontiguousarray(taps, np.int16)
    out = np.zeros(300, np.uint32) if out is None else out
    return amd.lib().opv_wbr_plan(C.byref(c) if cfg else None, None if centre is None else centre.ctypes.data,
                                  None if taps is None else taps.ctypes.data, out.ctypes.data if inc else None)


@pytest.mark.parametrize("M,U", [(1, 1), (625, 542), (1250, 271), (7680, 271), (32, 1), (1025, 1024)])
def test_plan_increments_equal_the_model(amd, M, U):
    fw = M * WIDE_RATE / U
    centre = [100000.0, 1.0, 54200.0 * 7, -100000.0, -1.0, -fw / 4, 0.0, -0.0,
              1e5 / 3, 12345.678901, np.pi * 1e4,
              fw / 2, -fw / 2, 0.75 * fw, -0.75 * fw, 3 * fw + 5000.0, -7 * fw - 5000.0, fw, 1e12]          # beyond +/-Fw/2: wraps
    got = amd.wbr_plan(M, U, centre, [1, 2, 3], 0)
    exp = wbr_model_inc(M, U, centre)
    assert got.dtype == np.uint32 and np.array_equal(got, exp), (got, exp)
    k = {f: j for j, f in enumerate(centre)}
    assert got[k[0.0]] == 0 and int(got[k[100000.0]]) + int(got[k[-100000.0]]) == 1 << 32        # a negative centre wraps
    if U == 1:
        assert np.array_equal(got, wb_model_inc(M, centre))
        if M <= 16:
            assert np.array_equal(got, amd.wb_plan(M, centre, [1, 2, 3], 0))


def test_plan_refuses_what_lies_outside_the_limits(amd):
    ok = dict(down=7, up=4, K=2, L=9, S=5, centre=[1000.0, -1000.0], taps=[100, -200, 100, 7, 7, 7, 7, 7, 7], reserved=0)

    def rc(**kw):
        a = dict(ok, **kw)
        taps = a["taps"]
        if taps is not None and len(taps) != a["L"]:
            taps = np.ones(max(a["L"], 1), np.int16)
        return plan_rc(amd, a["down"], a["up"], a["K"], a["L"], a["S"], a["centre"], taps, a["reserved"], a.get("inc", True), a.get("cfg", True))
    assert rc() == 0
    # up: 1 .. 1024
    assert rc(up=0, down=1) == EINVAL and rc(up=-1, down=1) == EINVAL and rc(up=1025, down=1026) == EINVAL
    assert rc(up=1, down=1) == 0 and rc(up=1024, down=1025) == 0
    # up <= down <= 32 up
    assert rc(down=2, up=3) == EINVAL and rc(down=4, up=3) == 0 and rc(down=0, up=1) == EINVAL and rc(down=-5, up=1) == EINVAL
    assert rc(down=33, up=1) == EINVAL and rc(down=32, up=1) == 0
    assert rc(down=65, up=2) == EINVAL and rc(down=63, up=2) == 0
    assert rc(down=32 * 1024 + 1, up=1024) == EINVAL and rc(down=32 * 1024 - 1, up=1024) == 0
    # lowest terms
    assert rc(down=6, up=4) == EINVAL and rc(down=3, up=3) == EINVAL and rc(down=542, up=271) == EINVAL and rc(down=7, up=4) == 0
    # 1 <= n_taps, J <= 1024
    assert rc(L=0) == EINVAL and rc(L=-1) == EINVAL and rc(L=1) == 0
    assert rc(down=1, up=1, L=1024) == 0 and rc(down=1, up=1, L=1025) == EINVAL
    assert rc(down=4, up=3, L=3 * 1024) == 0 and rc(down=4, up=3, L=3 * 1024 + 1) == EINVAL
    for K in (0, -3, 257):
        assert rc(K=K, centre=np.zeros(300)) == EINVAL, K
    assert rc(K=1, centre=[5.0]) == 0 and rc(K=256, centre=np.zeros(256)) == 0
    for S in (-1, 41, 64):
        assert rc(S=S) == EINVAL, S
    assert rc(S=0) == 0 and rc(S=40) == 0
    assert rc(reserved=1) == EINVAL and rc(reserved=-1) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        assert rc(centre=[1000.0, bad]) == EINVAL, bad
    assert rc(centre=None) == EINVAL and rc(taps=None) == EINVAL and rc(inc=False) == EINVAL and rc(cfg=False) == EINVAL
    assert b"opv_wbr" in amd.lib().opv_last_error()
    with pytest.raises(amd.OpvError):
        amd.wbr_plan(6, 4, [0.0], [1], 0)


def test_the_tap_cap_holds_per_phase(amd):
    """sum_j |taps[p + j U]| <= 2^21 for EVERY phase p, and nothing is asked of the sum over all taps"""
    U, M = 64, 65
    full = np.full(64 * U, -32768, np.int16)                               # every phase: 64 x 32768 = 2^21 exactly; all taps: 2^27

    def rc(taps):
        return plan_rc(amd, M, U, 1, len(taps), 40, [0.0], taps)
    assert np.abs(full.astype(np.int64)).sum() == 1 << 27 and rc(full) == 0
    for p in (0, 5, 63):
        extra = np.zeros(p + 1, np.int16)
        assert rc(np.concatenate([full, extra])) == 0                      # a ragged last row of zeros
        extra[p] = 1
        assert rc(np.concatenate([full, extra])) == EINVAL, p               # phase p alone at 2^21 + 1
        extra[p] = -1
        assert rc(np.concatenate([full, extra])) == EINVAL, p
    pos = np.full(64 * U, 32767, np.int16)                                 # every phase 64 short of the cap
    for p in (0, 63):
        extra = np.zeros(p + 1, np.int16)
        extra[p] = 64
        assert rc(np.concatenate([pos, extra])) == 0
        extra[p] = 65
        assert rc(np.concatenate([pos, extra])) == EINVAL
    # U = 1: the present door's rule on the whole filter
    assert plan_rc(amd, 4, 1, 1, 64, 0, [0.0], np.full(64, -32768, np.int16)) == 0
    assert plan_rc(amd, 4, 1, 1, 65, 0, [0.0], np.concatenate([np.full(64, -32768, np.int16), [1]])) == EINVAL


# ------------------------------------------------------------------ opv_wbr_outputs
def test_outputs_is_ceil_n_u_over_m_at_the_edges(amd):
    for M, U in ((1, 1), (3, 2), (7, 4), (625, 542), (1250, 271), (7680, 271), (32, 1), (1025, 1024), (32767, 1024)):
        assert gcd(M, U) == 1
        for N in (0, 1, 2, M - 1, M, M + 1, 2 * M - 1, 2 * M, 2 * M + 1, 271 * M - 1, 271 * M, 271 * M + 1, 86720, 50001,
                  (1 << 31) - 1, 1 << 31, (1 << 32) + 1, (1 << 40) + 7, (1 << 63) + 5, (1 << 64) - 1):
            assert amd.wbr_outputs(M, U, N) == -(-N * U // M), (M, U, N)
        prev = 0
        for N in range(0, 3 * M + 5 if M < 2000 else 400):
            got = amd.wbr_outputs(M, U, N)
            assert got == -(-N * U // M) and 0 <= got - prev <= 1, (M, U, N)        # never decreases, steps by at most 1 (down >= up)
            prev = got
    assert amd.wbr_outputs(7680, 271, (1 << 63) + 5) == -(-((1 << 63) + 5) * 271 // 7680)
    L = amd.lib()
    assert L.opv_wbr_outputs(None, 5) == 0
    for bad in (amd.WbrCfg(0, 1, 1, 1, 0, 0, 0), amd.WbrCfg(2, 3, 1, 1, 0, 0, 0), amd.WbrCfg(6, 4, 1, 1, 0, 0, 0), amd.WbrCfg(33, 1, 1, 1, 0, 0, 0),
                amd.WbrCfg(7, 4, 1, 1, 0, 1, 0), amd.WbrCfg(7, 0, 1, 1, 0, 0, 0)):
        assert L.opv_wbr_outputs(C.byref(bad), 5) == 0
    assert L.opv_wbr_outputs(C.byref(amd.WbrCfg(7, 4, 1, 1, 0, 0, 0)), 5) == 3


def test_wbr_cfg_layout_matches_header(amd, tmp_path):
    """size and field offsets of the ctypes mirror against what gcc makes of include/opv_demod.h (as test_wb_cfg_layout_matches_header)"""
    offsets = check_ctypes_layout(tmp_path, amd.WbrCfg, "opv_wbr_cfg", 32, ["down", "up", "n_channels", "n_taps", "out_shift", "reserved", "first_sample"])
    assert offsets["first_sample"] == amd.WbrCfg.first_sample.offset == 24
