"""CPU-only: the host half of the rational up-converter bank (include/opv_demod.h, opv_wbtxr_plan / opv_wbtxr_outputs /
opv_wbtx_create_rational; the rules are csrc/opv_wb_rules.cpp) against a numpy int64 restatement of the header's arithmetic.
The model is tests/wideband_models.py (wbtxr_outputs, wbtxr_model), and tests/test_gpu_wideband_tx_rational.py holds the device to
it with ==. The increment rule is the rational door's (opv_wbr_plan): one definition serves both directions."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

from fixtures_built import amd  # noqa: F401
from struct_layout import check_ctypes_layout
from wideband_models import WIDE_RATE, wb_model_inc, wbr_model_inc, wbtx_model, wbtxr_model, wbtxr_outputs

EINVAL = -1
MAX_INPUTS = 1 << 50


# ------------------------------------------------------------------ the model against a literal restatement, and against the integer bank's
@pytest.mark.parametrize("M,U,L", [(3, 2, 5), (7, 4, 9), (5, 1, 4)])
def test_model_agrees_with_a_literal_zero_stuff_filter_keep(amd, M, U, L):
    """zero-stuff x by M, the full FIR with `taps`, keep every U-th, mix, sum, round, clamp: in python integers, one product at a
    time (no numpy width anywhere), on a case with a wrapping phase product, S > 0, both clamps, negative half-way sums and an
    absent channel"""
    rng = np.random.default_rng(100 * M + U)
    T = amd.wb_lo_table()
    S, N = 4, 90
    W = -(-N * M // U)
    first = (1 << 32) - W // 2
    assert first < (1 << 32) <= first + W - 1
    taps = rng.integers(-3, 4, L).astype(np.int16)
    taps[0], taps[L - 1] = 2, -1
    chans = [rng.integers(-6, 7, 2 * N).astype(np.int16), None, rng.integers(-6, 7, 2 * N).astype(np.int16)]
    inc = wbr_model_inc(M, U, [0.0, 111111.0, -234567.0])
    got = wbtxr_model(T, chans, M, U, inc, taps, S, first)
    assert got.size == 2 * W
    halfway_neg = clamp_hi = clamp_lo = plain = 0
    stuffed = []
    for x in chans:
        z = [(0, 0)] * (N * M)
        if x is not None:
            for m in range(N):
                z[m * M] = (int(x[2 * m]), int(x[2 * m + 1]))
        stuffed.append(z)
    for n in range(W):
        assert n * U < N * M
        w = [0, 0]
        for k, z in enumerate(stuffed):
            yr = sum(int(taps[t]) * z[n * U - t][0] for t in range(L) if n * U - t >= 0)
            yi = sum(int(taps[t]) * z[n * U - t][1] for t in range(L) if n * U - t >= 0)
            phi = ((first + n) * int(inc[k])) & 0xFFFFFFFF
            i = phi >> 20
            c, s = int(T[i]), int(T[(i - 1024) & 4095])
            w[0] += yr * c - yi * s
            w[1] += yi * c + yr * s
        for comp in (0, 1):
            v = (w[comp] + (1 << (S - 1))) // (1 << S)                      # python's // is floor
            halfway_neg += w[comp] < 0 and w[comp] % (1 << S) == 1 << (S - 1)
            clamp_hi, clamp_lo, plain = clamp_hi + (v > 32767), clamp_lo + (v < -32768), plain + (-32768 < v < 32767)
            assert got[2 * n + comp] == min(max(v, -32768), 32767), (n, comp)
    assert halfway_neg >= 2 and clamp_hi >= 3 and clamp_lo >= 3 and plain >= 30, (halfway_neg, clamp_hi, clamp_lo, plain)


@pytest.mark.parametrize("M,L,S,N", [(1, 1, 0, 500), (1, 64, 29, 700), (4, 143, 32, 600), (3, 2, 32, 700), (16, 1024, 31, 450)])
def test_up_1_is_the_integer_banks_model(amd, M, L, S, N):
    rng = np.random.default_rng(M * 1000 + L)
    T = amd.wb_lo_table()
    first = (1 << 32) - 1000
    centres = list(rng.uniform(-M * WIDE_RATE / 2, M * WIDE_RATE / 2, 3))
    inc = wbr_model_inc(M, 1, centres)
    assert np.array_equal(inc, wb_model_inc(M, centres))
    taps = rng.integers(-32768, 32768, L).astype(np.int64)
    for p in range(min(M, L)):
        while np.abs(taps[p::M]).sum() > 65535:
            taps[p::M] //= 2
    chans = [rng.integers(-32768, 32768, 2 * N).astype(np.int16), None, rng.integers(-32768, 32768, 2 * N).astype(np.int16)]
    if S == 0:                                                             # no shift: unit taps and inputs, or everything clamps
        taps = np.ones(L, np.int64)
        chans[0], chans[2] = rng.integers(-1, 2, 2 * N).astype(np.int16), None
    a = wbtxr_model(T, chans, M, 1, inc, taps.astype(np.int16), S, first)
    b = wbtx_model(T, chans, M, inc, taps.astype(np.int16), S, first)
    assert a.shape == b.shape == (2 * N * M,) and np.array_equal(a, b)
    assert (np.abs(a.astype(np.int32)) < 32767).mean() > 0.5 and np.unique(a).size > 100


# ------------------------------------------------------------------ opv_wbtxr_plan
def plan_rc(amd, down, up, K, L, S, centre, taps, reserved=0, inc=True, cfg=True):
    c = amd.WbtxrCfg(down, up, K, L, S, reserved, 0)
    centre = None if centre is None else np.ascontiguousarray(centre, np.float64)
    taps = None if taps is None else np.ascontiguousarray(taps, np.int16)
    out = np.zeros(300, np.uint32)
    return amd.lib().opv_wbtxr_plan(C.byref(c) if cfg else None, None if centre is None else centre.ctypes.data,
                                    None if taps is None else taps.ctypes.data, out.ctypes.data if inc else None)


@pytest.mark.parametrize("M,U", [(1, 1), (625, 542), (1250, 271), (7680, 271), (32, 1), (1025, 1024)])
def test_plan_increments_equal_the_rational_doors(amd, M, U):
    fw = M * WIDE_RATE / U
    centre = [100000.0, 1.0, 54200.0 * 7, -100000.0, -1.0, -fw / 4, 0.0, -0.0, 1e5 / 3, 12345.678901, np.pi * 1e4,
              fw / 2, -fw / 2, 0.75 * fw, -0.75 * fw, 3 * fw + 5000.0, -7 * fw - 5000.0, fw, 1e12]
    got = amd.wbtxr_plan(M, U, centre, [1, 2, 3], 0)
    assert got.dtype == np.uint32 and np.array_equal(got, wbr_model_inc(M, U, centre))
    assert np.array_equal(got, amd.wbr_plan(M, U, centre, [1, 2, 3], 0))   # the door's own plan: a channel sent up comes down again
    if U == 1 and M <= 16:
        assert np.array_equal(got, amd.wbtx_plan(M, centre, [1, 2, 3], 0))


def test_plan_increments_beyond_the_doors_up_limit(amd):
    """up may exceed the door's 1024 here: the rule is still the door's, held to the model"""
    centre = [100000.0, -1234567.0, 0.0]
    assert np.array_equal(amd.wbtxr_plan(8192, 8191, centre, [1, 2, 3], 0), wbr_model_inc(8192, 8191, centre))


def test_plan_refuses_what_lies_outside_the_limits(amd):
    ok = dict(down=7, up=4, K=2, L=9, S=5, centre=[1000.0, -1000.0], taps=[100, -200, 100, 7, 7, 7, 7, 7, 7], reserved=0)

    def rc(**kw):
        a = dict(ok, **kw)
        taps = a["taps"]
        if taps is not None and len(taps) != a["L"]:
            taps = np.ones(max(a["L"], 1), np.int16)
        return plan_rc(amd, a["down"], a["up"], a["K"], a["L"], a["S"], a["centre"], taps, a["reserved"], a.get("inc", True), a.get("cfg", True))
    assert rc() == 0
    # 1 <= up <= down <= 8192
    assert rc(up=0, down=1) == EINVAL and rc(up=-1, down=1) == EINVAL and rc(up=1, down=1) == 0
    assert rc(down=2, up=3) == EINVAL and rc(down=4, up=3) == 0 and rc(down=0, up=1) == EINVAL and rc(down=-5, up=1) == EINVAL
    assert rc(down=8192, up=8191) == 0 and rc(down=8193, up=8192) == EINVAL and rc(down=8193, up=8190) == EINVAL
    # down <= 32 up
    assert rc(down=33, up=1) == EINVAL and rc(down=32, up=1) == 0
    assert rc(down=65, up=2) == EINVAL and rc(down=63, up=2) == 0
    assert rc(down=8192, up=255) == EINVAL and rc(down=8191, up=256) == 0
    # lowest terms
    assert rc(down=6, up=4) == EINVAL and rc(down=3, up=3) == EINVAL and rc(down=542, up=271) == EINVAL
    # 1 <= n_taps, J <= 64
    assert rc(L=0) == EINVAL and rc(L=-1) == EINVAL and rc(L=1) == 0
    assert rc(down=1, up=1, L=64) == 0 and rc(down=1, up=1, L=65) == EINVAL
    assert rc(down=4, up=3, L=4 * 64) == 0 and rc(down=4, up=3, L=4 * 64 + 1) == EINVAL
    assert rc(down=8192, up=8191, L=524288) == 0 and rc(down=8192, up=8191, L=524289) == EINVAL
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
    assert b"opv_wbtxr" in amd.lib().opv_last_error()
    with pytest.raises(amd.OpvError):
        amd.wbtxr_plan(6, 4, [0.0], [1], 0)


def test_the_tap_cap_holds_per_phase(amd):
    """sum_j |taps[p + j M]| <= 65535 for EVERY phase p, and nothing is asked of the sum over all taps"""
    M, U = 65, 64
    full = np.repeat(np.array([32767, -32768], np.int16), M)               # two rows: every phase holds 32767 and -32768 = 65535 exactly

    def rc(taps):
        return plan_rc(amd, M, U, 1, len(taps), 40, [0.0], taps)
    assert full.size == 2 * M and all(np.abs(full[p::M].astype(np.int64)).sum() == 65535 for p in range(M))
    assert np.abs(full.astype(np.int64)).sum() == 65 * 65535 and rc(full) == 0
    for p in (0, 5, 64):
        extra = np.zeros(p + 1, np.int16)
        assert rc(np.concatenate([full, extra])) == 0                      # a ragged last row of zeros
        extra[p] = 1
        assert rc(np.concatenate([full, extra])) == EINVAL, p               # phase p alone at 65536
        extra[p] = -1
        assert rc(np.concatenate([full, extra])) == EINVAL, p
    low = np.repeat(np.array([32767, -32700], np.int16), M)                # every phase 68 short of the cap
    for p in (0, 63):
        extra = np.zeros(p + 1, np.int16)
        extra[p] = 68
        assert rc(np.concatenate([low, extra])) == 0
        extra[p] = -69
        assert rc(np.concatenate([low, extra])) == EINVAL
    # U = 1: the integer bank's rule
    assert plan_rc(amd, 4, 1, 1, 7, 0, [0.0], [1, 1, 32767, 1, 1, 1, -32768]) == 0
    assert plan_rc(amd, 4, 1, 1, 7, 0, [0.0], [1, 1, -32768, 1, 1, 1, -32768]) == EINVAL


# ------------------------------------------------------------------ opv_wbtxr_outputs
def test_outputs_is_ceil_n_m_over_u_at_the_edges(amd):
    for M, U in ((1, 1), (3, 2), (7, 4), (625, 542), (1250, 271), (7680, 271), (32, 1), (8192, 8191), (8191, 256)):
        assert gcd(M, U) == 1
        for N in (0, 1, 2, U - 1, U, U + 1, 2 * U - 1, 2 * U, 2 * U + 1, 86720, 50001, (1 << 31) - 1, 1 << 31, (1 << 32) + 1,
                  (1 << 40) + 7, MAX_INPUTS - 1, MAX_INPUTS):
            assert amd.wbtxr_outputs(M, U, N) == -(-N * M // U) == wbtxr_outputs(M, U, N), (M, U, N)
        assert amd.wbtxr_outputs(M, U, MAX_INPUTS + 1) == 0 and amd.wbtxr_outputs(M, U, (1 << 64) - 1) == 0
        prev = 0
        for N in range(1, 3 * U + 5 if U < 600 else 300):
            got = amd.wbtxr_outputs(M, U, N)
            assert got == -(-N * M // U) and got - prev >= 1, (M, U, N)     # every input brings at least one wide sample (down >= up)
            prev = got
    assert amd.wbtxr_outputs(1250, 271, 86720) * 271 == 86720 * 1250       # one frame at up = 271 is a whole number of wide samples
    L = amd.lib()
    assert L.opv_wbtxr_outputs(None, 5) == 0
    for bad in (amd.WbtxrCfg(0, 1, 1, 1, 0, 0, 0), amd.WbtxrCfg(2, 3, 1, 1, 0, 0, 0), amd.WbtxrCfg(6, 4, 1, 1, 0, 0, 0), amd.WbtxrCfg(33, 1, 1, 1, 0, 0, 0),
                amd.WbtxrCfg(7, 4, 1, 1, 0, 1, 0), amd.WbtxrCfg(7, 0, 1, 1, 0, 0, 0), amd.WbtxrCfg(8193, 8192, 1, 1, 0, 0, 0)):
        assert L.opv_wbtxr_outputs(C.byref(bad), 5) == 0
    assert L.opv_wbtxr_outputs(C.byref(amd.WbtxrCfg(7, 4, 1, 1, 0, 0, 0)), 5) == 9


def test_wbtxr_cfg_layout_matches_header(amd, tmp_path):
    """size and field offsets of the ctypes mirror against what gcc makes of include/opv_demod.h (as test_wbr_cfg_layout_matches_header)"""
    fs = ["down", "up", "n_channels", "n_taps", "out_shift", "reserved", "first_sample"]
    assert fs == [f[0] for f in amd.WbrCfg._fields_]
    offsets = check_ctypes_layout(tmp_path, amd.WbtxrCfg, "opv_wbtxr_cfg", 32, fs)
    assert C.sizeof(amd.WbtxrCfg) == C.sizeof(amd.WbrCfg) == 32
    for f in fs:
        assert offsets[f] == getattr(amd.WbtxrCfg, f).offset == getattr(amd.WbrCfg, f).offset, f
