"""CPU-only: the host half of the wideband front door (include/opv_demod.h, opv_wb_*) - plan, LO table, output count, struct
layout - against a numpy int64 restatement of the header's arithmetic. The model is tests/wideband_models.py (wb_model_inc,
wb_model), and tests/test_gpu_wideband.py holds the device to the same functions with ==."""
import ctypes as C

import numpy as np
import pytest

from fixtures_built import amd  # noqa: F401
from struct_layout import check_ctypes_layout
from wideband_models import WIDE_RATE, wb_model, wb_model_inc

EINVAL = -1


# ------------------------------------------------------------------ opv_wb_plan
def plan_rc(amd, decim, K, L, S, centre, taps, inc=True, cfg=True):
    c = amd.WbCfg(decim, K, L, S, 0)
    centre = None if centre is None else np.ascontiguousarray(centre, np.float64)
    taps = None if taps is None else np.ascontiguousarray(taps, np.int16)
    out = np.zeros(300, np.uint32)
    return amd.lib().opv_wb_plan(C.byref(c) if cfg else None, None if centre is None else centre.ctypes.data,
                                 None if taps is None else taps.ctypes.data, out.ctypes.data if inc else None)


@pytest.mark.parametrize("decim", [1, 3, 4, 16])
def test_plan_increments_equal_the_model(amd, decim):
    fs = decim * WIDE_RATE
    centre = [100000.0, 1.0, 54200.0 * 7, -100000.0, -1.0, -fs / 4, 0.0, -0.0,
              1e5 / 3, 12345.678901, np.pi * 1e4,                          # not representable in 32 bits of a turn
              fs / 2, -fs / 2, 0.75 * fs, -0.75 * fs, 3 * fs + 5000.0, -7 * fs - 5000.0, fs, 1e12]        # beyond +/-Fs/2: wraps
    got = amd.wb_plan(decim, centre, [1, 2, 3], 0)
    exp = wb_model_inc(decim, centre)
    assert got.dtype == np.uint32 and np.array_equal(got, exp), (got, exp)
    k = {f: j for j, f in enumerate(centre)}
    assert got[k[0.0]] == 0 and got[k[fs]] == 0 and got[k[fs / 2]] == 1 << 31 and got[k[-fs / 2]] == 1 << 31
    assert got[k[-fs / 4]] == 3 << 30 and got[k[0.75 * fs]] == 3 << 30 and got[k[-0.75 * fs]] == 1 << 30
    assert int(got[k[100000.0]]) + int(got[k[-100000.0]]) == 1 << 32         # a negative centre wraps
    assert got[k[3 * fs + 5000.0]] == wb_model_inc(decim, [5000.0])[0] and got[k[1e5 / 3]] not in (0, 1 << 31)


def test_plan_refuses_what_lies_outside_the_limits(amd):
    ok = dict(decim=4, K=2, L=3, S=5, centre=[1000.0, -1000.0], taps=[100, -200, 100])

    def rc(**kw):
        a = dict(ok, **kw)
        return plan_rc(amd, a["decim"], a["K"], a["L"], a["S"], a["centre"], a["taps"], a.get("inc", True), a.get("cfg", True))
    assert rc() == 0
    for decim in (0, -1, 17, 1 << 20):
        assert rc(decim=decim) == EINVAL, decim
    for K in (0, -3, 257):
        assert rc(K=K, centre=np.zeros(300)) == EINVAL, K
    for L in (0, -1, 1025):
        assert rc(L=L, taps=np.ones(1100, np.int16)) == EINVAL, L
    for S in (-1, 41, 64):
        assert rc(S=S) == EINVAL, S
    assert rc(decim=1) == 0 and rc(decim=16) == 0 and rc(S=0) == 0 and rc(S=40) == 0
    assert rc(K=256, centre=np.zeros(256)) == 0 and rc(L=1, taps=[-32768]) == 0
    # sum |h| <= 2^21 exactly: 64 taps of -32768 is 2^21; one LSB more is refused
    assert rc(L=64, taps=np.full(64, -32768, np.int16)) == 0
    assert rc(L=65, taps=np.concatenate([np.full(64, -32768, np.int16), [1]])) == EINVAL
    assert rc(L=65, taps=np.concatenate([np.full(64, 32767, np.int16), [64]])) == 0
    assert rc(L=65, taps=np.concatenate([np.full(64, 32767, np.int16), [65]])) == EINVAL
    assert rc(L=1024, taps=np.full(1024, 2048, np.int16)) == 0 and rc(L=1024, taps=np.full(1024, -2049, np.int16)) == EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        assert rc(centre=[1000.0, bad]) == EINVAL, bad
    assert rc(centre=None) == EINVAL and rc(taps=None) == EINVAL and rc(inc=False) == EINVAL and rc(cfg=False) == EINVAL
    assert b"opv_wb" in amd.lib().opv_last_error()
    with pytest.raises(amd.OpvError):
        amd.wb_plan(17, [0.0], [1], 0)


def test_outputs_is_ceil_n_over_d_at_the_edges(amd):
    for D in (1, 2, 3, 4, 15, 16):
        for N in (0, 1, D - 1, D, D + 1, 2 * D - 1, 2 * D, 86720, 86721, (1 << 31) - 1, 1 << 31, (1 << 32) + 1, (1 << 40) + 7, (1 << 63) + 5, (1 << 64) - 1):
            assert amd.wb_outputs(D, N) == -(-N // D), (D, N)
    assert amd.lib().opv_wb_outputs(None, 5) == 0
    assert amd.lib().opv_wb_outputs(C.byref(amd.WbCfg(0, 1, 1, 0, 0)), 5) == 0


def test_lo_table_is_numpys_and_far_from_every_rounding_boundary(amd):
    T = amd.wb_lo_table()
    x = 32767.0 * np.cos(2.0 * np.pi * np.arange(4096) / 4096.0)
    assert T.dtype == np.int16 and np.array_equal(T, np.rint(x).astype(np.int16))
    # no libm can round an entry the other way: cos is good to ~1e-16 relative, i.e. ~4e-12 here; no entry is within 1e-6 of a half
    assert np.min(np.abs(np.abs(x - np.floor(x)) - 0.5)) > 1e-6
    assert T[0] == 32767 and T[1024] == 0 and T[2048] == -32767 and T[3072] == 0 and np.array_equal(T[1:], T[:0:-1])
    i = np.arange(4096)
    assert np.max(np.abs(T.astype(np.int64) ** 2 + T[(i - 1024) & 4095].astype(np.int64) ** 2 - 32767 ** 2)) < 2 * 32767        # (c, s) stay on the circle: |mr|, |mi| < 2^31


def test_wb_cfg_layout_matches_header(amd, tmp_path):
    """size and field offsets of the ctypes mirror against what gcc makes of include/opv_demod.h (as test_struct_layouts_match_header)"""
    check_ctypes_layout(tmp_path, amd.WbCfg, "opv_wb_cfg", 24, ["decim", "n_channels", "n_taps", "out_shift", "first_sample"])


def test_model_agrees_with_a_sample_by_sample_restatement(amd):
    """the vectorised model (wideband_models.wb_model) against the header's formulas written out one sample and one tap at a time in python integers
    (no numpy width anywhere), on a case with a wrapping phase product, S > 0, both clamps and negative half-way accumulators"""
    rng = np.random.default_rng(5)
    T = amd.wb_lo_table()
    D, L, first, N = 3, 7, (1 << 32) - 5, 41
    wide = rng.integers(-32768, 32768, 2 * N).astype(np.int16)
    taps = np.array([3000, -7000, 12000, 32767, 12000, -7000, 3000], np.int16)
    inc = wb_model_inc(D, [250000.0, -1234567.0])
    # S = 4: every output of this full-range case clamps. S = 33: none can (|acc| <= sum |taps| x 2^15 x 32767 x sqrt 2 < 2^46.8, and
    # 2^13.8 < 32767), so the rounding term and the floor show in every value
    for S in (4, 33):
        got = wb_model(T, wide, D, inc, taps, S, first)
        for k, w in enumerate(inc):
            m = []
            for n in range(N):
                phi = ((first + n) * int(w)) & 0xFFFFFFFF
                i = phi >> 20
                c, s = int(T[i]), int(T[(i - 1024) & 4095])
                x, y = int(wide[2 * n]), int(wide[2 * n + 1])
                m.append((x * c + y * s, y * c - x * s))
            for r in range(-(-N // D)):
                for comp in (0, 1):
                    acc = sum(int(taps[t]) * m[r * D - t][comp] for t in range(L) if r * D - t >= 0)
                    v = (acc + (1 << (S - 1))) // (1 << S)                  # python's // is floor
                    assert got[k, 2 * r + comp] == min(max(v, -32768), 32767), (S, k, r, comp)
        if S == 4:
            assert (got == 32767).any() and (got == -32768).any()
        else:
            assert (np.abs(got.astype(np.int32)) < 32767).all() and (got < 0).any() and (got > 0).any()
