"""CPU-only: the host half of the wideband transmit bank (include/opv_demod.h, opv_wbtx_*) - plan, limits, struct layout - against
a numpy int64 restatement of the header's arithmetic. The model is tests/wideband_models.py (wbtx_model), and
tests/test_gpu_wideband_tx.py holds the device to it with ==. The increment rule and the LO table are the receive bank's
(wideband_models.wb_model_inc, opv_wb_lo_table): one definition serves both directions."""
import ctypes as C

import numpy as np
import pytest

from fixtures_built import amd  # noqa: F401
from struct_layout import check_ctypes_layout
from wideband_models import WIDE_RATE, wb_model_inc, wbtx_model

EINVAL = -1


def test_model_agrees_with_a_sample_by_sample_restatement(amd):
    """the vectorised model (wideband_models.wbtx_model) against the header's formulas written out one sample and one tap at a time in python integers
    (no numpy width anywhere), on a case with a wrapping phase product, S > 0, both clamps, negative half-way sums, L % U != 0 and
    an absent channel"""
    rng = np.random.default_rng(11)
    T = amd.wb_lo_table()
    U, L, S, first, N = 3, 7, 4, (1 << 32) - 50, 36
    assert L % U
    taps = np.array([1, -2, 3, 2, -1, 1, 2], np.int16)
    chans = [rng.integers(-6, 7, 2 * N).astype(np.int16), None, rng.integers(-6, 7, 2 * N).astype(np.int16)]
    inc = wb_model_inc(U, [0.0, 111111.0, -1234567.0])
    got = wbtx_model(T, chans, U, inc, taps, S, first)
    assert first < (1 << 32) <= first + N * U
    halfway_neg = clamp_hi = clamp_lo = plain = 0
    for n in range(N * U):
        q, p = divmod(n, U)
        w = [0, 0]
        for k, x in enumerate(chans):
            if x is None:
                continue
            yr = sum(int(taps[p + j * U]) * int(x[2 * (q - j)]) for j in range(L) if p + j * U < L and q - j >= 0)
            yi = sum(int(taps[p + j * U]) * int(x[2 * (q - j) + 1]) for j in range(L) if p + j * U < L and q - j >= 0)
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
    assert halfway_neg >= 3 and clamp_hi >= 3 and clamp_lo >= 3 and plain >= 30, (halfway_neg, clamp_hi, clamp_lo, plain)


# ------------------------------------------------------------------ opv_wbtx_plan
def plan_rc(amd, interp, K, L, S, centre, taps, inc=True, cfg=True):
    c = amd.WbtxCfg(interp, K, L, S, 0)
    centre = None if centre is None else np.ascontiguousarray(centre, np.float64)
    taps = None if taps is None else np.ascontiguousarray(taps, np.int16)
    out = np.zeros(300, np.uint32)
    return amd.lib().opv_wbtx_plan(C.byref(c) if cfg else None, None if centre is None else centre.ctypes.data,
                                   None if taps is None else taps.ctypes.data, out.ctypes.data if inc else None)


@pytest.mark.parametrize("interp", [1, 3, 4, 16])
def test_plan_increments_equal_the_ddc_banks(amd, interp):
    fs = interp * WIDE_RATE
    centre = [100000.0, 1.0, -100000.0, -fs / 4, 0.0, -0.0, 1e5 / 3, 12345.678901, np.pi * 1e4, fs / 2, -fs / 2, 0.75 * fs,
              3 * fs + 5000.0, -7 * fs - 5000.0, fs, 1e12]
    got = amd.wbtx_plan(interp, centre, [1, 2, 3], 0)
    assert got.dtype == np.uint32 and np.array_equal(got, wb_model_inc(interp, centre))
    assert np.array_equal(got, amd.wb_plan(interp, centre, [1, 2, 3], 0))   # the DDC bank's own plan: a channel sent up comes down again


def test_plan_refuses_what_lies_outside_the_limits(amd):
    ok = dict(interp=4, K=2, L=3, S=5, centre=[1000.0, -1000.0], taps=[100, -200, 100])

    def rc(**kw):
        a = dict(ok, **kw)
        return plan_rc(amd, a["interp"], a["K"], a["L"], a["S"], a["centre"], a["taps"], a.get("inc", True), a.get("cfg", True))
    assert rc() == 0
    for interp in (0, -1, 17, 1 << 20):
        assert rc(interp=interp) == EINVAL, interp
    for K in (0, -3, 257):
        assert rc(K=K, centre=np.zeros(300)) == EINVAL, K
    for L in (0, -1, 1025):
        assert rc(L=L, taps=np.ones(1100, np.int16)) == EINVAL, L
    for S in (-1, 41, 64):
        assert rc(S=S) == EINVAL, S
    assert rc(interp=1) == 0 and rc(interp=16) == 0 and rc(S=0) == 0 and rc(S=40) == 0
    assert rc(K=256, centre=np.zeros(256)) == 0 and rc(L=1, taps=[-32768]) == 0 and rc(L=1024, taps=np.ones(1024, np.int16)) == 0
    # per phase sum |h| <= 65535 exactly. U = 1 (one phase: all the taps)
    assert rc(interp=1, L=3, taps=[32767, 32767, 1]) == 0 and rc(interp=1, L=3, taps=[32767, 32767, 2]) == EINVAL
    assert rc(interp=1, L=2, taps=[-32768, -32767]) == 0 and rc(interp=1, L=2, taps=[-32768, -32768]) == EINVAL
    assert rc(interp=1, L=1024, taps=np.full(1024, -63, np.int16)) == 0 and rc(interp=1, L=1024, taps=np.full(1024, 64, np.int16)) == EINVAL
    # a phase other than 0: U = 4, L = 7, phase 2 holds taps 2 and 6; the other phases stay small
    assert rc(interp=4, L=7, taps=[1, 1, 32767, 1, 1, 1, -32768]) == 0
    assert rc(interp=4, L=7, taps=[1, 1, -32768, 1, 1, 1, -32768]) == EINVAL
    assert rc(interp=4, L=7, taps=[1, 1, 1, 32767, 1, 1, 1]) == 0          # phase 3 has one tap only (L % U != 0)
    # the limit is per phase, not over all taps: four full phases pass
    assert rc(interp=4, L=8, taps=[32767, -32768, 32767, -32768, -32768, 32767, -32768, 32767]) == 0
    assert rc(interp=4, L=9, taps=[32767, -32768, 32767, -32768, -32768, 32767, -32768, 32767, 1]) == EINVAL   # phase 0 again
    for bad in (np.nan, np.inf, -np.inf):
        assert rc(centre=[1000.0, bad]) == EINVAL, bad
    assert rc(centre=None) == EINVAL and rc(taps=None) == EINVAL and rc(inc=False) == EINVAL and rc(cfg=False) == EINVAL
    assert b"opv_wbtx" in amd.lib().opv_last_error()
    with pytest.raises(amd.OpvError):
        amd.wbtx_plan(17, [0.0], [1], 0)


def test_wbtx_cfg_layout_matches_header(amd, tmp_path):
    """size and field offsets of the ctypes mirror against what gcc makes of include/opv_demod.h (as test_wb_cfg_layout_matches_header)"""
    fs = ["interp", "n_channels", "n_taps", "out_shift", "first_sample"]
    offsets = check_ctypes_layout(tmp_path, amd.WbtxCfg, "opv_wbtx_cfg", 24, fs)
    assert C.sizeof(amd.WbtxCfg) == C.sizeof(amd.WbCfg) == 24
    for f, g in zip(fs, [f[0] for f in amd.WbCfg._fields_]):
        assert offsets[f] == getattr(amd.WbtxCfg, f).offset == getattr(amd.WbCfg, g).offset, f
