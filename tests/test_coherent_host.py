"""CPU-only: what tests/test_gpu_coherent.py takes for granted about its inputs (tests/coherent_inputs.py), said by the oracle alone,
and the oracle held to the COMPILED REFERENCE's `-c` path on every one of them.

1. Every case meets the condition it was built for - the gain rule gives the whole capture in the tame regimes, both AFC clamps and
   both loop_freq clamps are visited, the silence branch produces exact +0.0, the default gains give a prefix of >= 1000 symbols.
   A recipe that stops meeting its condition fails HERE, before a device has seen it; the condition is never what gives way.
2. tests/test_oracle_pinned_live.py pins `-c` at (afc_alpha 0.002, pll_bw 35) on two captures. The GPU module compares the kernel
   with the oracle at six more settings; each is pinned here, every case, everything == (tests/hostile_inputs.py:
   assert_same_receive). afc_alpha = 0.5 is among them: the reference's command line reads -a with atof and passes any value on.
"""
import numpy as np
import pytest

import coherent_inputs as CI
from hostile_inputs import assert_same_receive, receive_pairs
from oracle_lib import Reference

WHOLE = ["tame_frozen", "tame_afc", "tame_afc_clamped", "loop_clamp", "silence", "edges", "offsets", "tie"]


def frames_of(name):
    return len(CI.case(name)["exp"]["frames"])


def test_case_list():
    assert len(CI.CASES) == len(set(CI.CASES)) == 4 + 4 + 4 + 18 + 1 + 2 + 8 + 4 + 1
    n = [CI.case(c)["nsym"] for c in CI.in_group("tame_frozen")]
    assert n == [21780] * 4, n


@pytest.mark.parametrize("name", [n for n in CI.CASES if CI.GROUP[n] in WHOLE])
def test_the_gain_rule_gives_the_whole_capture(name):
    c = CI.case(name)
    gmax = float(c["g"].max()) if c["nsym"] else 0.0
    print(f"{name}: {c['nsym']} symbols, largest gain {gmax:.3g}, E at the end {c['E'][-1] / max(c['M'], 1e-300):.2e} M")
    assert c["whole"] and c["P"] == c["nsym"] == c["n"] // 40, (c["P"], c["nsym"], gmax)
    assert len(c["E"]) == c["nsym"] + 1 and np.all(np.diff(c["E"]) >= 0)


def test_tame_frozen_releases_frames():
    per = {n: frames_of(n) for n in CI.in_group("tame_frozen")}
    assert all(CI.case(n)["setting"] == (0.0, 1.0) for n in per)
    assert max(per.values()) >= 3, per
    for n in per:                                                         # AFC frozen: fo never moves
        c = CI.case(n)
        assert np.all(c["extra"][:, 2] == c["est"]) and c["fin"][0] == c["est"], n


def test_tame_afc_releases_frames():
    per = {n: frames_of(n) for n in CI.in_group("tame_afc")}
    assert all(CI.case(n)["setting"] == (0.001, 1.0) for n in per)
    assert sum(v >= 2 for v in per.values()) >= 2, per


@pytest.mark.parametrize("name", ["clamped-n300", "clamped-p1900"])
def test_tame_afc_clamped_visits_both_clamps(name):
    c = CI.case(name)
    fo = c["extra"][:, 2]
    hi, lo = int(np.sum(fo == CI.FO_CLAMP)), int(np.sum(fo == -CI.FO_CLAMP))
    print(f"{name}: fo == +2000 behind {hi} symbols, == -2000 behind {lo}")
    assert c["setting"] == (0.05, 1.0) and hi >= 100 and lo >= 100 and np.all(np.abs(fo) <= CI.FO_CLAMP)


def test_tame_afc_clamped_truncations_end_on_the_clamps():
    hi, lo, full = CI.case("clamped-cut-hi"), CI.case("clamped-cut-lo"), CI.case("clamped-p1900")
    assert hi["fin"][0] == CI.FO_CLAMP and lo["fin"][0] == -CI.FO_CLAMP
    assert hi["nsym"] != lo["nsym"]
    for c in (hi, lo):
        K = c["nsym"]
        assert c["n"] == 40 * K and c["est"] == full["est"]
        assert c["soft"].tobytes() == full["soft"][:K].tobytes() and c["fin"][0] == full["extra"][K - 1, 2]


@pytest.mark.parametrize("name", CI.in_group("default_prefix"))
def test_default_prefix_is_long_enough(name):
    c = CI.case(name)
    print(f"{name}: P = {c['P']} of {c['nsym']} symbols, gain at the end {c['g'][-1]:.3g}")
    assert c["setting"] in CI.DEFAULT and c["P"] >= 1000


def test_loop_clamp_is_visible():
    c = CI.case("loop-clamp")
    K, lf = c["nsym"], c["extra"][:, 1]
    print(f"loop-clamp: K = {K}, loop_freq behind each symbol {lf.tolist()}")
    assert c["setting"] == (0.0, 5000.0) and 8 <= K <= 12 and c["n"] == 40 * K + 17 and c["P"] == K
    assert np.any(lf == CI.LOOP_FREQ_CLAMP) and np.any(lf == -CI.LOOP_FREQ_CLAMP) and np.all(np.abs(lf) <= CI.LOOP_FREQ_CLAMP)
    assert abs(c["fin"][1]) == CI.LOOP_FREQ_CLAMP            # what the chunk line shows


def exact_plus_zero(v):
    return np.all(v == 0.0) and not np.any(np.signbit(v))


def test_silence_gives_exact_plus_zero():
    z = CI.case("silence-zeros")
    assert z["n"] == 300 * 40 + 22 and z["nsym"] == 300 and exact_plus_zero(z["soft"])
    assert z["fin"] == (z["est"], 0.0, 0.0) and len(z["exp"]["frames"]) == 0 and len(z["exp"]["events"]) == 0
    g = CI.case("silence-gaps")
    soft = g["soft"]
    a, b = CI.GAP_WHOLE
    assert exact_plus_zero(soft[a:b]) and soft[a - 1] != 0.0 and soft[b] != 0.0
    r0, r1 = CI.GAP_RAGGED
    assert r0 % 40 == 13 and r1 % 40 == 7
    assert soft[r0 // 40] != 0.0 and exact_plus_zero(soft[r0 // 40 + 1: r1 // 40]) and soft[r1 // 40] != 0.0     # 13 / 33 live samples
    zeros = np.nonzero(soft == 0.0)[0]
    assert zeros.size >= 100 and exact_plus_zero(soft[zeros])
    # what the branch does to the loop: phase error 0 and atan2(0, 0) = 0, so loop_freq and fo stand still through the gap
    assert np.all(g["extra"][a:b, 1] == g["extra"][a - 1, 1]) and np.all(g["extra"][a:b, 2] == g["extra"][a - 1, 2])
    # the first live symbol moves the loop again; the AFC one symbol later (its previous correlation is still the gap's zero)
    assert g["extra"][b, 1] != g["extra"][a - 1, 1] and g["extra"][b, 2] == g["extra"][a - 1, 2] and g["extra"][b + 1, 2] != g["extra"][b, 2]


def test_edges_symbol_counts():
    n = [(CI.case(c)["n"], CI.case(c)["nsym"]) for c in CI.in_group("edges")]
    assert n == [(0, 0), (39, 0), (40, 1), (41, 1), (79, 1), (80, 2), (86719, 2167), (86720, 2168)], n


def test_offset_estimates_differ_in_sign_and_size():
    est = [CI.case(c)["est"] for c in CI.OFFSETS]
    print(f"offset estimates of one context's four streams: {est}")
    assert len(set(est)) == 4 and min(est) < -1000 and max(est) > 500 and any(-500 < e < 0 for e in est), est


def test_equal_tone_energies_at_symbol_0():
    """tie-dc: the dominant tone is chosen by `en1 > en2`, so at exact equality the upper tone's correlation drives the loop. Symbol 0
    of a real constant at an estimate of exactly 0 Hz is such an equality with energy in it: restated here in the oracle's order of
    operations with the same libm, then seen in the oracle's trace - the phase error has the sign of Im c2."""
    import math
    c = CI.case("tie-dc")
    assert c["est"] == 0.0 and c["nsym"] == 200 and np.all(c["x"][1::2] == 0) and np.all(c["x"][0::2] == 12345)
    inc1, inc2 = 2.0 * math.pi * (-13550.0 + 0.0) / 2168000.0, 2.0 * math.pi * (13550.0 + 0.0) / 2168000.0
    p1 = p2 = c1r = c1i = c2r = c2i = 0.0
    for _ in range(40):
        xr, xi = 12345.0, 0.0                                              # the carrier phase is 0 throughout symbol 0
        k1, s1, k2, s2 = math.cos(p1), math.sin(p1), math.cos(p2), math.sin(p2)
        c1r += xr * k1 - xi * (-s1); c1i += xr * (-s1) + xi * k1
        c2r += xr * k2 - xi * (-s2); c2i += xr * (-s2) + xi * k2
        p1 += inc1; p2 += inc2
    en1, en2 = c1r * c1r + c1i * c1i, c2r * c2r + c2i * c2i
    assert en1 == en2 and en1 > 1e10 and c2i == -c1i and c2i < 0.0, (c1r, c1i, c2r, c2i)
    assert c["soft"][0] == c2r - c1r == 0.0
    pll_alpha = 2.0 * 0.707 * (1.0 * 2.0 * math.pi) / 54200.0
    carrier0 = c["extra"][0, 0]
    assert carrier0 == pll_alpha * (c2i / math.hypot(c2r, c2i)) and carrier0 < 0.0, carrier0        # c1 would have given > 0
    assert np.all(c["soft"][1:] != 0.0)


# ------------------------------------------------------------------ 2. the oracle == the compiled reference, every case
@pytest.fixture(scope="module")
def pairs():
    jobs = [(CI.case(n)["x"], dict(streaming=False, coherent=True, afc_alpha=CI.case(n)["setting"][0], pll_bw=CI.case(n)["setting"][1]))
            for n in CI.CASES]
    return dict(zip(CI.CASES, receive_pairs(jobs)))


@pytest.mark.skipif(not Reference.available(), reason="oracle/_ref/libopv_ref.so not built")
@pytest.mark.parametrize("name", CI.CASES)
def test_oracle_equals_the_reference(pairs, name):
    a, b = pairs[name]
    c = CI.case(name)
    assert a["soft"].tobytes() == c["soft"].tobytes()                     # (the pair's oracle run is the case's)
    assert_same_receive(a, b, f"-c {name} afc_alpha {c['setting'][0]} pll_bw {c['setting'][1]}")
