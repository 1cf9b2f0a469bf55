"""CPU-only: csrc/opv_tf_rule.h - opv_tf_clamp_cannot_act(tf, n), the per-call proof that lets k_msk_frontend_rb run a
demodulate() call without the timing loop's clamp - compiled with g++ (tests/tf_rule_probe.cpp gives it a C face) and called
through ctypes. The rule as the header states it: true iff |tf| + 2 * beta * (n / 39 + 2) < 0.1 and tf is not a NaN, beta = 1e-5
(reference src/opv-demod.cpp:118, :283-284). What is checked is what the kernel relies on: wherever the rule says "cannot act", a
walk of n / 39 + 2 symbols that each push tf outward by the most the rule allows (2 * beta) stays strictly inside +/-0.1, so
fmin(fmax(tf, -0.1), 0.1) would have returned tf itself on every one of them."""
import ctypes
import math
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "opv-cxx-demod_amd" / "csrc"
BETA, TFMAX, CHUNK = 0.00001, 0.1, 86720


@pytest.fixture(scope="module")
def rule(tmp_path_factory):
    so = tmp_path_factory.mktemp("tf_rule") / "libtfrule.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-ffp-contract=off", "-shared", "-I", str(CSRC), "-o", str(so),
                    str(ROOT / "tests" / "tf_rule_probe.cpp")], check=True)
    L = ctypes.CDLL(str(so))
    L.probe_tf_clamp_cannot_act.argtypes = [ctypes.c_double, ctypes.c_uint64]
    L.probe_tf_beta.restype = L.probe_tf_max.restype = ctypes.c_double
    L.probe_tf_worst_walk.restype = ctypes.c_double
    L.probe_tf_worst_walk.argtypes = [ctypes.c_double, ctypes.c_uint64, ctypes.c_double]
    return L


def threshold(n):
    """the rule's own left-hand side without |tf|, in the header's order of operations"""
    return 2.0 * BETA * float(n // 39 + 2)


def test_constants_are_the_references(rule):
    assert rule.probe_tf_beta() == BETA and rule.probe_tf_max() == TFMAX


def test_free_calls_stay_strictly_inside_the_clamp(rule):
    """random (tf, n): wherever the rule holds, the worst walk it covers never reaches +/-0.1, in either direction; and the rule is
    the stated inequality on every draw"""
    rng = np.random.default_rng(20261021)
    tfs = np.concatenate([rng.uniform(-0.11, 0.11, 700), rng.uniform(-0.06, -0.05, 150), rng.uniform(0.05, 0.06, 150)])
    ns = np.concatenate([rng.integers(1, 200_000, 600), np.full(300, CHUNK), rng.integers(CHUNK - 4000, CHUNK + 1, 100)])
    free = 0
    for tf, n in zip(tfs.tolist(), ns.tolist()):
        got = bool(rule.probe_tf_clamp_cannot_act(tf, n))
        assert got == (abs(tf) + threshold(n) < TFMAX), (tf, n)
        if got:
            free += 1
            for ted in (2.0, -2.0):
                assert rule.probe_tf_worst_walk(tf, n, ted) < TFMAX, (tf, n, ted)
    assert 200 < free < 800                               # both sides of the rule were drawn


def test_the_edges_fall_on_the_guarded_side(rule):
    for n in (1, 39, 2168 * 40, CHUNK, 150_000):
        assert not rule.probe_tf_clamp_cannot_act(math.nan, n)
        assert not rule.probe_tf_clamp_cannot_act(-math.nan, n)
        for tf in (0.1, -0.1, math.nextafter(0.1, 0.0), math.nextafter(-0.1, 0.0), math.inf, -math.inf):
            assert not rule.probe_tf_clamp_cannot_act(tf, n), (tf, n)
        for tf in (0.0999, -0.0999):                      # (a call of a few symbols cannot carry even this to the clamp)
            assert bool(rule.probe_tf_clamp_cannot_act(tf, n)) == (n < 39 * 3), (tf, n)
        # the threshold itself: the largest tf the rule lets through, found by bisection on the rule, and its neighbours
        lo, hi = 0.0, 0.1
        assert rule.probe_tf_clamp_cannot_act(lo, n) and not rule.probe_tf_clamp_cannot_act(hi, n)
        while math.nextafter(lo, 1.0) < hi:
            mid = 0.5 * (lo + hi)
            if rule.probe_tf_clamp_cannot_act(mid, n):
                lo = mid
            else:
                hi = mid
        assert abs(lo - (TFMAX - threshold(n))) < 1e-15
        for s in (1.0, -1.0):
            assert rule.probe_tf_clamp_cannot_act(s * lo, n) and not rule.probe_tf_clamp_cannot_act(s * hi, n)
            # One ulp below the threshold the call is free. The rule's own worst case (|ted| = 2 on every symbol) then ends within
            # rounding of 0.1 itself; what the kernel can produce - |ted| <= 1 up to the rounding of a quotient - stays strictly
            # inside by half the rule's allowance, far more than n / 39 + 2 roundings of tf.
            assert rule.probe_tf_worst_walk(s * lo, n, s * (1.0 + 1e-9)) < TFMAX
            assert rule.probe_tf_worst_walk(s * lo, n, s * 2.0) <= TFMAX + (n // 39 + 2) * 2.0**-57
    # a -s call: the threshold is near 0.055
    assert rule.probe_tf_clamp_cannot_act(0.055, CHUNK) and not rule.probe_tf_clamp_cannot_act(0.056, CHUNK)


def test_large_calls_do_not_overflow(rule):
    """n up to 2^31 and beyond: the symbol bound is formed in 64 bits, a batch-mode call over a huge capture keeps the clamp"""
    for n in (195_000, 2**31 - 1, 2**31, 2**32 - 1, 2**32, 2**40, 2**63, 2**64 - 1):
        assert not rule.probe_tf_clamp_cannot_act(0.0, n), n
    # the largest call a zero tf passes: 2e-5 * (n / 39 + 2) < 0.1  <=>  n / 39 + 2 <= 4999
    assert rule.probe_tf_clamp_cannot_act(0.0, 39 * 4997 + 38) and not rule.probe_tf_clamp_cannot_act(0.0, 39 * 4998)
