"""CPU-only: the link report's interface (header, EXPORTS, the numpy mirror of opv_link against gcc's layout), link_esn0_db, and
the CPU model tests/link_model.py pinned to the oracle on inputs whose answers are known without any model: clean frames,
flipped symbols, zeroed symbols, and the noise level the GPU tests rely on for being non-vacuous."""
import ctypes as C
import math
import re
import subprocess

import numpy as np
import pytest

import soft_log_inputs as S
from amd_lib import ROOT
from fixtures_built import amd  # noqa: F401
from link_model import BOUND, CODED, link_model

NAMES = ["opv_enable_link_report", "opv_pop_frames_link", "opv_device_link", "opv_link_payloads"]


def test_header_declares_the_link_report_and_exports_carry_it(amd):
    text = (ROOT / "include" / "opv_demod.h").read_text()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
        assert n in amd.EXPORTS, n
        assert hasattr(amd.lib(), n), n
    assert re.search(r"#define OPV_ABI_VERSION 7\b", text)
    assert "typedef struct opv_link" in code
    assert "DO NOT MIGRATE" in text                         # the import rule is stated where a caller reads it


def test_link_dtype_matches_the_header(amd, tmp_path):
    """LINK_DTYPE against gcc's sizeof / offsetof of opv_link: 40 bytes"""
    fs = list(amd.LINK_DTYPE.names)
    assert fs == ["valid", "bit_errors", "weak", "nonfinite", "m1", "m2", "ma"]
    src = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{ROOT / "include" / "opv_demod.h"}"', "int main(void){",
           'printf("opv_link %zu\\n", sizeof(opv_link));']
    src += [f'printf("{f} %zu\\n", offsetof(opv_link, {f}));' for f in fs]
    src.append("return 0;}")
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-o", str(tmp_path / "l"), str(tmp_path / "l.c")], check=True)
    got = dict(ln.split() for ln in subprocess.run([str(tmp_path / "l")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["opv_link"]) == amd.LINK_DTYPE.itemsize == 40
    for f in fs:
        assert int(got[f]) == amd.LINK_DTYPE.fields[f][1], f
    assert [amd.LINK_DTYPE.fields[f][0].str for f in fs] == ["<i4"] * 4 + ["<f8"] * 3


def test_link_esn0_db(amd):
    rec = np.zeros(5, amd.LINK_DTYPE)
    rec["valid"] = [1, 1, 0, 1, 1]
    rec["nonfinite"] = [0, 0, 0, 2, 0]
    rec["ma"] = [500.0, 500.0, 500.0, 500.0, 3.0]
    rec["m2"] = [500.0 ** 2 + 250.0 ** 2, 500.0 ** 2, 500.0 ** 2 + 1.0, 500.0 ** 2 + 1.0, 8.0]
    db = amd.link_esn0_db(rec)
    assert db[0] == pytest.approx(10 * math.log10(500.0 ** 2 / (2 * 250.0 ** 2)), abs=1e-12)      # A^2 / 2 sigma^2: 3.01 dB
    assert db[1] == math.inf and math.isnan(db[2]) and math.isnan(db[3])
    assert db[4] == math.inf                                 # m2 < ma^2 (rounding can do that to a clean frame): +inf, not nan
    assert float(amd.link_esn0_db(rec[0])) == db[0]          # one record as well as an array
    assert "NOT a" in amd.link_esn0_db.__doc__ and "calibrated" in amd.link_esn0_db.__doc__


def noisy(oracle, sigma, seed, n=8):
    rng = np.random.default_rng(seed)
    return [S.payload(oracle, k, sigma=sigma, rng=rng) for k in range(n)]


def test_model_on_clean_flipped_and_zeroed_symbols(oracle):
    tx = oracle.bert_frames(8)
    rng = np.random.default_rng(11)
    for k in range(8):
        clean = S.payload(oracle, k)
        r = link_model(oracle, clean)
        assert (r["valid"], r["bit_errors"], r["weak"], r["nonfinite"]) == (1, 0, 0, 0)
        assert np.array_equal(r["frame"], tx[k]) and r["m1"] == S.A and r["m2"] == S.A ** 2 and r["ma"] == S.A
        at = rng.choice(CODED, 7, replace=False)
        p = clean.copy()
        p[at] = -p[at]
        r = link_model(oracle, p)
        assert r["bit_errors"] == 7 and r["weak"] == 0 and np.array_equal(r["frame"], tx[k])
        assert r["ma"] == S.A * (CODED - 14) / CODED and r["m2"] == S.A ** 2
        p = clean.copy()
        p[at] = 0.0                                          # q = 4: a hard 1, wrong wherever a 0 was sent
        r = link_model(oracle, p)
        enc = oracle.encode_frame(tx[k])
        assert r["weak"] == 7 and r["bit_errors"] == int((enc[at] == 0).sum()) and np.array_equal(r["frame"], tx[k])
    r = link_model(oracle, np.zeros(CODED))
    assert r["valid"] == 0 and r["metric"] == -1 and r["bit_errors"] == r["weak"] == 0 and r["m1"] == r["m2"] == r["ma"] == 0.0


def test_model_at_sigma_250_decodes_and_counts_tens_of_errors(oracle):
    """the non-vacuity condition of the noisy GPU cases: A = 500, sigma = 250 - every frame still decodes to what was sent and the
    decoder corrected 20 .. 80 channel bits of each (expectation 2144 Q(2) = 49)"""
    tx = oracle.bert_frames(8)
    for k, p in enumerate(noisy(oracle, 250.0, seed=250)):
        r = link_model(oracle, p)
        print("sigma 250 frame", k, "bit_errors", r["bit_errors"], "weak", r["weak"])
        assert np.array_equal(r["frame"], tx[k]), k
        assert 20 <= r["bit_errors"] <= 80, (k, r["bit_errors"])
        assert r["valid"] == 1 and r["nonfinite"] == 0
        # the estimator reads about A^2 / 2 sigma^2 = 3.01 dB. Its spread on N = 2144 symbols: var(ma^2) / ma^4 = 4 sigma^2 / (N A^2),
        # var(noise power) / noise^2 = 2 / N, together 0.0014 -> (10 / ln 10) sqrt(0.0014) = 0.16 dB; five of those
        db = 10 * math.log10(r["ma"] ** 2 / (2 * (r["m2"] - r["ma"] ** 2)))
        assert abs(db - 3.01) < 0.8, (k, db)


def test_bound_is_what_the_derivation_says():
    assert BOUND == 2146 * 2.0 ** -53
