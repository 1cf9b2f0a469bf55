"""CPU model of the per-frame link report (include/opv_demod.h: opv_link) for ONE payload of 2144 soft symbols, built on the
oracle alone: q and the decoded frame from oracle.frame_decode, the expected channel bits from oracle.encode_frame.

    rec = link_model(oracle, soft)      # dict(valid, bit_errors, weak, nonfinite, m1, m2, ma, frame, metric, enc, q)
    check_record(dev, rec, tag)         # the comparison every test uses

The integers are exact. m1 is the decoder's scale, summed sequentially like the reference (src/opv-demod.cpp:856-858). m2 and ma are
math.fsum (the correctly rounded sum) of the once-rounded products, divided by 2144; a sum that is not finite - non-finite
terms, or finite terms that overflow - is reported as nan.

Bound for m2 and ma: the device adds 2144 once-rounded products in an unspecified but fixed order. Any order of N additions is
within (N - 1) u sum|terms| of the exact sum of its terms (u = 2^-53, first order), the products add u sum|terms|, the final
division one more rounding: |dev - model| <= (N + 2) u sum|terms| / N = 2146 x 2^-53 x B with B = sum|terms| / N, which is m2
for m2 and m1 for ma (|soft_i e_i| = |soft_i|)."""
import math

import numpy as np

CODED = 2144
U = 2.0 ** -53
BOUND = (CODED + 2) * U


def _fsum_mean(terms):
    try:
        v = math.fsum(terms) / CODED
    except (OverflowError, ValueError):                     # finite terms whose sum overflows; +inf and -inf among the terms
        return math.nan
    return v if math.isfinite(v) else math.nan


def link_model(oracle, soft):
    soft = np.ascontiguousarray(soft, np.float64).reshape(CODED)
    d = oracle.frame_decode(soft)
    if d["metric"] < 0:                                     # dropped (ref :859): valid = 0, every field 0
        return dict(valid=0, bit_errors=0, weak=0, nonfinite=0, m1=0.0, m2=0.0, ma=0.0, frame=d["frame"], metric=d["metric"],
                    enc=None, q=None)
    enc = oracle.encode_frame(d["frame"])
    q = d["q"]
    m1 = 0.0
    for v in soft.tolist():                                 # sequential, in index order
        m1 += abs(v)
    m1 /= CODED
    e = 1.0 - 2.0 * enc.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = soft * soft                                    # once-rounded products
        se = soft * e                                       # exact
    return dict(valid=1, bit_errors=int(((q >= 4) != (enc != 0)).sum()), weak=int(((q == 3) | (q == 4)).sum()),
                nonfinite=int((~np.isfinite(soft)).sum()), m1=m1, m2=_fsum_mean(sq.tolist()), ma=_fsum_mean(se.tolist()),
                frame=d["frame"], metric=d["metric"], enc=enc, q=q)


def check_record(dev, rec, tag):
    """one device record (a LINK_DTYPE element) against the model: integers ==; m1 == and m2 / ma within the bound wherever
    nonfinite == 0; where the model's m2 / ma is not finite the device's must not be either. Prints nothing, asserts."""
    for k in ("valid", "bit_errors", "weak", "nonfinite"):
        assert int(dev[k]) == rec[k], (tag, k, int(dev[k]), rec[k])
    if rec["valid"] == 0:
        assert float(dev["m1"]) == 0.0 and float(dev["m2"]) == 0.0 and float(dev["ma"]) == 0.0, (tag, dev)
        return
    if rec["nonfinite"]:
        return                                              # m1 / m2 / ma unspecified
    assert float(dev["m1"]) == rec["m1"], (tag, "m1", float(dev["m1"]), rec["m1"])
    for k, b in (("m2", rec["m2"]), ("ma", rec["m1"])):
        got, exp = float(dev[k]), rec[k]
        if math.isfinite(exp):
            assert abs(got - exp) <= BOUND * b, (tag, k, got, exp, abs(got - exp), BOUND * b)
        else:
            assert not math.isfinite(got), (tag, k, got, exp)
