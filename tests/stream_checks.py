"""What a stream of the product is compared with the oracle BY: the soft-symbol bounds, the tracker-event rule, the two reported
input classes and check_stream, which every GPU module of the suite holds its streams to. One definition each; the tests of
tests/test_gpu_parity.py and the other GPU modules import them from here. Needs no device to import."""
import numpy as np

from hostile_inputs import gapped_capture as _gapped_capture  # noqa: F401  (the silence-gap capture, under the name its users know)
from oracle_lib import format_events

SOFT_RTOL = 1e-5      # contract (BASELINE.json north_star)
SOFT_TIGHT = 1e-9     # what fp64 re-association actually leaves (SURVEY.md §7-3 measured 6e-12)


def soft_err(a, b):
    assert a.shape == b.shape
    scale = np.mean(np.abs(b)) + 1e-300
    abs_norm = np.max(np.abs(a - b)) / scale
    big = np.abs(b) > 1e-3 * scale
    rel = np.max(np.abs(a[big] - b[big]) / np.abs(b[big])) if big.any() else 0.0
    return abs_norm, rel


RAW_FIELD = __import__("re").compile(r"raw=(-?\d+)\)")


def events_match(amd, got_ev, exp_ev):
    """Tracker events: kind, symbol index and counters are integers -> exact. corr / raw are fp64
    sums of soft symbols, which agree with the reference to ~1e-14 relative, not bit for bit. The printed
    lines must be IDENTICAL except for one field: the integer printed by `raw=%.0f` in the HUNTING->VERIFYING
    line (a 12-digit number: the signed sum of 24 soft symbols) may differ in its last place(s) - by at most
    1 + 2e-11 |raw|, i.e. one unit for the 1e10-scale sums of the amplitude-2000 captures and a few units for
    full-scale ones (soft symbols ~4e11, agreeing to ~3e-13 each). Everything else in every line - including
    corr=%.3f - is compared as text. How many lines may carry a difference follows from the values themselves:
    a rounding boundary falls between two numbers d apart with probability min(1, d), so the expected count is
    the sum of that over the printed lines (~1e-3 per line at 16 dB / amplitude 2000, ~0.1 at 6 dB where the soft
    symbols sit at the reference's own 2.5e-10 noise floor); the bound is that expectation plus four standard
    deviations, plus one."""
    assert len(got_ev) == len(exp_ev), "number of tracker events differs"
    if len(exp_ev) == 0:
        return 0
    for k in ("kind", "count", "sym_idx"):
        assert np.array_equal(got_ev[k], exp_ev[k]), f"tracker event field {k} differs"
    assert np.allclose(got_ev["corr"], exp_ev["corr"], rtol=0, atol=1e-9)
    # raw is a signed sum of 24 soft symbols (cancellation is normal on noise): absolute tolerance on
    # the scale of the soft symbols, i.e. of the largest |raw| seen
    assert np.allclose(got_ev["raw"], exp_ev["raw"], rtol=0, atol=1e-8 * (np.max(np.abs(exp_ev["raw"])) + 1.0))
    a, b = amd.format_events(got_ev), format_events(exp_ev)
    ndiff = 0
    for x, y in zip(a, b):
        if x == y:
            continue
        # the only licence: the raw= integer, off by one
        assert RAW_FIELD.sub("raw=#)", x) == RAW_FIELD.sub("raw=#)", y), f"tracker line differs outside raw=: {x!r} vs {y!r}"
        rx, ry = RAW_FIELD.search(x), RAW_FIELD.search(y)
        assert rx and ry and abs(int(rx.group(1)) - int(ry.group(1))) <= 1 + 2e-11 * abs(int(ry.group(1))), \
            f"raw= differs by more than its last place: {x!r} vs {y!r}"
        ndiff += 1
    printed = exp_ev["kind"] == 1                       # only the HUNTING->VERIFYING line prints raw=
    expect = float(np.sum(np.minimum(1.0, np.abs(got_ev["raw"][printed] - exp_ev["raw"][printed]))))
    assert ndiff <= 1 + expect + 4.0 * np.sqrt(expect), \
        f"{ndiff} of {int(printed.sum())} raw= fields differ in the last digit, {expect:.2f} expected from the values"
    return ndiff


def no_ties(st, tag="", edge_ties=0, offset_ties=0):
    """The two input classes the product reports (include/opv_demod.h). edge_ties (reference src/opv-demod.cpp:272,291: a
    tone choice decided by the rounding of the reference's own LO) is NOT reproduced and must not occur on ordinary
    captures: a regression that starts to hit it would otherwise pass. offset_ties (:161,195) counts offset-search
    candidates the near-tie guard re-evaluated in the reference's order - reproduced, the estimate is compared with the
    oracle's wherever this is called - but a guard that fires on ordinary captures more than once in several hundred streams
    (two fine candidates within 1e-11 where neighbours are ~1e-8 apart) would mean the one-pass evaluation lost accuracy.
    offset_ties=None: counted by the caller."""
    assert st.edge_ties == edge_ties, f"{tag}: edge_ties {st.edge_ties} (expected {edge_ties})"
    if offset_ties is not None:
        assert st.offset_ties == offset_ties, f"{tag}: offset_ties {st.offset_ties} (expected {offset_ties})"


def check_stream(amd, got, exp, tag="", edge_ties=0, offset_ties=0):
    no_ties(got["state"], tag, edge_ties, offset_ties)
    assert np.array_equal(got["frames"], exp["frames"]), f"{tag}: decoded bytes differ"
    assert np.array_equal(got["meta"]["viterbi_metric"], exp["metrics"]), f"{tag}: Viterbi metrics differ"
    assert np.array_equal(got["meta"]["release_symbol"], exp["frame_sym"]), f"{tag}: sync positions differ"
    events_match(amd, got["events"], exp["events"])
    assert got["state"].total_symbols == exp["n_soft"]
    a, r = soft_err(got["soft"], exp["soft"])
    print(f"{tag}: soft max|d|/mean|soft| = {a:.3e}, max rel = {r:.3e}")
    assert a < SOFT_RTOL and r < SOFT_RTOL
    assert a < SOFT_TIGHT, f"{tag}: soft error {a:.3e} far above fp64 re-association level"
    e0, e1 = got["state"].est_offset_hz, exp["est_offset"]
    assert (np.isnan(e0) and np.isnan(e1)) or e0 == e1, f"{tag}: offset estimate {e0} vs {e1}"
    assert abs(got["state"].freq_offset_hz - exp["final_freq_offset"]) < 1e-6
    assert got["state"].sync_state == exp["final_state"]
    ch = got["chunks"]
    assert len(ch) == len(exp["chunks"])
    assert np.array_equal(ch[:, 3:], exp["chunks"][:, 3:])          # leftover, symbols per call
    assert np.allclose(ch[:, :3], exp["chunks"][:, :3], rtol=0, atol=1e-7)


def _visible_gpus():
    try:
        import torch
        return torch.cuda.device_count()           # (does not initialise a GPU on this image)
    except Exception:
        return 0
