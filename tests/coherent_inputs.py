"""The coherent front-end's (`-c`, csrc/k_coherent.hip) captures, settings and oracle-side quantities, CPU only: one definition for
tests/test_coherent_host.py (every condition below holds for the oracle, and the oracle == the compiled reference on every case)
and tests/test_gpu_coherent.py (the kernel against the oracle). Everything is made from the oracle's transmit chain and the numpy
channel model at test time; nothing here needs a device, and nothing is read from a fixture.

How far the reference's Costas loop can be followed is MEASURED per case, on the oracle alone, and how closely is DERIVED:

gain      Oracle.coherent_demodulate runs twice, from carrier_phase0 = 0 and from 1e-9 rad. M = 80 sqrt(2) max|int16 component|
          bounds |c1| + |c2| (40 samples of magnitude <= sqrt(2) max on each tone). g(s) is the running maximum of
          |soft_a - soft_b| up to symbol s over 1e-9 M: how much of a phase perturbation the loop has handed on by then. The
          prefix P is the first symbol with g > 64, or the whole capture if there is none.
envelope  E(s) = max(1, g(s)) [(s + 1) 80 2^-51 + 2^-40] M. The oracle adds each of its three phases 40 times per symbol, each
          addition rounding by at most 2^-51 (the phases stay below 8 in magnitude), where the kernel forms them in closed form
          with one addition; a correlation of magnitude <= M / 2 turns by its tone phase's error plus the carrier's, which is
          M 80 2^-51 per symbol, accumulating. The floor 2^-40 M covers the last places of the device's sincos / hypot / atan2 and
          the order of the 40-term sums. Nothing in E comes from what the kernel gives.
"""
import functools

import numpy as np

from hostile_inputs import slip_capture
from oracle_lib import CODED_BITS, FRAME_SYMBOLS, SPS, Oracle, impair
from soak_inputs import pathological_captures

PERTURB = 1e-9           # rad on the initial carrier phase
GAIN_LIMIT = 64.0
FROZEN, AFC, CLAMPED, LOOP = (0.0, 1.0), (0.001, 1.0), (0.05, 1.0), (0.0, 5000.0)      # (afc_alpha, pll_bw in Hz)
DEFAULT = [(0.001, 50.0), (0.002, 35.0), (0.5, 50.0)]
FO_CLAMP, LOOP_FREQ_CLAMP = 2000.0, 0.1
EDGE_CUTS = [0, 39, 40, 41, 79, 80, 40 * 2167 + 39, 40 * 2168]
# the two gaps of exact zeros in "n300_gaps": whole symbols 5000 .. 5099; from 13 samples into symbol 9000 to 7 samples into 9060
GAP_WHOLE = (5000, 5100)
GAP_RAGGED = (40 * 9000 + 13, 40 * 9060 + 7)


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


# ------------------------------------------------------------------ captures
@functools.lru_cache(maxsize=None)
def captures():
    """name -> int16 IQ. Ten BERT frames of KB5MU from frame 7 (21 780 symbols) through four channels, two captures of the hostile
    set, and what the silence cases need."""
    o = oracle()
    base = o.modulate(o.bert_frames(10, "KB5MU", first=7))
    iq10 = o.modulate(o.bert_frames(10))                       # the hostile set's own base (tests/conftest.py: iq10)
    c = dict(clean=base,
             n300=impair(base, 2000.0, 300.0, 16.0),
             n1200=impair(base, 3000.0, -1200.0, 12.0),
             a16000=impair(base, 16000.0),
             p1900=impair(base, 2500.0, 1900.0, 16.0, seed=5),
             patho0=pathological_captures(iq10)[0],
             slip3000=slip_capture(iq10, 3000.0),
             zeros=np.zeros(2 * (300 * SPS + 22), np.int16))
    # a real constant: with the estimate at exactly 0 Hz the two tone correlations of symbol 0 are exact conjugates, en1 == en2 != 0
    c["dc"] = np.zeros(2 * (200 * SPS + 11), np.int16)
    c["dc"][0::2] = 12345
    g = c["n300"].copy().reshape(-1, 2)
    g[SPS * GAP_WHOLE[0]: SPS * GAP_WHOLE[1]] = 0
    g[GAP_RAGGED[0]: GAP_RAGGED[1]] = 0
    c["n300_gaps"] = g.reshape(-1)
    # four offsets for one context whose streams must each carry their own estimate
    for f0 in (-1530.0, -225.0, 135.0, 1440.0):
        c[f"f0{f0:+.0f}"] = impair(base[: 2 * SPS * 3000], 4000.0, f0, 20.0, seed=int(abs(f0)))
    return {k: np.ascontiguousarray(v) for k, v in c.items()}


FOUR = ["clean", "n300", "n1200", "a16000"]
OFFSETS = ["f0-1530", "f0-225", "f0+135", "f0+1440"]


# ------------------------------------------------------------------ the oracle on one capture and setting
def gain(x, est, setting):
    """-> dict(soft, extra [nsym, 3] = (carrier, loop_freq, fo) behind each symbol, fin = (fo, loop_freq, carrier) behind the
    last, M, g [nsym], P, whole, E [nsym + 1]: E[nsym] is the envelope a symbol behind the last would have (the loop state's)"""
    o = oracle()
    alpha_bw = dict(afc_alpha=setting[0], pll_bw=setting[1])
    a, d, extra = o.coherent_demodulate(x, est, extra=True, carrier_phase0=0.0, **alpha_bw)
    b, _ = o.coherent_demodulate(x, est, carrier_phase0=PERTURB, **alpha_bw)
    nsym = len(a)
    M = 80.0 * np.sqrt(2.0) * float(np.max(np.abs(x.astype(np.int32)))) if x.size else 0.0
    g = np.maximum.accumulate(np.abs(a - b)) / (PERTURB * M) if M > 0.0 else np.zeros(nsym)
    over = np.nonzero(g > GAIN_LIMIT)[0]
    P = int(over[0]) if over.size else nsym
    g1 = np.concatenate([g, g[-1:] if nsym else np.zeros(1)])
    E = np.maximum(1.0, g1) * ((np.arange(nsym + 1) + 1.0) * 80.0 * 2.0 ** -51 + 2.0 ** -40) * M
    return dict(soft=a, extra=extra, fin=(d.freq_offset, d.loop_freq, d.carrier_phase), M=M, g=g, P=P, whole=not over.size, E=E)


def make(x, setting):
    o = oracle()
    exp = o.receive(x, streaming=False, coherent=True, afc_alpha=setting[0], pll_bw=setting[1])
    case = dict(x=x, n=x.size // 2, nsym=x.size // 2 // SPS, setting=setting, exp=exp, est=exp["est_offset"])
    case.update(gain(x, exp["est_offset"], setting))
    assert case["soft"].tobytes() == exp["soft"].tobytes() and case["fin"][0] == exp["final_freq_offset"]
    return case


def _on_clamp(case, column, value):
    """symbols behind which the oracle's loop state `column` of extra sits exactly on `value`"""
    return np.nonzero(case["extra"][:, column] == value)[0]


def _names():
    n = [("tame_frozen", f"frozen-{c}") for c in FOUR] + [("tame_afc", f"afc-{c}") for c in FOUR]
    n += [("tame_afc_clamped", "clamped-n300"), ("tame_afc_clamped", "clamped-p1900"),
          ("tame_afc_clamped", "clamped-cut-hi"), ("tame_afc_clamped", "clamped-cut-lo")]
    n += [("default_prefix", f"default{k}-{c}") for k in range(len(DEFAULT)) for c in FOUR + ["patho0", "slip3000"]]
    n += [("loop_clamp", "loop-clamp"), ("silence", "silence-zeros"), ("silence", "silence-gaps")]
    n += [("edges", f"edge-{cut}") for cut in EDGE_CUTS]
    n += [("offsets", c) for c in OFFSETS] + [("tie", "tie-dc")]
    return n


GROUP = {name: group for group, name in _names()}
CASES = [name for _, name in _names()]


def in_group(group):
    return [n for n in CASES if GROUP[n] == group]


@functools.lru_cache(maxsize=None)
def case(name):
    """The oracle's whole account of one case (computed once per process): the capture `x`, `n`, `nsym`, `setting`, `est`, `exp`
    (Oracle.receive -c) and gain()'s fields."""
    caps = captures()
    kind, _, cap = name.partition("-")
    if kind == "frozen":
        return make(caps[cap], FROZEN)
    if kind == "afc":
        return make(caps[cap], AFC)
    if kind == "clamped" and not cap.startswith("cut"):
        return make(caps[cap], CLAMPED)
    if kind == "clamped":
        # the capture cut behind a symbol K that leaves the oracle's fo exactly on +2000 (hi) / -2000 (lo): the chunk line then
        # shows the loop state right behind symbol K. The cut changes nothing in front of it only if the offset estimate stays
        # the same, which it does from 40 000 samples on (the search reads min(N, 40 000)): K >= 1000.
        full = case("clamped-p1900")
        at = _on_clamp(full, 2, FO_CLAMP if cap == "cut-hi" else -FO_CLAMP)
        K = int(at[at >= 1000][0]) + 1
        c = make(full["x"][: 2 * SPS * K], CLAMPED)
        assert c["est"] == full["est"] and c["soft"].tobytes() == full["soft"][:K].tobytes()
        return c
    if kind.startswith("default"):
        return make(caps[cap], DEFAULT[int(kind[len("default"):])])
    if name == "loop-clamp":
        # K * 40 + 17 samples with K = min(P, 12), P being the cut capture's own (its offset estimate is its own too): the largest
        # such K whose last symbol leaves loop_freq on its clamp, so that the chunk line shows it
        for K in range(12, 0, -1):
            c = make(caps["p1900"][: 2 * (SPS * K + 17)], LOOP)
            if c["P"] == K and abs(c["fin"][1]) == LOOP_FREQ_CLAMP:
                return c
        raise AssertionError("no cut of the capture ends inside the prefix with loop_freq on its clamp")
    if name == "silence-zeros":
        return make(caps["zeros"], AFC)
    if name == "silence-gaps":
        return make(caps["n300_gaps"], AFC)
    if kind == "edge":
        return make(caps["n300"][: 2 * int(cap)], AFC)
    if name == "tie-dc":
        return make(caps["dc"], AFC)
    if kind.startswith("f0"):
        return make(caps[name], AFC)
    raise KeyError(name)


# ------------------------------------------------------------------ which of the oracle's frames a soft log inside E must give
@functools.lru_cache(maxsize=None)
def tracked(name):
    """Oracle.track over the case's oracle soft log (every released frame, dropped ones too)"""
    return oracle().track(case(name)["soft"])


def fragile_frames(name):
    """One bool per frame the oracle's tracker released: True where some soft symbol of its payload lies so close to a decision
    that a log within E of the oracle's may decide otherwise. The decoder (FrameDecoder::decode) divides by scale = mean |soft|
    over the payload and quantises v = int(3.5 - 3.5 soft / scale + 0.5) to 0 .. 7: the boundaries are soft = scale (4 - k) / 3.5
    for k = 1 .. 7, zero among them. A log within E moves a symbol by <= E(s) and the scale by <= max E over the payload, i.e. a
    boundary by <= |4 - k| / 3.5 of that: a symbol within E(s) + max E of a boundary is fragile (an upper bound on both terms)."""
    c, t = case(name), tracked(name)
    out = []
    for r, p in zip(t["frame_sym"].astype(np.int64), t["payloads"]):
        assert p.tobytes() == c["soft"][r - (CODED_BITS - 1): r + 1].tobytes()
        E = c["E"][r - (CODED_BITS - 1): r + 1]
        scale = np.mean(np.abs(p))
        bounds = scale * (4.0 - np.arange(1, 8)) / 3.5
        dist = np.min(np.abs(p[:, None] - bounds[None, :]), axis=1)
        out.append(bool(np.any(dist <= E + E.max())))
    return np.array(out, bool)


__all__ = ["AFC", "CASES", "CLAMPED", "DEFAULT", "EDGE_CUTS", "FO_CLAMP", "FOUR", "FRAME_SYMBOLS", "FROZEN", "GAP_RAGGED", "GAP_WHOLE",
           "GROUP", "LOOP", "LOOP_FREQ_CLAMP", "OFFSETS", "case", "captures", "fragile_frames", "gain", "in_group", "make", "oracle", "tracked"]
