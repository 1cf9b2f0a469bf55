"""What the four GPU modules of the wideband converters (tests/test_gpu_wideband*.py) share: device buffers with canaries, the
sources a push can take, the inputs and preconditions of the exactness cases, and the two end-to-end plans with the fixtures'
CPU halves - the D = 4 plan at 8.672 MS/s (PLAN_D4) and the 1250 / 271 plan at 10 MS/s (PLAN_10M), each with its taps, capture,
object and stream check under a name of its own. The models are tests/wideband_models.py; the bounds tests/stream_checks.py.
Importing needs no device: torch arrives through the torch_dev fixture."""
import numpy as np

from oracle_lib import impair
from stream_checks import SOFT_TIGHT, check_stream, events_match
from stream_runs import CHUNK, collect
from wideband_models import (WIDE_RATE, per_phase_taps, tx_phase_taps, wb_model, wb_model_inc, wbr_model, wbr_model_inc,
                             wbtxr_outputs)

CANARY, GAP = 0x5A5B, 64                 # int16 fill of what a push must not touch; int16 per canary


# ------------------------------------------------------------------ device buffers
class Sources:
    """one wide capture as the three kinds of source a push can take: views of a pinned copy, of a pageable copy, of a device copy"""

    def __init__(self, torch_dev, wide):
        torch, dev = torch_dev
        self.pinned_t = torch.from_numpy(wide.copy()).pin_memory()
        self.pinned = self.pinned_t.numpy()
        self.pageable = wide.copy()
        self.dev_t = self.pinned_t.to(dev)
        torch.cuda.synchronize()

    def push(self, wb, kind, lo, hi):
        """wide samples [lo, hi)"""
        if kind == "device":
            wb.push_device(self.dev_t.data_ptr() + 4 * lo, hi - lo)
        else:
            wb.push((self.pinned if kind == "pinned" else self.pageable)[2 * lo: 2 * hi])


class Out:
    """a device buffer of n wide samples between two canaries; everything starts as canary"""

    def __init__(self, torch_dev, n):
        torch, dev = torch_dev
        self.n = n
        self.buf = torch.full((2 * n + 2 * GAP,), CANARY, dtype=torch.int16, device=dev)

    def ptr(self, at=0):
        return self.buf.data_ptr() + 2 * GAP + 4 * at

    def get(self):
        """the n samples, after asserting that both canaries are intact"""
        x = self.buf.cpu().numpy()
        assert (x[:GAP] == CANARY).all() and (x[-GAP:] == CANARY).all(), "a push wrote outside its output"
        return x[GAP:-GAP]


class Inputs:
    """chans[k] (interleaved int16 IQ, the same length each) in one device tensor, a row per channel"""

    def __init__(self, torch_dev, chans):
        torch, dev = torch_dev
        self.t = torch.from_numpy(np.stack(chans)).to(dev)
        self.row = self.t.stride(0) * 2
        torch.cuda.synchronize()

    def ptr(self, k, at=0):
        return self.t.data_ptr() + k * self.row + 4 * at


def assert_equal(got, exp, tag):
    assert got.size == exp.size, (tag, got.size, exp.size)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{tag}: {bad.size} of {got.size} values differ, first at {bad[0]}: {got[bad[0]]} vs {exp[bad[0]]}"


def push_pieces(tx, src, out, M, U, K, cuts):
    """pushes inputs [cuts[i], cuts[i + 1]) of every channel in turn, each to where the rational count puts it in `out`"""
    for lo, hi in zip(cuts, cuts[1:]):
        tx.push([src.ptr(k, lo) for k in range(K)], hi - lo, out.ptr(wbtxr_outputs(M, U, lo)))
        assert tx.samples() == hi


# ------------------------------------------------------------------ the exactness cases: inputs and preconditions
def exactness_inputs(kind, rng, side, fw, K, N, L, phases, halfway_taps=(1, 1)):
    """-> (inputs, taps, centres) of an exactness case, drawn from rng in this order: K centres uniform in +/- fw / 2, the inputs
    (N samples of interleaved int16 IQ each: ONE wide capture on the receive side "rx", K channels on the transmit side "tx"; the
    small-valued kinds have one whatever K is), the taps (L of them, the filter's cap held on each of its `phases` phases).
      random     full-range inputs, random taps
      fullscale  inputs of -32768 / 32767 that begin with runs of 40 equal values, Hamming taps of gain ~4: both clamps fire
      small      +/-9 and one tap of 3, unit: +/-1 and one tap of 1 (out_shift = 0: products, no rounding term); small at centre 0
      halfway    +/-7 at centre 0 and `halfway_taps`: sums of 32767 x I, half-way between two outputs wherever I = 4 (mod 8)
      bound      every channel -32768 at centre 0 and the taps -32768, -32767: the largest sum the transmit side's limits allow"""
    assert side in ("rx", "tx")
    n_inputs = 1 if side == "rx" else K
    centres = list(rng.uniform(-fw / 2, fw / 2, K))

    def fullscale():
        x = rng.choice(np.array([-32768, 32767], np.int16), 2 * N)
        x[: 2 * 600] = np.repeat(rng.choice(np.array([-32768, 32767], np.int16), 2 * 600 // 40), 40)     # runs: the filter's sum builds up
        return x
    if kind == "random":
        inputs = [rng.integers(-32768, 32768, 2 * N).astype(np.int16) for _ in range(n_inputs)]
        taps = per_phase_taps(rng, L, phases) if side == "rx" else tx_phase_taps(rng, L, phases)
    elif kind == "fullscale":
        inputs = [fullscale() for _ in range(n_inputs)]
        h = np.hamming(L)
        # rx: gain 3.9 x 2^19 x 32767 / 2^34 = 3.9: runs of full scale leave the int16 range; tx: 65000 x 32767 / 2^29 = 3.97 per channel
        taps = np.rint(h / h.sum() * (3.9 * (1 << 19) if side == "rx" else 65000)).astype(np.int16)
    elif kind == "small":
        centres[0] = 0.0
        inputs, taps = [rng.integers(-9, 10, 2 * N).astype(np.int16)], np.array([3], np.int16)
    elif kind == "unit":
        inputs, taps = [rng.integers(-1, 2, 2 * N).astype(np.int16)], np.array([1], np.int16)          # |I c - Q s| <= 46340: some clamp, most do not
    elif kind == "halfway":
        centres[0] = 0.0
        inputs, taps = [rng.integers(-7, 8, 2 * N).astype(np.int16)], np.array(halfway_taps, np.int16)  # (|32767 x 7| / 8 stays inside int16: no clamp hides the rounding)
    else:
        assert kind == "bound"
        centres = [0.0] * K
        inputs, taps = [np.full(2 * N, -32768, np.int16) for _ in range(n_inputs)], np.array([-32768, -32767], np.int16)
    assert len(taps) == L
    return inputs, taps, centres


def assert_exactness_preconditions(kind, exp, unclamped=(), halfway=None):
    """what the MODEL's output `exp` must show before the device is asked for it, by the case's kind:
      a kind named in `unclamped`: the case does not hide behind the clamp
      fullscale  both clamps fire, and some outputs are inside
      halfway    halfway = (w, out): w, the sums before rounding (int64, S = 3), has negative half-way values; out, the model's
                 outputs for them, is their floor, and neither rounding half away from zero nor C's truncating division gives it
      bound      the sum is 256 y c, just under 2^54 per component of the 2^55 bound, and comes out unclamped after S = 40"""
    inside = np.abs(exp.astype(np.int32)) < 32767
    if kind in unclamped:
        assert inside.mean() > 0.6 and np.unique(exp).size > 100, "the case must not hide behind the clamp"
    if kind == "fullscale":
        assert (exp == 32767).sum() > 10 and (exp == -32768).sum() > 10 and inside.sum() > 10
    if kind == "halfway":
        w, out = halfway
        half = (w < 0) & (w % 8 == 4)
        assert half.sum() > 5
        assert np.array_equal(out, (w + 4) >> 3)                           # floor
        away = np.sign(w) * ((np.abs(w) + 4) >> 3)                         # round half away from zero / truncation of the magnitude
        trunc = np.trunc((w + 4) / 8.0).astype(np.int64)                   # C's division, which truncates
        assert (away != out).any() and (trunc != out).any()
    if kind == "bound":
        # per channel y = 65535 x 32768 = 2^31 - 2^15 (the largest |y| the limits allow), c = 32767
        total = 256 * (65535 * 32768) * 32767
        assert (1 << 53) < total < (1 << 55) and (exp[2:] == (total + (1 << 39)) >> 40).all() and 0 < exp[2] < 32767


def run_absent_channel_schedule(tx, src, out, schedule, K, fed, out_at):
    """the pushes of test_any_split_absent_channels_shared_buffers_and_reset: (n_in, channels present) in turn, channel 3 always
    reading channel 0's buffer, an absent channel handed over as null; `fed` (what the model is to be fed) gets zeros where a channel
    was absent. out_at(n): the wide sample the outputs of input n start at."""
    at = 0
    for n, present in schedule:
        for k in range(K):
            if k not in present:
                fed[k][2 * at: 2 * (at + n)] = 0
        tx.push([src.ptr(0 if k == 3 else k, at) if k in present else None for k in range(K)], n, out.ptr(out_at(at)))
        at += n
        assert tx.samples() == at


def loopback_on_the_cpu(amd, oracle, loop, up_model, down_model):
    """the loopback chain on the CPU, from the two models and the oracle alone: -> dict(tx[k], chans[k], wide, model[k], exp[k]). All
    three channels start at sample 0 and the run ends with the modulator's 4000 silent samples. up_model(T, chans) -> the wide
    capture, down_model(T, wide) -> the four slots' IQ."""
    F = loop["frames"]
    tx = [amd.bert_frames(F, "WT%d" % k, first=10 * k) for k in range(3)]
    chans = [amd.modulate(f) for f in tx]
    for x in chans:
        assert x.size == 2 * (F * CHUNK + loop["tail"]) and not x[2 * F * CHUNK:].any()           # the tail is silence: an all-null push makes it
    T = amd.wb_lo_table()
    wide = up_model(T, chans)
    assert 8000 < np.max(np.abs(wide.astype(np.int32))) < 32767           # well inside int16: no clamp between the banks
    model = down_model(T, wide)
    exp = [oracle.receive(model[k], streaming=True) for k in range(4)]
    # the precondition, from the reference alone: every transmitted frame on slots 0 - 2, nothing on the empty slot
    for k in range(3):
        assert np.array_equal(exp[k]["frames"], tx[k]), f"loopback plan: the oracle alone does not decode channel {k}"
    assert len(exp[3]["frames"]) == 0, "loopback plan: the oracle releases frames on the empty slot"
    return dict(tx=tx, chans=chans, wide=wide, model=model, exp=exp)


# ------------------------------------------------------------------ the D = 4 plan (tests/test_gpu_wideband.py's docstring)
PLAN_D4 = dict(D=4, centres=[-1100000.0, 0.0, 1600000.0, 2700000.0], L=321, cutoff_hz=200000.0, out_shift=30,
               channels={0: dict(amp=3000.0, f0_hz=1700.0, ebn0_db=None), 1: dict(amp=1000.0, f0_hz=600.0, ebn0_db=12.0),
                         2: dict(amp=3000.0, f0_hz=-1900.0, ebn0_db=None)}, empty=3, seed=70)
LOOP_D4 = dict(U=4, centres=PLAN_D4["centres"][:3], out_shift=32, frames=2, tail=4000)


def plan_taps_d4():
    L, fs = PLAN_D4["L"], PLAN_D4["D"] * WIDE_RATE
    t = np.arange(L) - (L - 1) / 2
    h = np.sinc(2 * PLAN_D4["cutoff_hz"] / fs * t) * np.hamming(L)
    taps = np.rint(h / h.sum() * (1 << 15)).astype(np.int16)
    assert np.abs(taps.astype(np.int64)).sum() <= 1 << 21
    return taps


def loop_taps_d4():
    """PLAN_D4's 321-tap Hamming sinc scaled to sum 4 x 2^15: unity gain through the zero-stuffing by 4 (x 32767 / 2^32 from the LO)"""
    L, fs = PLAN_D4["L"], PLAN_D4["D"] * WIDE_RATE
    t = np.arange(L) - (L - 1) / 2
    h = np.sinc(2 * PLAN_D4["cutoff_hz"] / fs * t) * np.hamming(L)
    taps = np.rint(h / h.sum() * 4 * (1 << 15)).astype(np.int16)
    assert all(np.abs(taps[p::4].astype(np.int64)).sum() <= 65535 for p in range(4))
    return taps


def make_plan_capture_d4(amd, oracle, n_frames, empty_is_silent=True):
    """-> dict(wide, taps, tx[k], model[k] (int16 IQ per slot), exp[k] (the oracle on model[k]))"""
    D, centres = PLAN_D4["D"], PLAN_D4["centres"]
    fs = D * WIDE_RATE
    tx, z = {}, None
    for k, c in PLAN_D4["channels"].items():
        tx[k] = amd.bert_frames(n_frames, "WB%d" % k, first=10 * k)
        iq = impair(amd.modulate(tx[k]), amp=c["amp"], f0_hz=c["f0_hz"], ebn0_db=c["ebn0_db"], seed=PLAN_D4["seed"] + k)
        zk = np.repeat(iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64), D)           # repeated by D ...
        zk = zk * np.exp(2j * np.pi * centres[k] / fs * np.arange(zk.size, dtype=np.float64))       # ... mixed up ...
        z = zk if z is None else z + zk                                                           # ... and summed
    assert max(np.max(np.abs(z.real)), np.max(np.abs(z.imag))) < 32767
    wide = np.empty(2 * z.size, np.int16)
    wide[0::2], wide[1::2] = np.rint(z.real), np.rint(z.imag)
    taps = plan_taps_d4()
    model = wb_model(amd.wb_lo_table(), wide, D, wb_model_inc(D, centres), taps, PLAN_D4["out_shift"])
    exp = [oracle.receive(model[k], streaming=True) for k in range(len(centres))]
    # the precondition, from the reference alone: every transmitted frame of every channel, the 12 dB one included (at least 2 each),
    # nothing from the empty slot
    for k in PLAN_D4["channels"]:
        assert np.array_equal(exp[k]["frames"], tx[k]), f"plan: the oracle alone does not decode channel {k}"
        assert len(exp[k]["frames"]) >= 2
    if empty_is_silent:
        assert len(exp[PLAN_D4["empty"]]["frames"]) == 0, "plan: the oracle releases frames on the empty slot"
    return dict(wide=wide, taps=taps, tx=tx, model=model, exp=exp)


def plan_wideband_d4(amd, d, first_sample=0):
    return amd.Wideband(d, PLAN_D4["D"], list(range(len(PLAN_D4["centres"]))), PLAN_D4["centres"], plan_taps_d4(), PLAN_D4["out_shift"], first_sample)


def check_plan_streams_d4(amd, d, cap, tag):
    for k, exp in enumerate(cap["exp"]):
        got = collect(d, k)
        assert got["state"].stalled == 0
        check_stream(amd, got, exp, f"{tag} slot {k}", edge_ties=0, offset_ties=None)
    assert len(cap["exp"][PLAN_D4["empty"]]["frames"]) == 0 and d.state(PLAN_D4["empty"]).frames_released == 0       # the empty slot releases none


# ------------------------------------------------------------------ the 1250 / 271 plan (tests/test_gpu_wideband_rational.py's docstring)
PLAN_10M = dict(down=1250, up=271, centres=[-3100000.0, 0.0, 1700000.0, 3900000.0], J=96, cutoff_hz=200000.0, out_shift=30,
                channels={0: dict(PLAN_D4["channels"][0]), 1: dict(PLAN_D4["channels"][1], ebn0_db=14.0), 2: dict(PLAN_D4["channels"][2])},
                empty=3, seed=70)
LOOP_10M = dict(down=PLAN_10M["down"], up=PLAN_10M["up"], centres=PLAN_10M["centres"][:3], out_shift=32, frames=2, tail=4000)


def plan_taps_10m(J=None):
    U, M = PLAN_10M["up"], PLAN_10M["down"]
    L = (J or PLAN_10M["J"]) * U
    fs = U * (M * WIDE_RATE / U)                                           # the prototype runs at up x the wide rate
    t = np.arange(L) - (L - 1) / 2
    h = np.sinc(2 * PLAN_10M["cutoff_hz"] / fs * t) * np.hamming(L)
    taps = np.rint(h / h.sum() * U * (1 << 15)).astype(np.int16)            # every phase sums to about 2^15: unity gain with out_shift = 30
    assert max(np.abs(taps[p::U].astype(np.int64)).sum() for p in range(U)) <= 1 << 21
    return taps


def loop_taps_10m():
    """the door's prototype (Hamming-windowed sinc, cutoff 200 kHz, at 1250 x 2.168 MS/s) cut to L = 100 002 - 96 x 271 = 73 986 taps
    (J = 60), so that the two filters' delays add to exactly one symbol, and scaled to sum 1250 x 2^15: unity gain through the
    zero-stuffing by 1250 (x 32767 / 2^32 from the LO)"""
    M = LOOP_10M["down"]
    L = 100002 - PLAN_10M["J"] * PLAN_10M["up"]
    assert L == 73986 and -(-L // M) == 60 and (L - 1) + (PLAN_10M["J"] * PLAN_10M["up"] - 1) == 2 * 40 * M
    t = np.arange(L) - (L - 1) / 2
    h = np.sinc(2 * PLAN_10M["cutoff_hz"] / (M * WIDE_RATE) * t) * np.hamming(L)
    taps = np.rint(h / h.sum() * M * (1 << 15)).astype(np.int16)
    assert max(np.abs(taps[p::M].astype(np.int64)).sum() for p in range(M)) <= 65535
    return taps


def fft_resample(z, up_to, down_from):
    """z at rate F -> rate F x up_to / down_from by zero-padding its spectrum (z is padded to a multiple of down_from first)"""
    n = -(-z.size // down_from) * down_from
    Z = np.fft.fft(np.concatenate([z, np.zeros(n - z.size, z.dtype)]))
    m = n // down_from * up_to
    W = np.zeros(m, np.complex128)
    W[: n // 2], W[m - (n - n // 2):] = Z[: n // 2], Z[n // 2:]
    return np.fft.ifft(W) * (m / n)


def make_channel_10m(amd, k, n_frames):
    c = PLAN_10M["channels"][k]
    tx = amd.bert_frames(n_frames, "WB%d" % k, first=10 * k)
    iq = impair(amd.modulate(tx), amp=c["amp"], f0_hz=c["f0_hz"], ebn0_db=c["ebn0_db"], seed=PLAN_10M["seed"] + k)
    return tx, fft_resample(iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64), PLAN_10M["down"], PLAN_10M["up"])


def to_wide(z):
    assert max(np.max(np.abs(z.real)), np.max(np.abs(z.imag))) < 32767
    wide = np.empty(2 * z.size, np.int16)
    wide[0::2], wide[1::2] = np.rint(z.real), np.rint(z.imag)
    return wide


def make_plan_wide_10m(amd, n_frames):
    """-> (wide int16 IQ, tx[k]): the plan's channels side by side at 10 MS/s, before the door (host code only)"""
    M, U, centres = PLAN_10M["down"], PLAN_10M["up"], PLAN_10M["centres"]
    fw = M * WIDE_RATE / U
    tx, z = {}, None
    for k in PLAN_10M["channels"]:
        tx[k], zk = make_channel_10m(amd, k, n_frames)
        zk = zk * np.exp(2j * np.pi * centres[k] / fw * np.arange(zk.size, dtype=np.float64))
        z = zk if z is None else z + zk
    return to_wide(z), tx


def first_one_tap_window(exp):
    """the oracle's first one-tap window (soft = -/+2^-31: hostile_inputs.ambiguous), or n_soft if it shows none"""
    amb = np.nonzero((exp["soft"] != 0) & (np.abs(exp["soft"]) < 1.0))[0]
    return (int(amb[0]) if amb.size else exp["n_soft"]), amb.size


def make_plan_capture_10m(amd, oracle, n_frames):
    """-> dict(wide, taps, tx[k], model[k] (int16 IQ per slot), exp[k] (the oracle on model[k]))"""
    M, U, centres = PLAN_10M["down"], PLAN_10M["up"], PLAN_10M["centres"]
    wide, tx = make_plan_wide_10m(amd, n_frames)
    taps = plan_taps_10m()
    model = wbr_model(amd.wb_lo_table(), wide, M, U, wbr_model_inc(M, U, centres), taps, PLAN_10M["out_shift"])
    exp = [oracle.receive(model[k], streaming=True) for k in range(len(centres))]
    for k in PLAN_10M["channels"]:                                         # the precondition, from the reference alone
        assert np.array_equal(exp[k]["frames"], tx[k]), f"plan: the oracle alone does not decode channel {k}"
        assert len(exp[k]["frames"]) >= 2
    assert len(exp[PLAN_10M["empty"]]["frames"]) == 0, "plan: the oracle releases frames on the empty slot"
    # which check a slot gets is read off the oracle's output alone (check_plan_streams_10m): the noisy channel must get the full
    # one, and on the clean ones every one-tap window must lie behind the symbols of both frames, in the modulator's tail of zeros
    assert first_one_tap_window(exp[1])[1] == 0
    for k in (0, 2):
        assert first_one_tap_window(exp[k])[0] >= n_frames * 2168, f"plan: channel {k} has a one-tap window inside its frames"
    return dict(wide=wide, taps=taps, tx=tx, model=model, exp=exp)


def plan_wideband_10m(amd, d, first_sample=0):
    return amd.Wideband.rational(d, PLAN_10M["down"], PLAN_10M["up"], list(range(len(PLAN_10M["centres"]))), PLAN_10M["centres"], plan_taps_10m(),
                                 PLAN_10M["out_shift"], first_sample)


def check_up_to_the_first_window(amd, st, frames, meta, events, log, exp, tag, soft=None):
    """A stream whose ORACLE output shows one-tap windows (a clean channel behind this door is digitally silent wherever the
    modulator's capture is: its 40 leading and 4000 trailing zeros - no other channel's images leak in, as they do behind the
    zero-order hold of the D = 4 plan): there the reference's tone choice is the rounding of its own LO, which the
    product reports in edge_ties and does not reproduce (include/opv_demod.h), so the suite's rule for that class applies
    (stream_runs.check_capture): soft symbols, chunk rows and tracker lines up to the oracle's first such window,
    every frame, metric and release symbol, the symbol count and the offset estimate; edge_ties at most the oracle's windows.
    Measured on the MI355X on the plan's slot 0 (one window counted, at a symbol behind both frames): soft symbols within 2.3e-12
    of their mean over the WHOLE run, the last chunk row's carried frequency 7.7e-4 Hz off, everything else ==."""
    k_end, n_amb = first_one_tap_window(exp)
    assert n_amb >= 1 and st.stalled == 0 and st.edge_ties <= n_amb, f"{tag}: edge_ties {st.edge_ties}, the oracle shows {n_amb} one-tap windows"
    assert st.total_symbols == exp["n_soft"], f"{tag}: {st.total_symbols} symbols, oracle {exp['n_soft']}"
    assert np.array_equal(frames, exp["frames"]), f"{tag}: decoded bytes differ"
    assert np.array_equal(meta["viterbi_metric"], exp["metrics"]), f"{tag}: Viterbi metrics differ"
    assert np.array_equal(meta["release_symbol"], exp["frame_sym"]), f"{tag}: sync positions differ"
    e0, e1 = st.est_offset_hz, exp["est_offset"]
    assert (np.isnan(e0) and np.isnan(e1)) or e0 == e1, f"{tag}: offset estimate {e0} vs {e1}"
    events_match(amd, events[events["sym_idx"] < k_end], exp["events"][exp["events"]["sym_idx"] < k_end])
    if soft is not None and k_end:
        assert len(soft) == exp["n_soft"]
        a = float(np.max(np.abs(soft[:k_end] - exp["soft"][:k_end]))) / (np.mean(np.abs(exp["soft"])) + 1e-300)
        assert a < SOFT_TIGHT, f"{tag}: soft error {a:.3e} before symbol {k_end}"
    ech = exp["chunks"]
    done = np.nonzero(np.cumsum(ech[:, 4]) <= k_end)[0]                    # demodulate() calls that ended before the window
    assert len(log) >= done.size, f"{tag}: {len(log)} chunk rows"
    for c in done:
        assert np.array_equal(log[c, 3:], ech[c, 3:]), f"{tag}: call {c}: leftover / symbols {log[c, 3:]} vs {ech[c, 3:]}"
        assert np.allclose(log[c, :3], ech[c, :3], rtol=0, atol=1e-7), f"{tag}: call {c}: {log[c]} vs {ech[c]}"


def check_plan_streams_10m(amd, d, cap, tag):
    """every slot whose oracle output shows no one-tap window: check_stream in full, edge_ties == 0; the others: up to the first"""
    for k, exp in enumerate(cap["exp"]):
        got = collect(d, k)
        assert got["state"].stalled == 0
        if first_one_tap_window(exp)[1] == 0:
            check_stream(amd, got, exp, f"{tag} slot {k}", edge_ties=0, offset_ties=None)
        else:
            check_up_to_the_first_window(amd, got["state"], got["frames"], got["meta"], got["events"], got["chunks"], exp, f"{tag} slot {k}", got["soft"])
    assert d.state(PLAN_10M["empty"]).frames_released == 0
