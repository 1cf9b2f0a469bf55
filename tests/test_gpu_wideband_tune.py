"""GPU: the LO schedule of the four wideband converters (opv_wb_retune / opv_wbtx_retune, include/opv_demod.h "per-channel retune and
Doppler ramps"; the scheduled kernels k_wb_ddc_tuned, k_wbr_ddc_tuned, k_wbtx_duc_tuned, k_wbtxr_duc_tuned). The kernels are
integer-exact, so every sample is held with == to the models of tests/wideband_tune_model.py, which take a sample's phase from the
header's formula on its absolute index and know nothing of pushes, tiles or the device's re-basing.

The plans are the suite's: D = 4 / L = 321 at 8.672 MS/s and 1250 / 271 at 10 MS/s with J = 96 on the receive side
(wideband_device.PLAN_D4, PLAN_10M), U = 4 / L = 321 and 1250 / 271 on the transmit side. The rational up-converter takes at
most 64 taps per phase (opv_wbtxr_plan), so its filter is the loopback plan's J = 60 (wideband_device.loop_taps_10m), not J = 96.

The end-to-end case moves a transmitter: channel 0 of the D = 4 loopback leaves its up-converter on a ramp of E2E_RATE =
+500 000 Hz/s from its first sample, which turns to -500 000 Hz/s at wide sample 150 000 (17 ms in): 8.6 kHz off after 17 ms,
far outside the +/-2000 Hz the reference's AFC follows. The rate was chosen on the CPU, and the fixture asserts what it was chosen
for before the device sees a sample: the oracle alone on the model of a door that does NOT follow loses a frame of channel 0 (it
releases two frames, the second with other bytes than were sent; the reference's non-coherent detector rides out the first 8 kHz),
the oracle alone on the model of a door that carries the same schedule decodes every frame of every channel and shows no one-tap
window inside the frames (its first, as on the plain loopback, lies in the modulator's tail of zeros)."""
import numpy as np
import pytest

from fixtures import amd, torch_dev  # noqa: F401
from stream_checks import check_stream
from stream_runs import CHUNK, code_raised_by, collect
from wideband_device import (LOOP_D4, PLAN_10M, PLAN_D4, Inputs, Out, assert_equal, check_up_to_the_first_window, first_one_tap_window,
                             loop_taps_10m, loop_taps_d4, loopback_on_the_cpu, plan_taps_10m, plan_taps_d4)
from wideband_models import WIDE_RATE, wb_model, wb_model_inc, wbr_model_inc, wbr_outputs, wbtxr_outputs
from wideband_tune_model import (TUNE_GAP, TUNE_SEGS, creation, schedule, seg_phase, wb_tuned_model, wbr_tuned_model, wbtx_tuned_model,
                                 wbtxr_tuned_model)

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY, ESTATE = -1, -4, -6
K = 5
FIRSTS = {"across_2_32": (1 << 32) - 3000, "beyond_2_40": (1 << 40) + 12345}
E2E_RATE = 5.0e5


# ------------------------------------------------------------------ the four kinds, each with its plan, inputs, model and run
class Kind:
    """one of the four converters on its plan. n_in: samples fed per input (the wide capture, or each channel); wide(n): the wide
    sample at which input n stands (receive: n itself); carry: wide samples mixed again by the next push (transmit: none)"""

    def __init__(self, name):
        self.name, self.rx, self.rational = name, name.startswith("rx"), name.endswith("rat")
        self.down, self.up = (PLAN_10M["down"], PLAN_10M["up"]) if self.rational else (4, 1)
        if self.rx:
            self.taps, self.S = (plan_taps_10m(), PLAN_10M["out_shift"]) if self.rational else (plan_taps_d4(), PLAN_D4["out_shift"])
            self.carry = (PLAN_10M["J"] if self.rational else PLAN_D4["L"]) - 1
            self.n_in = 20000
        else:
            self.taps, self.S = (loop_taps_10m(), 32) if self.rational else (loop_taps_d4(), 32)
            self.carry = 0
            self.n_in = 4336 if self.rational else 5000                    # about 20 000 wide samples written
        self.fw = self.down * WIDE_RATE / self.up
        rng = np.random.default_rng(sum(map(ord, name)))
        self.centres = list(rng.uniform(-0.45 * self.fw, 0.45 * self.fw, K))
        self.centres[3] = -abs(self.centres[3])                            # channel 3 is retuned to a negative centre
        if self.rx:
            self.inputs = rng.integers(-32768, 32768, 2 * self.n_in).astype(np.int16)
        else:
            self.inputs = [rng.integers(-6000, 6001, 2 * self.n_in).astype(np.int16) for _ in range(K)]
        self.inc = wbr_model_inc(self.down, self.up, self.centres)

    def wide(self, n):
        return n if self.rx else (wbtxr_outputs(self.down, self.up, n) if self.rational else n * self.down)

    def tile_edge(self, cut):
        """a wide sample on the edge between the first two workgroups of a push that starts at input `cut`"""
        if not self.rx:
            return self.wide(cut) + 256                                    # a workgroup writes 256 wide samples
        if not self.rational:
            return (-(-cut // 4) + 256) * 4                                # 256 outputs per workgroup: the newest sample of tile 1's first output
        return (wbr_outputs(self.down, self.up, cut) + 256) * self.down // self.up

    def make(self, amd, d, first):
        if self.rx:
            if self.rational:
                return amd.Wideband.rational(d, self.down, self.up, list(range(K)), self.centres, self.taps, self.S, first)
            return amd.Wideband(d, self.down, list(range(K)), self.centres, self.taps, self.S, first)
        if self.rational:
            return amd.WidebandTx.rational(d, self.down, self.up, self.centres, self.taps, self.S, first)
        return amd.WidebandTx(d, self.down, self.centres, self.taps, self.S, first)

    def model(self, amd, segs, first):
        """the bytes of the whole run behind the schedules segs[k]: [K][...] on the receive side, one capture on the transmit side"""
        T = amd.wb_lo_table()
        if self.rx:
            if self.rational:
                return wbr_tuned_model(T, self.inputs, self.down, self.up, segs, self.taps, self.S, first)
            return wb_tuned_model(T, self.inputs, self.down, segs, self.taps, self.S, first)
        if self.rational:
            return wbtxr_tuned_model(T, self.inputs, self.down, self.up, segs, self.taps, self.S, first)
        return wbtx_tuned_model(T, self.inputs, self.down, segs, self.taps, self.S, first)

    def run(self, amd, torch_dev, first, cuts, retunes, asynchronous=False, after=None):
        """pushes inputs [cuts[i], cuts[i + 1]) in turn; before push i the batches retunes.get(i, []) are issued, each a list of
        (channel, at, centre_hz, rate_hz_s). -> the bytes as model() lays them out. asynchronous (receive): every push is
        opv_wb_push_async and nothing waits before the last one is enqueued. after(obj): called before the object is closed."""
        n_wide = self.wide(self.n_in)
        d = amd.Demod(K, max_samples=n_wide + 64, streaming=True)
        obj = self.make(amd, d, first)
        try:
            if self.rx:
                pinned = torch_dev[0].from_numpy(self.inputs.copy()).pin_memory()
                block = pinned.numpy()
            else:
                src, out = Inputs(torch_dev, self.inputs), Out(torch_dev, n_wide)
            for i, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
                for batch in retunes.get(i, []):
                    obj.retune(batch)
                if self.rx:
                    (obj.push_async if asynchronous else obj.push)(block[2 * lo: 2 * hi])
                else:
                    obj.push([src.ptr(k, lo) for k in range(K)], hi - lo, out.ptr(self.wide(lo)))
            if self.rx and asynchronous:
                d.push_wait()
            got = np.stack([d.iq(k) for k in range(K)]) if self.rx else out.get()
            if after:
                after(obj)
            return got
        finally:
            obj.close()
            d.close()

    def assert_equal(self, got, exp, tag):
        if self.rx:
            assert got.shape == exp.shape, (tag, got.shape, exp.shape)
            for k in range(K):
                assert_equal(got[k], exp[k], f"{tag} channel {k}")
        else:
            assert_equal(got, exp, tag)


KINDS = {name: None for name in ("rx_int", "rx_rat", "tx_int", "tx_rat")}


@pytest.fixture(scope="module")
def kinds():
    return {name: Kind(name) for name in KINDS}


def the_case(kd, first):
    """-> (cuts, tunes[k] = [(at, centre, rate)], when[k] = the push before which channel k's tunes are issued). Wide samples below are
    counted from the run's first one; `first` is added at the end.
      channel 0  never retuned
      channel 1  one ramp, from the LAST sample of push 0: on the receive side that is A - 1 of push 1, inside the history it mixes again
      channel 2  three segments exactly OPV_WB_TUNE_GAP apart, the first at A - carry of push 2: the oldest sample that push still mixes
                 (transmit: 100 samples in front of push 2's first); the other two fall inside tiles
      channel 3  retuned at the FIRST sample of push 1, once push 0 has gone, to a negative centre on a negative ramp
      channel 4  a segment on the edge between the first two workgroups of push 1, and one that starts beyond the end of the run"""
    n = kd.n_in
    cuts = [0, 2999, 9000, 14001, n] if kd.rx else [0, 650 if kd.rational else 749, n * 9 // 20, n * 7 // 10 + 1, n]   # (push 1 starts just below wide sample 3000)
    w = [kd.wide(c) for c in cuts]
    f = kd.centres
    tunes = {
        1: [(w[1] - 1, f[1] + 31000.0, 8.0e6)],
        2: [(w[2] - (kd.carry or 100), f[2] - 9000.0, -3.0e6), (w[2] - (kd.carry or 100) + TUNE_GAP, f[2], 0.0),
            (w[2] - (kd.carry or 100) + 2 * TUNE_GAP, -f[2], 1.0e7)],
        3: [(w[1], f[3] - 55000.0, -9.5e6)],
        4: [(kd.tile_edge(cuts[1]), f[4] + 2.0e5, 2.5e6), (w[4] + 5000, 0.0, 0.0)],
    }
    assert f[3] - 55000.0 < 0 and tunes[2][2][0] < w[4] and w[1] < tunes[4][0][0] < w[2]
    if first + w[0] < (1 << 32):
        assert first + w[1] - 1 < (1 << 32) <= first + w[2]                 # a crosses 2^32 inside the run, beside two boundaries
    tunes = {k: [(first + at, c, r) for at, c, r in v] for k, v in tunes.items()}
    return cuts, tunes, {1: 0, 2: 0, 3: 1, 4: 0}


def schedules_of(kd, tunes):
    return [schedule(kd.inc[k], kd.down, kd.up, tunes.get(k, [])) for k in range(K)]


def batches(tunes, when):
    """-> {push: [one batch of every channel issued before it]}"""
    out = {}
    for k, v in tunes.items():
        out.setdefault(when[k], [[]])[0].extend((k, at, c, r) for at, c, r in v)
    return out


@pytest.fixture(scope="module")
def expected(amd, kinds):
    """the model's bytes of the_case, computed once per (kind, first) and shared by the tests below; never written to"""
    cache = {}

    def get(name, first):
        if (name, first) not in cache:
            kd = kinds[name]
            exp = kd.model(amd, schedules_of(kd, the_case(kd, first)[1]), first)
            plain = kd.model(amd, creation(kd.inc), first)
            assert (np.abs(exp.astype(np.int32)) < 32767).mean() > 0.9, "the case must not hide behind the clamp"
            for k in range(K if kd.rx else 0):                              # the schedule is visible in every retuned channel
                assert np.array_equal(exp[k], plain[k]) == (k == 0), k
            exp.setflags(write=False)
            plain.setflags(write=False)
            cache[name, first] = exp, plain
        return cache[name, first]
    return get


# ------------------------------------------------------------------ 1. every sample == the model
@pytest.mark.parametrize("first", list(FIRSTS))
@pytest.mark.parametrize("name", list(KINDS))
def test_every_sample_equals_the_scheduled_model(amd, torch_dev, kinds, expected, name, first):
    """the_case in four pushes: boundaries on the last and on the first sample of a push, at A - 1 and A - carry of the following
    push, inside a tile and on a tile's edge, a segment beyond the end; a crosses 2^32 inside the run, or lies beyond 2^40"""
    kd, first = kinds[name], FIRSTS[first]
    cuts, tunes, when = the_case(kd, first)
    exp, _ = expected(name, first)

    def after(obj):
        segs = schedules_of(kd, tunes)
        assert [s.astuple() for s in obj.segments(0)] == segs[0]           # never retuned: its creation segment
        assert [s.astuple() for s in obj.segments(4)] == segs[4][-2:]      # what the run has passed is dropped, what lies ahead is kept
        assert [s.astuple() for s in obj.segments(1)] == segs[1][-1:]
    kd.assert_equal(kd.run(amd, torch_dev, first, cuts, batches(tunes, when), after=after), exp, name)


# ------------------------------------------------------------------ 2. a retune to where the channel is changes no byte
@pytest.mark.parametrize("name", list(KINDS))
def test_retune_to_the_own_centre_equals_never_retuned(amd, torch_dev, kinds, expected, name):
    """every channel retuned to its own centre, rate 0, continuous phase, at different samples: the scheduled kernel beside the
    unscheduled one gives the bytes of an object that was never retuned (== the model of the creation schedules)"""
    kd, first = kinds[name], FIRSTS["across_2_32"]
    _, plain = expected(name, first)
    n = kd.n_in
    cuts = [0, n // 3 + 1, n]
    w = kd.wide(cuts[1])
    own = [[(k, first + w + 700 * k, kd.centres[k], 0.0) for k in range(K)]]

    def after(obj):
        for k in range(K):
            (seg,) = obj.segments(k)
            assert seg.start == first + w + 700 * k and seg.phase == seg_phase((0, 0, int(kd.inc[k]) << 32, 0), seg.start) and seg.ramp == 0
    kd.assert_equal(kd.run(amd, torch_dev, first, cuts, {}), plain, name + " never retuned")
    kd.assert_equal(kd.run(amd, torch_dev, first, cuts, {1: own}, after=after), plain, name + " retuned to its own centres")


# ------------------------------------------------------------------ 3. any split
@pytest.mark.parametrize("name", list(KINDS))
def test_any_split_and_any_time_of_retune_gives_the_same_bytes(amd, torch_dev, kinds, expected, name):
    """the_case in ONE push with every retune made up front, and in many pushes with each channel's retunes made at the last moment
    that is still before their `at`; on the receive side a third run is all opv_wb_push_async, the retunes falling between two
    asynchronous pushes with no opv_push_wait. The same bytes, == the model."""
    kd, first = kinds[name], FIRSTS["beyond_2_40"]
    _, tunes, _ = the_case(kd, first)
    exp, _ = expected(name, first)
    n = kd.n_in
    one = {0: [[(k, at, c, r) for k, v in tunes.items() for at, c, r in v if k != 3] + [(3,) + tunes[3][0]]]}
    kd.assert_equal(kd.run(amd, torch_dev, first, [0, n], one), exp, name + " one push")
    cuts = sorted(set([0, n] + list(range(1, n, 1777)) + list(range(n // 2, n, 613))))
    late = {}
    for k, v in tunes.items():
        for at, c, r in v:                                                  # before the last push that starts at or before `at`
            i = max(j for j, lo in enumerate(cuts[:-1]) if first + kd.wide(lo) <= at)
            late.setdefault(i, []).append([(k, at, c, r)])
    kd.assert_equal(kd.run(amd, torch_dev, first, cuts, late), exp, name + " many pushes")
    if kd.rx:
        kd.assert_equal(kd.run(amd, torch_dev, first, cuts, late, asynchronous=True), exp, name + " asynchronous pushes")


# ------------------------------------------------------------------ 4. refusals change nothing
@pytest.mark.parametrize("name", list(KINDS))
def test_refused_retunes_change_nothing(amd, torch_dev, kinds, expected, name):
    """every refusal code, a batch with one bad entry, a 17th segment, a detached object: the lists stay what they were and the
    pushes give the bytes of an object that was never asked; opv_wbtx_reset restores the creation schedule"""
    kd, first = kinds[name], FIRSTS["across_2_32"]
    _, plain = expected(name, first)
    n = kd.n_in
    cuts = [0, n // 4 + 1, n]
    d = amd.Demod(K, max_samples=kd.wide(n) + 64, streaming=True)
    obj = kd.make(amd, d, first)
    try:
        if kd.rx:
            push = lambda lo, hi: obj.push(kd.inputs[2 * lo: 2 * hi])      # noqa: E731
        else:
            src, out = Inputs(torch_dev, kd.inputs), Out(torch_dev, kd.wide(n))
            push = lambda lo, hi: obj.push([src.ptr(k, lo) for k in range(K)], hi - lo, out.ptr(kd.wide(lo)))   # noqa: E731
        created = [[s.astuple() for s in obj.segments(k)] for k in range(K)]
        assert created == creation(kd.inc)
        push(cuts[0], cuts[1])
        A = first + kd.wide(cuts[1])
        good = (1, A + 50, 1.0e5, 1.0e5)

        def refused(batch, code):
            assert code_raised_by(amd, lambda: obj.retune(batch)) == code, batch
            assert [[s.astuple() for s in obj.segments(k)] for k in range(K)] == created
        refused([good, (0, A - 1, 0.0, 0.0)], ESTATE)                       # the past
        refused([good, (K, A + 50, 0.0, 0.0)], EINVAL)
        refused([good, (-1, A + 50, 0.0, 0.0)], EINVAL)
        refused([good, (0, A + 50, np.nan, 0.0)], EINVAL)
        refused([good, (0, A + 50, 0.0, np.inf)], EINVAL)
        refused([good, (0, A + 50, 0.0, 1.0000001e7)], EINVAL)
        refused([good, (1, A + 50 + TUNE_GAP - 1, 0.0, 0.0)], EINVAL)       # two entries of a channel inside the gap
        refused([(1, A + 50 + (i + 1) * TUNE_GAP, 0.0, 0.0) for i in range(TUNE_SEGS)], ECAPACITY)    # the creation segment and sixteen more
        assert code_raised_by(amd, lambda: amd._chk(amd.lib().opv_wb_retune(obj.h, 1, None) if kd.rx else amd.lib().opv_wbtx_retune(obj.h, 1, None))) == EINVAL
        assert code_raised_by(amd, lambda: amd._chk(amd.lib().opv_wb_retune(obj.h, -1, None) if kd.rx else amd.lib().opv_wbtx_retune(obj.h, -1, None))) == EINVAL
        assert code_raised_by(amd, lambda: obj.segments(K)) == EINVAL and code_raised_by(amd, lambda: obj.segments(-1)) == EINVAL
        obj.retune([])                                                      # nothing asked, nothing changed
        push(cuts[1], cuts[2])
        got = np.stack([d.iq(k) for k in range(K)]) if kd.rx else out.get()
        kd.assert_equal(got, plain, name + " after the refusals")
        # fifteen more fit behind the creation segment, a gap apart from each other; a sixteenth does not
        A = first + kd.wide(n)
        obj.retune([(2, A + 10 + i * TUNE_GAP, 1.0e5 * i, -1.0e5 * i) for i in range(TUNE_SEGS - 1)])
        full = [s.astuple() for s in obj.segments(2)]
        assert len(full) == TUNE_SEGS and full == schedule(kd.inc[2], kd.down, kd.up, [(A + 10 + i * TUNE_GAP, 1.0e5 * i, -1.0e5 * i) for i in range(TUNE_SEGS - 1)])
        assert code_raised_by(amd, lambda: obj.retune([(2, A + TUNE_SEGS * TUNE_GAP, 0.0, 0.0)])) == ECAPACITY
        assert code_raised_by(amd, lambda: obj.retune([(2, A + 14 * TUNE_GAP + 4095, 0.0, 0.0)])) == EINVAL    # inside the gap of the last one
        assert [s.astuple() for s in obj.segments(2)] == full
        if not kd.rx:
            obj.reset(first)
            assert [[s.astuple() for s in obj.segments(k)] for k in range(K)] == created
            out2 = Out(torch_dev, kd.wide(n))
            obj.push([src.ptr(k, 0) for k in range(K)], n, out2.ptr())
            kd.assert_equal(out2.get(), plain, name + " after the reset")
        # a given phase is taken as it is
        A = first + kd.wide(obj.samples() if not kd.rx else n) + (TUNE_SEGS + 1) * TUNE_GAP
        obj.retune([(0, A, 1.0e5, 0.0, 0xDEADBEEF12345678)])
        assert obj.segments(0)[-1].astuple() == (A, 0xDEADBEEF12345678, int(wbr_model_inc(kd.down, kd.up, [1.0e5])[0]) << 32, 0)
        d.close()                                                           # the object outlives its context: detached
        assert code_raised_by(amd, lambda: obj.retune([(3, A, 0.0, 0.0)])) == ESTATE
    finally:
        obj.close()
        d.close()


# ------------------------------------------------------------------ 5. end to end: a moving transmitter, followed
def e2e_tunes(first=0):
    """channel 0 of the loopback: from the first sample its centre moves up by E2E_RATE, from wide sample 150 000 down again"""
    f0, fw = LOOP_D4["centres"][0], LOOP_D4["U"] * WIDE_RATE
    return [(first, f0, E2E_RATE), (first + 150000, f0 + E2E_RATE * 150000 / fw, -E2E_RATE)]


@pytest.fixture(scope="module")
def moving(amd, oracle):
    """the chain on the CPU from the scheduled models and the oracle alone, and the two preconditions the rate was chosen for"""
    U, D = LOOP_D4["U"], PLAN_D4["D"]
    up_segs = [schedule(w, U, 1, e2e_tunes() if k == 0 else []) for k, w in enumerate(wb_model_inc(U, LOOP_D4["centres"]))]
    inc_d = wb_model_inc(D, PLAN_D4["centres"])
    down_segs = [schedule(w, D, 1, e2e_tunes() if k == 0 else []) for k, w in enumerate(inc_d)]
    assert up_segs[0] == down_segs[0]                                       # the door carries the transmitter's schedule
    loop = loopback_on_the_cpu(
        amd, oracle, LOOP_D4,
        lambda T, chans: wbtx_tuned_model(T, chans, U, up_segs, loop_taps_d4(), LOOP_D4["out_shift"]),
        lambda T, wide: wb_tuned_model(T, wide, D, down_segs, plan_taps_d4(), PLAN_D4["out_shift"]))
    # (loopback_on_the_cpu asserted every frame of slots 0 - 2 and none on 3.) No one-tap window inside the frames: as on the plain
    # loopback, the first one a slot shows lies in the modulator's tail of zeros, behind the symbols of both frames
    assert first_one_tap_window(loop["exp"][3])[1] >= 1                     # the empty slot's class (the test's docstring)
    for k in range(3):
        assert first_one_tap_window(loop["exp"][k])[0] >= LOOP_D4["frames"] * 2168, f"the corrected door's slot {k} shows a one-tap window inside its frames"
    blind = wb_model(amd.wb_lo_table(), loop["wide"], D, inc_d, plan_taps_d4(), PLAN_D4["out_shift"])
    seen = oracle.receive(blind[0], streaming=True)["frames"]
    kept = sum(any(np.array_equal(f, g) for g in seen) for f in loop["tx"][0])
    assert kept < len(loop["tx"][0]), "a door that does not follow must lose frames of channel 0: the rate is too small"
    for k in (1, 2):
        assert np.array_equal(blind[k], loop["model"][k])                   # the channels that do not move are served as before
    return loop


def test_a_moving_transmitter_is_followed_end_to_end(amd, torch_dev, moving):
    """TxBank -> WidebandTx (channel 0 on e2e_tunes) -> Wideband (the same schedule on channel 0) -> Demod, the retunes made as the
    first round goes out. The wide capture == the model, every stream's IQ == the model, frames == the transmitted ones, and every
    stream is held to the oracle by the suite's rule for its class (wideband_device.check_plan_streams_10m: which check a slot gets
    is read off the oracle's output alone): slots 0 - 2 check_stream in full with edge_ties == 0, as check_plan_streams_d4 does. The
    empty slot is digitally silent behind a real up-converter and a transmitter that moves - the oracle alone shows dozens of one-tap
    windows on it from its 7th symbol on, for every rate tried, where the plain loopback shows three - and there the reference's
    tone choice is the rounding of its own LO, which the product reports in edge_ties and does not reproduce: it is held up to the
    first such window, releases no frame, and edge_ties stays within the oracle's count."""
    torch, dev = torch_dev
    F, U, tail = LOOP_D4["frames"], LOOP_D4["U"], LOOP_D4["tail"]
    n_wide = (F * CHUNK + tail) * U
    d = amd.Demod(4, max_samples=n_wide // PLAN_D4["D"] + 64, streaming=True)
    bank = amd.TxBank(d, 3)
    up = amd.WidebandTx(d, U, LOOP_D4["centres"], loop_taps_d4(), LOOP_D4["out_shift"])
    wb = amd.Wideband(d, PLAN_D4["D"], [0, 1, 2, 3], PLAN_D4["centres"], plan_taps_d4(), PLAN_D4["out_shift"])
    try:
        lanes = torch.zeros((3, 2 * CHUNK), dtype=torch.int16, device=dev)
        out = Out(torch_dev, n_wide)
        ptrs = [lanes[k].data_ptr() for k in range(3)]
        t0, t1 = e2e_tunes()
        assert t1[0] < CHUNK * U                                            # the turn lies inside the first round: both are made before it
        for obj in (up, wb):
            obj.retune([(0,) + t0])
            obj.retune([(0,) + t1])
        for r in range(F):
            assert bank.round([0, 1, 2], [moving["tx"][k][r: r + 1] for k in range(3)], ptrs) >= 0
            up.push(ptrs, CHUNK, out.ptr(r * CHUNK * U))
            wb.push_device(out.ptr(r * CHUNK * U), CHUNK * U)
        up.push([None] * 3, tail, out.ptr(F * CHUNK * U))
        wb.push_device(out.ptr(F * CHUNK * U), tail * U)
        assert_equal(out.get(), moving["wide"], "wide capture")
        for k in range(4):
            assert_equal(d.iq(k), moving["model"][k], f"slot {k} IQ")
        wb.flush()
        d.process()
        d.sync()
        for k, exp in enumerate(moving["exp"]):
            got = collect(d, k)
            assert got["state"].stalled == 0
            if k < 3:                                                       # check_plan_streams_d4's check of a slot
                check_stream(amd, got, exp, f"moving transmitter slot {k}", edge_ties=0, offset_ties=None)
                assert np.array_equal(got["frames"], moving["tx"][k]), k
            else:                                                           # check_plan_streams_10m's check of a slot with one-tap windows
                check_up_to_the_first_window(amd, got["state"], got["frames"], got["meta"], got["events"], got["chunks"], exp,
                                             "moving transmitter, the empty slot", got["soft"])
                assert len(got["frames"]) == 0 and d.state(k).frames_released == 0
    finally:
        wb.close()
        up.close()
        bank.close()
        d.close()
