"""CPU-only: the host half of the transmit bank (include/opv_demod.h, opv_txb_*; csrc/opv_txb_rules.cpp) - what a round
refuses and the geometry of its launches (opv_txb_plan_round), the tests' own model of the carried sign parity pinned to the
host modulator (tests/tx_bank_model.py; tests/test_gpu_tx_bank.py relies on it), the model's samples of a modulator that
stands anywhere in its run (tests/test_gpu_tx_bank_limits.py relies on them) pinned to the host modulator and to the patch tap,
and the host's evaluation of one entry of the device's list of ambiguous samples (opv_tap_txb_patch) against the host modulator's sample at that position."""
import ctypes as C
import re

import numpy as np
import pytest

import tx_bank_model as M
from fixtures_built import amd  # noqa: F401
from tx_bank_runs import drawn_frames, stream_frames

EINVAL, ECAPACITY = -1, -4
FRAME_BYTES_OUT = M.FRAME_SAMPLES * 4
MAX_RUN_FRAMES = 65536


def refusal(amd, *args):
    """the code opv_txb_plan_round refuses with (0: it does not)"""
    try:
        amd.txb_plan_round(*args)
    except amd.OpvError as e:
        return int(re.match(r"opv error (-?\d+):", str(e)).group(1))
    return 0


def test_plan_round_refuses_what_the_header_says(amd):
    fresh = [(0, 0)] * 4
    A = 1 << 20                                                     # a 16-byte aligned "device address"
    assert refusal(amd, fresh, [0, 1], [1, 2], [A, A + FRAME_BYTES_OUT]) == 0
    assert refusal(amd, fresh, [0, 4], [1, 1], [A, A + FRAME_BYTES_OUT]) == EINVAL          # stream out of range
    assert refusal(amd, fresh, [-1], [1], [A]) == EINVAL
    assert refusal(amd, fresh, [2, 2], [1, 1], [A, A + FRAME_BYTES_OUT]) == EINVAL          # named twice
    assert refusal(amd, fresh, [2, 2], [0, 0], [0, 0]) == EINVAL                            # ... even with nothing to do
    assert refusal(amd, fresh, [0], [1], [A + 8]) == EINVAL                                 # misaligned
    assert refusal(amd, fresh, [0], [1], [0]) == EINVAL                                     # null output
    assert refusal(amd, fresh, [0, 1], [2, 1], [A, A + FRAME_BYTES_OUT]) == EINVAL          # overlap: the second frame of entry 0
    assert refusal(amd, fresh, [0, 1], [1, 1], [A + FRAME_BYTES_OUT - 16, A]) == EINVAL     # overlap by one 16-byte store
    assert refusal(amd, fresh, [0, 1, 2], [1, 1, 1], [A + 2 * FRAME_BYTES_OUT, A, A + FRAME_BYTES_OUT]) == 0   # touching is not overlapping
    assert refusal(amd, fresh, [0, 1], [0, 1], [A + 8, A]) == 0                             # an entry of 0 frames: its output is not looked at
    assert refusal(amd, [(0, 2)], [0], [1], [A]) == EINVAL                                  # a state no modulator can be in
    assert refusal(amd, [(0, 0, 1)], [0], [1], [A]) == EINVAL
    assert refusal(amd, [(0, -1)], [0], [1], [A]) == EINVAL
    # the raw entry point: null pointers, count < 0
    L = amd.lib()
    st = (amd.TxbState * 2)()
    ids, nf, addr = (C.c_int * 1)(0), (C.c_size_t * 1)(1), (C.c_size_t * 1)(A)
    fb, fs = (C.c_uint32 * 2)(), (C.c_uint64 * 1)()
    assert L.opv_txb_plan_round(2, st, 1, ids, nf, addr, fb, fs) == 0
    for bad in range(7):
        args = [st, 1, ids, nf, addr, fb, fs]
        if bad == 1:
            args[1] = -1                                                                    # count < 0
        else:
            args[bad] = None
        assert L.opv_txb_plan_round(2, *args) == EINVAL, bad
        assert b"opv_txb_round" in L.opv_last_error()
    assert L.opv_txb_plan_round(0, st, 1, ids, nf, addr, fb, fs) == EINVAL
    assert L.opv_txb_plan_round(2, st, 0, None, None, None, fb, fs) == 0 and fb[0] == 0     # an empty round is a round


def test_plan_round_run_length_limit(amd):
    A = 1 << 20
    full = MAX_RUN_FRAMES * M.FSYMS
    assert amd.TXB_MAX_RUN_FRAMES == MAX_RUN_FRAMES >= 65536
    assert refusal(amd, [(full - M.FSYMS, 1)], [0], [1], [A]) == 0                          # the last frame of a run fits
    assert refusal(amd, [(full - M.FSYMS, 1)], [0], [2], [A]) == ECAPACITY
    assert refusal(amd, [(full - M.FSYMS + 1, 1)], [0], [1], [A]) == ECAPACITY              # (an odd position, one symbol too far)
    assert refusal(amd, [(full, 0)], [0], [1], [A]) == ECAPACITY
    assert refusal(amd, [(full, 0)], [0], [0], [A]) == 0                                    # standing still is always possible
    assert refusal(amd, [(0, 0)], [0], [MAX_RUN_FRAMES + 1], [A]) == ECAPACITY
    assert refusal(amd, [(full + 1, 0)], [0], [0], [A]) == EINVAL                           # not a state
    # what is wrong with the call is said before what is wrong with a run's length
    assert refusal(amd, [(full, 0), (0, 0)], [0, 1], [1, 1], [A, A + 8]) == EINVAL


def test_plan_round_geometry(amd):
    """first_block / first_symbol for frame counts 0, 1, 2 and 3 against a numpy restatement: 0, 34, 68 and 102 workgroups of 64
    symbols (a frame is 33 full ones + 56 symbols; an entry's last one is partial), entries back to back in the grid; the first
    symbol is the stream's position, odd positions (as opv_txb_set_state may leave them) included"""
    states = [(0, 0), (2168 * 7, 1), (12345, 0), (2168 * 1560 + 1, 1), (3, 1)]
    streams = [3, 0, 4, 1]
    n_frames = [0, 1, 2, 3]
    A = 1 << 20
    addr = [0, A, A + FRAME_BYTES_OUT, A + 3 * FRAME_BYTES_OUT]
    fb, fs = amd.txb_plan_round(states, streams, n_frames, addr)
    blocks = -(-(np.array(n_frames) * M.FSYMS) // 64)
    assert blocks.tolist() == [0, 34, 68, 102]
    assert fb.tolist() == np.concatenate([[0], np.cumsum(blocks)]).tolist() == [0, 0, 34, 102, 204]
    assert fs.tolist() == [states[s][0] for s in streams] == [2168 * 1560 + 1, 0, 3, 2168 * 7]
    # eight frames are 271 workgroups exactly (8 x 2168 = 271 x 64): not 8 x 34
    fb, _ = amd.txb_plan_round(states, [2, 1], [8, 1], [A, A + 8 * FRAME_BYTES_OUT])
    assert fb.tolist() == [0, 271, 305]


def decoded_sign(amd, iq, frame):
    """T of the host modulator in front of frame `frame` (>= 1) of a run, read off the first sample of the frame: its first
    symbol is the sync word's first bit, 0, so it goes out on tone 1 with sign T (reference src/opv-mod.cpp:241-245) and its
    sample 0 is (T sin ph1, T cos ph1) x 16383, truncated - and at a symbol start one of the two sits at a flat top"""
    sym = frame * M.FSYMS
    ph1 = M.symbol_phases(amd, sym, 1)[0, 0]
    i, q = int(iq[2 * sym * M.SPS]), int(iq[2 * sym * M.SPS + 1])
    assert max(abs(i), abs(q)) >= 16382, (i, q)                                             # non-silent
    return int(np.sign(i) * np.sign(np.sin(ph1))) if abs(i) > abs(q) else int(np.sign(q) * np.sign(np.cos(ph1)))


@pytest.mark.parametrize("callsign,token", [("W5NYV", 0xBBAADD), ("KB5MU", 0x123456), ("N0CALL", 0x00F00D), ("AI6YM-3", 0x7)])
def test_sign_parity_model_is_the_host_modulators(amd, callsign, token):
    """For 3 BERT frames - and for each prefix of them - the parity of the on-air bits (opv_tap_tx_frame's interleaved2144 + the
    sync word) is the sign the host modulator carries into the NEXT frame: T = -1 where the parity is odd. This is what
    opv_txb_state.sign_parity means, and what the GPU tests of the bank model it as."""
    frames = amd.bert_frames(4, callsign=callsign, token=token)
    tx = amd.TxStream()
    iq = np.concatenate([tx.frames(frames[:1]), tx.frames(frames[1:3]), tx.frames(frames[3:])])   # (carried from call to call)
    tx.close()
    assert np.array_equal(iq, amd.modulate(frames)[:iq.size])
    assert not iq[:2 * M.SPS].any()                                                          # symbol 0 of the run is silent
    for k in (1, 2, 3):
        par = M.sign_parity(amd, frames[:k])
        assert decoded_sign(amd, iq, k) == (-1 if par else 1), k
    # the model's tone / sign codes say the same about every symbol of the run: a silent symbol 0, and sample 0 of every other
    # symbol on the tone and with the sign the code names
    codes = M.symbol_codes(M.onair_bits(amd, frames))
    ph = M.symbol_phases(amd, 0, codes.size)
    first = iq.reshape(-1, M.SPS, 2)[:, 0, :].astype(np.int64)
    assert codes[0] == 0 and not first[0].any()
    p = np.where(np.abs(codes) == 1, ph[:, 0], ph[:, 1])
    want = np.sign(codes)[:, None] * np.stack([np.sin(p), np.cos(p)], axis=1) * 16383.0
    assert np.all(np.abs(first[1:] - want[1:]) <= 1.0 + 1e-6)                                # (truncation, flat tops: within one count)
    assert set(np.unique(codes[1:]).tolist()) == {-2, -1, 1, 2}


def test_samples_model_is_the_host_modulators(amd):
    """M.samples - the model's samples of a modulator that stands anywhere - against the host modulator: a run from symbol 0
    (silent symbol included), and frames 2..3 of a 4-frame run from the position and the sign parity the first two leave."""
    frames = amd.bert_frames(4, callsign="KB5MU", token=0x123456)
    host = amd.modulate(frames)[:2 * 4 * M.FRAME_SAMPLES]
    first = M.samples(amd, frames[:3])
    assert first.dtype == np.int16 and first.size == 2 * 3 * M.FRAME_SAMPLES
    assert np.array_equal(first, amd.modulate(frames[:3])[:2 * 3 * M.FRAME_SAMPLES])
    assert not first[:2 * M.SPS].any() and first[2 * M.SPS:4 * M.SPS].any()
    assert np.array_equal(M.samples(amd, frames[2:4], 2 * M.FSYMS, M.sign_parity(amd, frames[:2])), host[2 * 2 * M.FRAME_SAMPLES:])
    assert M.samples(amd, frames[:0], 5).size == 0
    # the parity matters: the other one is the same signal with the other sign
    flipped = M.samples(amd, frames[2:3], 2 * M.FSYMS, 1 - M.sign_parity(amd, frames[:2]))
    assert np.array_equal(flipped, -host[2 * 2 * M.FRAME_SAMPLES:2 * 3 * M.FRAME_SAMPLES])


def test_a_frames_parity_is_its_first_bytes(amd):
    """Why tests/test_gpu_tx_bank_limits.py draws its frames: a frame's on-air parity is a function of the low six bits of its
    first byte alone, in a BERT frame a byte of the callsign - every frame of one tx_bank_runs.stream_frames stream has the same
    parity. Drawn frames have both."""
    for k in (0, 7, 9, 10, 30):
        assert len(set(M.frame_parities(amd, stream_frames(amd, k, 6)).tolist())) == 1, k
    fr = drawn_frames(0, 256)
    par = M.frame_parities(amd, fr)
    assert 64 < par.sum() < 192
    other = fr.copy()
    other[:, 1:] = drawn_frames(1, 256)[:, 1:]
    other[:, 0] ^= 0xC0
    assert np.array_equal(M.frame_parities(amd, other), par)
    by_byte = {}
    for b, p in zip((fr[:, 0] & 63).tolist(), par.tolist()):
        by_byte.setdefault(b, set()).add(p)
    assert all(len(v) == 1 for v in by_byte.values()) and len(by_byte) > 50


# first symbol of a frame's worth of samples far into a run: inside the flat-top bit zone, either side of the end of the
# build-time checkpoint table (4096 frames), and an odd position that is no frame start (b_n and the phases follow the symbol)
FAR_STARTS = [1600 * M.FSYMS, 4095 * M.FSYMS, 4097 * M.FSYMS, 777 * M.FSYMS + 1001]


@pytest.mark.parametrize("first_symbol", FAR_STARTS)
def test_samples_model_far_positions_are_the_patch_taps(amd, first_symbol):
    """Far into a run the host modulator is no cheap yardstick (its cost grows with the position); opv_tap_txb_patch is, one
    sample at a time, and test_patch_tap_is_the_host_modulators_sample holds it to the host modulator. 200 drawn
    (symbol, sample) pairs of one frame at each position, all four tone / sign codes among them, both parities over the cases."""
    frame = amd.bert_frames(1, callsign="FAR", token=first_symbol & 0xFFFFFF)
    parity = (first_symbol // 7) & 1
    got = M.samples(amd, frame, first_symbol, parity).reshape(M.FSYMS, M.SPS, 2)
    codes = M.symbol_codes(M.onair_bits(amd, frame), first_symbol, parity)
    rng = np.random.default_rng(first_symbol)
    syms = np.concatenate([[0, M.FSYMS - 1], rng.integers(0, M.FSYMS, 198)])
    smps = np.concatenate([[0, M.SPS - 1], rng.integers(0, M.SPS, 198)])
    assert set(codes[syms].tolist()) == {-2, -1, 1, 2}
    for k, i in zip(syms.tolist(), smps.tolist()):
        assert np.array_equal(got[k, i], amd.txb_patch(first_symbol + k, i, int(codes[k]))), (k, i)
    assert {(s // 7) & 1 for s in FAR_STARTS} == {0, 1}


def test_patch_tap_is_the_host_modulators_sample(amd):
    """opv_tap_txb_patch - how a round's host patch evaluates one entry of the device's list of ambiguous samples (symbol of the
    run, sample in the symbol, tone / sign code; no frames) - against the host modulator's own sample at that position: both
    tones, both signs, the first and the last sample of a symbol and some between, symbols in front of and far behind a
    checkpoint, and a silent one."""
    frames = amd.bert_frames(5, callsign="PATCH", token=0x5EED)
    iq = amd.modulate(frames).reshape(-1, 2)
    codes = M.symbol_codes(M.onair_bits(amd, frames))
    rng = np.random.default_rng(17)
    for code in (1, -1, 2, -2):
        where = np.flatnonzero(codes == code)
        assert where.size > 100
        picks = np.concatenate([where[:2], where[-2:], rng.choice(where, 12, replace=False),
                                where[where % 128 == 0][:1], where[where % 128 == 127][:1]])
        for sym in picks:
            for sample in (0, 39, int(rng.integers(1, 39))):
                got = amd.txb_patch(int(sym), sample, code)
                assert np.array_equal(got, iq[sym * M.SPS + sample]), (code, int(sym), sample)
    assert np.array_equal(amd.txb_patch(0, 7, 0), [0, 0]) and not iq[7].any()
    for bad in ((0, 40, 1), (0, -1, 1), (0, 0, 3), (MAX_RUN_FRAMES * M.FSYMS, 0, 1)):
        with pytest.raises(amd.OpvError):
            amd.txb_patch(*bad)
