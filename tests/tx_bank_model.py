"""The tests' own model of a transmit-bank modulator (tests/test_tx_bank_host.py pins it to the host modulator, the GPU tests
rely on it): the on-air bits of a frame, the sign parity they carry, the tone / sign code of every symbol, the NCO phases at a
symbol start, and from these the samples of a modulator that stands anywhere in its run (libm, plain Python floats). Numpy over the library's parity taps (opv_tap_tx_frame, opv_tap_tx_checkpoints); nothing here needs a GPU."""
import math

import numpy as np

FSYMS = 2168
SPS = 40
FRAME_SAMPLES = FSYMS * SPS          # 86720
SYNC_WORD = 0x02B8DB                 # reference src/opv-mod.cpp:45 (24 bits, MSB first)
CKPT_SYMS = 128
PI = math.pi
INC1 = 2.0 * PI * (-13550.0) / 2168000.0
INC2 = 2.0 * PI * (+13550.0) / 2168000.0


def onair_bits(amd, frames):
    """[F][2168] bits as they go on the air: 24 sync bits, then the interleaved coded bits"""
    frames = np.ascontiguousarray(frames, np.uint8).reshape(-1, 134)
    sync = np.array([(SYNC_WORD >> (23 - b)) & 1 for b in range(24)], np.uint8)
    return np.stack([np.concatenate([sync, amd.tx_frame_taps(f)[2]]) for f in frames]) if len(frames) else np.zeros((0, FSYMS), np.uint8)


def frame_parities(amd, frames):
    """parity of each frame's 2168 on-air bits"""
    return (onair_bits(amd, frames).sum(axis=1) & 1).astype(np.int64)


def sign_parity(amd, frames, start=0):
    """sign_parity of a modulator that stood at parity `start` and has sent `frames` since"""
    return int((start + frame_parities(amd, frames).sum()) & 1)


def symbol_codes(bits, first_symbol=0, parity=0):
    """tone / sign code of every symbol (+-1 tone 1, +-2 tone 2, 0 silent) of the on-air bits `bits` (flattened), sent by a
    modulator that stands at symbol first_symbol with sign parity `parity` (reference src/opv-mod.cpp:228-257)"""
    bits = np.asarray(bits, np.int64).reshape(-1)
    before = (parity + np.concatenate([[0], np.cumsum(bits)[:-1]])) & 1       # parity of the run's bits in front of each symbol
    T = np.where(before == 1, -1, 1)
    sym = first_symbol + np.arange(bits.size)
    code = np.where(bits == 0, T, 2 * np.where(sym & 1, -T, T))
    code[sym == 0] = 0                                                          # symbol 0 of a run: T = 0 right after reset
    return code


def _wrap(p):
    p = np.where(p > PI, p - 2.0 * PI, p)
    return np.where(p < -PI, p + 2.0 * PI, p)


def symbol_phases(amd, first_symbol, n_symbols):
    """[n][2] (ph1, ph2) at the start of symbols first_symbol .. + n - 1 of a run: the checkpoint sequence every 128 symbols,
    replayed with the reference's adds and wraps (src/opv-mod.cpp:274-279), all intervals side by side"""
    j0, j1 = first_symbol // CKPT_SYMS, (first_symbol + n_symbols - 1) // CKPT_SYMS
    p = amd.tx_checkpoints(j0, j1 - j0 + 1).copy()
    out = np.empty((j1 - j0 + 1, CKPT_SYMS, 2))
    for s in range(CKPT_SYMS):
        out[:, s, :] = p
        for _ in range(SPS):
            p[:, 0] = _wrap(p[:, 0] + INC1)
            p[:, 1] = _wrap(p[:, 1] + INC2)
    flat = out.reshape(-1, 2)
    a = first_symbol - j0 * CKPT_SYMS
    return flat[a:a + n_symbols]


def sample_phases(p, inc):
    """the 40 phases of one symbol's samples from its start phase `p`: the reference's add and wrap (src/opv-mod.cpp:274-279)
    in plain Python floats"""
    out = []
    for _ in range(SPS):
        out.append(p)
        p += inc
        if p > PI:
            p -= 2.0 * PI
        elif p < -PI:
            p += 2.0 * PI
    return out


def samples(amd, frames, first_symbol=0, parity=0):
    """int16[2 * 40 * n_symbols]: what a modulator that stands at symbol `first_symbol` of its run with sign parity `parity`
    makes of the whole frames `frames` - wherever it stands: first_symbol need not be a multiple of 2168, the symbol's index
    only drives b_n and the phases. Each sample is int(16383.0 * (sgn * math.sin(ph))) / math.cos: THIS process's libm and
    truncation toward zero (reference src/opv-mod.cpp:268-279), not numpy's vector paths; silent symbol 0 gives zeros."""
    codes = symbol_codes(onair_bits(amd, frames), first_symbol, parity)
    ph = symbol_phases(amd, first_symbol, codes.size) if codes.size else np.zeros((0, 2))
    flat = []
    for a, (p1, p2) in zip(codes.tolist(), ph.tolist()):
        if a == 0:
            flat += [0] * (2 * SPS)
            continue
        sgn = 1.0 if a > 0 else -1.0
        for p in sample_phases(p1, INC1) if abs(a) == 1 else sample_phases(p2, INC2):
            flat.append(int(16383.0 * (sgn * math.sin(p))))
            flat.append(int(16383.0 * (sgn * math.cos(p))))
    return np.array(flat, np.int16)


def flat_bits(ph):
    """per symbol start and tone: does THIS process's libm answer exactly 1.0 at the flat top (k_tx_modulate.hip)"""
    return np.array([[abs(math.sin(v)) == 1.0 or abs(math.cos(v)) == 1.0 for v in row] for row in ph])
