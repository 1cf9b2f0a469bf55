"""The LO schedule of the four wideband converters (include/opv_demod.h, "per-channel retune and Doppler ramps") restated in Python
integers, and the four converters' models behind it. numpy and Python integers only: importable with no device and no build.

A segment is a tuple (start, phase, inc, ramp); a schedule is a list of them with ascending start; `segs` is one schedule per
channel. The phase of every sample is taken from the header's formula as it stands, on the ABSOLUTE index with d = a - start in
full (Python integers, or uint64 held to them): nothing here is re-based to a push, a tile or 32 bits, which is what the device does. The filters
are those of tests/wideband_models.py, stated again around an LO index per sample instead of an increment."""
import numpy as np

from wideband_models import WIDE_RATE, wbr_outputs, wbtxr_outputs

M64 = (1 << 64) - 1
TUNE_GAP, TUNE_SEGS, TUNE_MAX_RATE = 4096, 16, 1.0e7


# ------------------------------------------------------------------ the rule
def tri(d):
    """d (d - 1) / 2 as an integer, modulo 2^64"""
    return (d * (d - 1) // 2) & M64


def seg_phase(seg, a):
    start, phase, inc, ramp = (int(v) for v in seg)
    d = (int(a) - start) & M64
    return (phase + d * inc + ramp * tri(d)) & M64


def model_inc32(down, up, centre_hz):
    fw = np.float64(down) * WIDE_RATE / np.float64(up)
    return int(np.rint(np.float64(centre_hz) / fw * 4294967296.0)) % (1 << 32)


def model_ramp(down, up, rate_hz_s):
    fw = np.float64(down) * WIDE_RATE / np.float64(up)
    return int(np.rint(np.float64(rate_hz_s) / fw / fw * 18446744073709551616.0))


def seg_next(prev, down, up, at, centre_hz, rate_hz_s=0.0, phase=None):
    """the segment behind `prev` from `at` on; `phase`: given, not continued"""
    return (int(at), seg_phase(prev, at) if phase is None else int(phase) & M64, model_inc32(down, up, centre_hz) << 32,
            model_ramp(down, up, rate_hz_s))


def creation(inc):
    """the creation schedules of a plan's increments"""
    return [[(0, 0, int(w) << 32, 0)] for w in inc]


def schedule(inc32, down, up, tunes):
    """one channel's schedule: its creation segment and then `tunes` = [(at, centre_hz, rate_hz_s[, phase])] in turn (nothing pruned)"""
    segs = [(0, 0, int(inc32) << 32, 0)]
    for t in tunes:
        segs.append(seg_next(segs[-1], down, up, *t))
    return segs


def lo_index(segs, a0, n, exact=False):
    """the LO index phi64 >> 52 of absolute samples a0 .. a0 + n - 1 (int64 array): sample a uses the last segment with start <= a"""
    a0, n = int(a0), int(n)
    out = np.zeros(n, np.int64)
    starts = [int(s[0]) for s in segs]
    assert starts == sorted(starts) and starts[0] <= a0
    for i, (start, phase, inc, ramp) in enumerate(segs):
        lo = max(start, a0)
        hi = min(starts[i + 1], a0 + n) if i + 1 < len(segs) else a0 + n
        if hi <= lo:
            continue
        if exact:
            d = np.arange(lo - start, hi - start, dtype=object)           # Python integers: no width to overflow
            phi = (int(phase) + d * int(inc) + int(ramp) * (d * (d - 1) // 2)) & M64
            out[lo - a0: hi - a0] = (phi >> 52).astype(np.int64)
        else:
            # the same in uint64, which wraps modulo 2^64 by itself; d is still a - start in full (test_wideband_tune_host.py holds
            # this branch to the one above)
            with np.errstate(over="ignore"):
                d = np.uint64(lo - start) + np.arange(hi - lo, dtype=np.uint64)
                odd = (d & np.uint64(1)).astype(bool)
                t = np.where(odd, d * ((d - np.uint64(1)) >> np.uint64(1)), (d >> np.uint64(1)) * (d - np.uint64(1)))
                phi = np.uint64(int(phase)) + d * np.uint64(int(inc)) + np.uint64(int(ramp) & M64) * t
            out[lo - a0: hi - a0] = (phi >> np.uint64(52)).astype(np.int64)
    return out


def _lo(T, segs_k, a0, n):
    i = lo_index(segs_k, a0, n)
    return T[i], T[(i - 1024) & 4095]


def _round_clip(a, S):
    if S:
        a = (a + (1 << (S - 1))) >> S
    return np.clip(a, -32768, 32767)


# ------------------------------------------------------------------ receive
def wb_tuned_model(T, wide, decim, segs, taps, out_shift, first_sample=0):
    """wb_model behind schedules: [K][2 ceil(N / D)] int16, convolution by decimation phase"""
    T = np.asarray(T, np.int64)
    I, Q = np.asarray(wide[0::2], np.int64), np.asarray(wide[1::2], np.int64)
    N, L, D = I.size, len(taps), int(decim)
    n_out = (N + D - 1) // D
    h = np.asarray(taps, np.int64)
    out = np.zeros((len(segs), 2 * n_out), np.int16)
    for k in range(len(segs)):
        c, s = _lo(T, segs[k], first_sample, N)
        acc = []
        for m in (I * c + Q * s, Q * c - I * s):
            tot = np.zeros(n_out, np.int64)
            for p in range(min(D, L)):
                x = np.concatenate([np.zeros(1 if p else 0, np.int64), m[D - p if p else 0::D]])[:n_out]
                if x.size:
                    tot[:x.size] += np.convolve(x, h[p::D])[:x.size]
            acc.append(tot)
        out[k, 0::2], out[k, 1::2] = _round_clip(acc[0], out_shift), _round_clip(acc[1], out_shift)
    return out


def wbr_tuned_model(T, wide, down, up, segs, taps, out_shift, first_sample=0):
    """wbr_model behind schedules: [K][2 ceil(N U / M)] int16, a gather per output"""
    T = np.asarray(T, np.int64)
    I, Q = np.asarray(wide[0::2], np.int64), np.asarray(wide[1::2], np.int64)
    N, L, M, U = I.size, len(taps), int(down), int(up)
    J = -(-L // U)
    n_out = wbr_outputs(M, U, N)
    tab = np.zeros(J * U, np.int64)
    tab[:L] = np.asarray(taps, np.int64)
    tab = np.ascontiguousarray(tab.reshape(J, U).T)
    r = np.arange(n_out, dtype=np.int64)
    n_r, p_r = (r * M) // U, (r * M) % U
    jj = np.arange(J, dtype=np.int64)
    out = np.zeros((len(segs), 2 * n_out), np.int16)
    block = max(1, (1 << 21) // J)
    for k in range(len(segs)):
        c, s = _lo(T, segs[k], first_sample, N)
        acc = []
        for m in (I * c + Q * s, Q * c - I * s):
            mp = np.concatenate([np.zeros(J - 1, np.int64), m])
            tot = np.zeros(n_out, np.int64)
            for b in range(0, n_out, block):
                e = min(b + block, n_out)
                tot[b:e] = (tab[p_r[b:e]] * mp[(n_r[b:e, None] + (J - 1)) - jj[None, :]]).sum(axis=1)
            acc.append(tot)
        out[k, 0::2], out[k, 1::2] = _round_clip(acc[0], out_shift), _round_clip(acc[1], out_shift)
    return out


# ------------------------------------------------------------------ transmit
def wbtx_tuned_model(T, chans, U, segs, taps, S, first_sample=0):
    """wbtx_model behind schedules: the 2 N U values of the wide capture; every channel present"""
    T = np.asarray(T, np.int64)
    U, N = int(U), len(chans[0]) // 2
    h = np.asarray(taps, np.int64)
    wr, wi = np.zeros(N * U, np.int64), np.zeros(N * U, np.int64)
    for k in range(len(segs)):
        y = []
        for x in (np.asarray(chans[k][0::2], np.int64), np.asarray(chans[k][1::2], np.int64)):
            v = np.zeros(N * U, np.int64)
            for p in range(min(U, len(h))):
                v[p::U] = np.convolve(x, h[p::U])[:N]
            y.append(v)
        c, s = _lo(T, segs[k], first_sample, N * U)
        wr += y[0] * c - y[1] * s
        wi += y[1] * c + y[0] * s
    out = np.empty(2 * N * U, np.int16)
    out[0::2], out[1::2] = _round_clip(wr, S), _round_clip(wi, S)
    return out


def wbtxr_tuned_model(T, chans, down, up, segs, taps, S, first_sample=0):
    """wbtxr_model behind schedules: the 2 ceil(N M / U) values of the wide capture; every channel present"""
    T = np.asarray(T, np.int64)
    M, U, L, N = int(down), int(up), len(taps), len(chans[0]) // 2
    J = -(-L // M)
    W = wbtxr_outputs(M, U, N)
    tab = np.zeros(J * M, np.int64)
    tab[:L] = np.asarray(taps, np.int64)
    tab = np.ascontiguousarray(tab.reshape(J, M).T)
    n = np.arange(W, dtype=np.int64)
    q_n, p_n = (n * U) // M, (n * U) % M
    jj = np.arange(J, dtype=np.int64)
    xs = [[np.concatenate([np.zeros(J - 1, np.int64), np.asarray(ch[c::2], np.int64)]) for c in (0, 1)] for ch in chans]
    lo = [_lo(T, segs[k], first_sample, W) for k in range(len(segs))]
    wr, wi = np.zeros(W, np.int64), np.zeros(W, np.int64)
    block = max(1, (1 << 21) // J)
    for b in range(0, W, block):
        e = min(b + block, W)
        rows = tab[p_n[b:e]]
        at = (q_n[b:e, None] + (J - 1)) - jj[None, :]
        for k in range(len(segs)):
            yr, yi = ((rows * x[at]).sum(axis=1) for x in xs[k])
            c, s = lo[k][0][b:e], lo[k][1][b:e]
            wr[b:e] += yr * c - yi * s
            wi[b:e] += yi * c + yr * s
    out = np.empty(2 * W, np.int16)
    out[0::2], out[1::2] = _round_clip(wr, S), _round_clip(wi, S)
    return out
