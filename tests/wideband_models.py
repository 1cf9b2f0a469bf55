"""The integer models of the four wideband converters: the arithmetic of include/opv_demod.h (opv_wb_*, opv_wbr_*, opv_wbtx_*,
opv_wbtxr_*) restated in numpy int64, and the tap generators their tests draw from. numpy only: importable with no device and no
build. The CPU tests (tests/test_wideband*_host.py) hold the host code to these functions, and the models to each other and to
literal one-product-at-a-time restatements; the GPU tests (tests/test_gpu_wideband*.py) hold the device to them with ==.

wb_model (convolution by decimation phase) and wbr_model (gather per output) are two independent derivations of the receive side,
as wbtx_model and wbtxr_model are of the transmit side: with up = 1 they must agree, and the tests say so."""
import numpy as np

WIDE_RATE = 2168000.0


# ------------------------------------------------------------------ increments and output counts
def wb_model_inc(decim, centre_hz):
    """inc_k = (uint32) llrint(f_k / (D * 2 168 000) * 2^32), modulo 2^32 (python integers: no width to overflow)"""
    return np.array([int(np.rint(np.float64(f) / (np.float64(decim) * WIDE_RATE) * 4294967296.0)) % (1 << 32) for f in centre_hz], np.uint32)


def wbr_model_inc(down, up, centre_hz):
    """fw = (double)M x 2 168 000.0 / (double)U; inc_k = (uint32) llrint(f_k / fw x 2^32), modulo 2^32 (python integers: no width to overflow)"""
    fw = np.float64(down) * WIDE_RATE / np.float64(up)
    return np.array([int(np.rint(np.float64(f) / fw * 4294967296.0)) % (1 << 32) for f in centre_hz], np.uint32)


def wbr_outputs(down, up, n):
    return -(-(int(n) * int(up)) // int(down))


def wbtxr_outputs(down, up, n):
    """W(N) = ceil(N M / U) in python integers"""
    return -(-(int(n) * int(down)) // int(up))


# ------------------------------------------------------------------ receive: the integer door
def wb_model(T, wide, decim, inc, taps, out_shift, first_sample=0):
    """wide: interleaved int16 IQ of the WHOLE capture (n = 0 at its first sample). Returns [K][2 * ceil(N / D)] int16: what every
    channel's stream must hold, whatever the split into pushes. Every product and sum is exact in int64 (|acc| < 2^52)."""
    T = np.asarray(T, np.int64)
    I, Q = np.asarray(wide[0::2], np.int64), np.asarray(wide[1::2], np.int64)
    N, L, D = I.size, len(taps), int(decim)
    n_out = (N + D - 1) // D
    h = np.asarray(taps, np.int64)
    a = (np.arange(N, dtype=np.uint64) + np.uint64(first_sample % (1 << 64))) & np.uint64(0xFFFFFFFF)      # only the low 32 bits of a reach phi
    out = np.zeros((len(inc), 2 * n_out), np.int16)
    for k, w in enumerate(inc):
        phi = (a * np.uint64(int(w))) & np.uint64(0xFFFFFFFF)              # (a < 2^32 and inc < 2^32: the product fits uint64)
        i = (phi >> np.uint64(20)).astype(np.int64)
        c, s = T[i], T[(i - 1024) & 4095]
        acc = []
        for m in (I * c + Q * s, Q * c - I * s):
            assert np.max(np.abs(m), initial=0) < 1 << 31
            # acc[r] = sum_t h[t] m[r D - t], taken by decimation phase (t = p + j D): sum_p (x_p * h_p)[r] with x_p[r] = m[r D - p]
            # (0 in front of sample 0) and h_p = h[p], h[p + D], ... - the same int64 products and sums, in another order
            tot = np.zeros(n_out, np.int64)
            for p in range(min(D, L)):
                x = np.concatenate([np.zeros(1 if p else 0, np.int64), m[D - p if p else 0::D]])[:n_out]
                if x.size:
                    tot[:x.size] += np.convolve(x, h[p::D])[:x.size]
            acc.append(tot)
        ar, ai = acc
        if out_shift:
            ar, ai = (ar + (1 << (out_shift - 1))) >> out_shift, (ai + (1 << (out_shift - 1))) >> out_shift       # numpy's >> on int64 is arithmetic: floor
        out[k, 0::2], out[k, 1::2] = np.clip(ar, -32768, 32767), np.clip(ai, -32768, 32767)
    return out


# ------------------------------------------------------------------ receive: the rational door
def wbr_model(T, wide, down, up, inc, taps, out_shift, first_sample=0):
    """wide: interleaved int16 IQ of the WHOLE capture (n = 0 at its first sample). Returns [K][2 * ceil(N U / M)] int16: what every
    channel's stream must hold, whatever the split into pushes. acc[r] = sum_j taps[p_r + j U] m[n_r - j] by a gather of m per
    output (rows of r, columns of j), in blocks of outputs; every product and sum is exact in int64 (|acc| < 2^52)."""
    T = np.asarray(T, np.int64)
    I, Q = np.asarray(wide[0::2], np.int64), np.asarray(wide[1::2], np.int64)
    N, L, M, U = I.size, len(taps), int(down), int(up)
    J = -(-L // U)
    n_out = wbr_outputs(M, U, N)
    tab = np.zeros(J * U, np.int64)
    tab[:L] = np.asarray(taps, np.int64)
    tab = np.ascontiguousarray(tab.reshape(J, U).T)                        # tab[p, j] = taps[p + j U]
    r = np.arange(n_out, dtype=np.int64)
    n_r, p_r = (r * M) // U, (r * M) % U
    assert n_out == 0 or n_r[-1] < N
    jj = np.arange(J, dtype=np.int64)
    a = (np.arange(N, dtype=np.uint64) + np.uint64(first_sample % (1 << 64))) & np.uint64(0xFFFFFFFF)      # only the low 32 bits of a reach phi
    out = np.zeros((len(inc), 2 * n_out), np.int16)
    block = max(1, (1 << 21) // J)
    for k, w in enumerate(inc):
        phi = (a * np.uint64(int(w))) & np.uint64(0xFFFFFFFF)
        i = (phi >> np.uint64(20)).astype(np.int64)
        c, s = T[i], T[(i - 1024) & 4095]
        acc = []
        for m in (I * c + Q * s, Q * c - I * s):
            assert np.max(np.abs(m), initial=0) < 1 << 31
            mp = np.concatenate([np.zeros(J - 1, np.int64), m])           # m[n] = 0 for n < 0: sample n sits at n + J - 1
            tot = np.zeros(n_out, np.int64)
            for b in range(0, n_out, block):
                e = min(b + block, n_out)
                tot[b:e] = (tab[p_r[b:e]] * mp[(n_r[b:e, None] + (J - 1)) - jj[None, :]]).sum(axis=1)
            acc.append(tot)
        ar, ai = acc
        if out_shift:
            ar, ai = (ar + (1 << (out_shift - 1))) >> out_shift, (ai + (1 << (out_shift - 1))) >> out_shift       # numpy's >> on int64 is arithmetic: floor
        out[k, 0::2], out[k, 1::2] = np.clip(ar, -32768, 32767), np.clip(ai, -32768, 32767)
    return out


# ------------------------------------------------------------------ transmit: the integer bank
def wbtx_model(T, chans, U, inc, taps, S, first_sample=0):
    """chans[k]: interleaved int16 IQ of channel k's WHOLE input (every channel N samples; None = N zeros, N taken from the others
    or, if all are None, an int N in its place). Returns the 2 * N * U interleaved int16 values of the wide capture, whatever the
    split into pushes. Every product and sum is exact in int64 (|y| < 2^31, |sum| < 2^55)."""
    T = np.asarray(T, np.int64)
    U = int(U)
    sizes = {c if isinstance(c, (int, np.integer)) else len(c) // 2 for c in chans if c is not None}
    assert len(sizes) == 1, "every channel delivers the same number of samples"
    N = int(sizes.pop())
    h = np.asarray(taps, np.int64)
    n = np.arange(N * U, dtype=np.uint64)
    a = (n + np.uint64(first_sample % (1 << 64))) & np.uint64(0xFFFFFFFF)                                   # only the low 32 bits of a reach phi
    wr, wi = np.zeros(N * U, np.int64), np.zeros(N * U, np.int64)
    for k, w in enumerate(inc):
        if chans[k] is None or isinstance(chans[k], (int, np.integer)):
            continue                                                       # zeros in, zeros out: nothing to add
        y = []
        for x in (np.asarray(chans[k][0::2], np.int64), np.asarray(chans[k][1::2], np.int64)):
            # y[q U + p] = sum_j h[p + j U] x[q - j]: by phase, the convolution of x with h[p::U] (a phase without a tap gives zeros)
            v = np.zeros(N * U, np.int64)
            for p in range(min(U, len(h))):
                v[p::U] = np.convolve(x, h[p::U])[:N]
            assert np.max(np.abs(v), initial=0) < 1 << 31
            y.append(v)
        yr, yi = y
        phi = (a * np.uint64(int(w))) & np.uint64(0xFFFFFFFF)              # (a < 2^32 and inc < 2^32: the product fits uint64)
        i = (phi >> np.uint64(20)).astype(np.int64)
        c, s = T[i], T[(i - 1024) & 4095]
        wr += yr * c - yi * s
        wi += yi * c + yr * s
    if S:
        wr, wi = (wr + (1 << (S - 1))) >> S, (wi + (1 << (S - 1))) >> S    # numpy's >> on int64 is arithmetic: floor
    out = np.empty(2 * N * U, np.int16)
    out[0::2], out[1::2] = np.clip(wr, -32768, 32767), np.clip(wi, -32768, 32767)
    return out


# ------------------------------------------------------------------ transmit: the rational bank
def wbtxr_model(T, chans, down, up, inc, taps, S, first_sample=0):
    """chans[k]: interleaved int16 IQ of channel k's WHOLE input (every channel N samples; None = N zeros, N taken from the others
    or, if all are None, an int N in its place). Returns the 2 * ceil(N M / U) interleaved int16 values of the wide capture, whatever
    the split into pushes. y[n] = sum_j taps[p_n + j M] x[q_n - j] by a gather of x per output (rows of n, columns of j) from the
    (M, J) table, in blocks of outputs; every product and sum is exact in int64 (|y| < 2^31, |sum| < 2^55)."""
    T = np.asarray(T, np.int64)
    M, U, L = int(down), int(up), len(taps)
    sizes = {c if isinstance(c, (int, np.integer)) else len(c) // 2 for c in chans if c is not None}
    assert len(sizes) == 1, "every channel delivers the same number of samples"
    N = int(sizes.pop())
    J = -(-L // M)
    W = wbtxr_outputs(M, U, N)
    tab = np.zeros(J * M, np.int64)
    tab[:L] = np.asarray(taps, np.int64)
    tab = np.ascontiguousarray(tab.reshape(J, M).T)                        # tab[p, j] = taps[p + j M]
    n = np.arange(W, dtype=np.int64)
    q_n, p_n = (n * U) // M, (n * U) % M
    assert W == 0 or q_n[-1] < N
    jj = np.arange(J, dtype=np.int64)
    a = (n.astype(np.uint64) + np.uint64(first_sample % (1 << 64))) & np.uint64(0xFFFFFFFF)               # only the low 32 bits of a reach phi
    live = [k for k in range(len(inc)) if chans[k] is not None and not isinstance(chans[k], (int, np.integer))]
    # x[m] = 0 for m < 0: sample m sits at m + J - 1
    xs = {k: [np.concatenate([np.zeros(J - 1, np.int64), np.asarray(chans[k][c::2], np.int64)]) for c in (0, 1)] for k in live}
    wr, wi = np.zeros(W, np.int64), np.zeros(W, np.int64)
    block = max(1, (1 << 21) // J)
    for b in range(0, W, block):
        e = min(b + block, W)
        rows = tab[p_n[b:e]]                                               # the gathers are the same for every channel: once per block
        at = (q_n[b:e, None] + (J - 1)) - jj[None, :]
        for k in live:
            yr, yi = ((rows * x[at]).sum(axis=1) for x in xs[k])
            assert max(np.max(np.abs(yr), initial=0), np.max(np.abs(yi), initial=0)) < 1 << 31
            phi = (a[b:e] * np.uint64(int(inc[k]))) & np.uint64(0xFFFFFFFF)        # (a < 2^32 and inc < 2^32: the product fits uint64)
            i = (phi >> np.uint64(20)).astype(np.int64)
            c, s = T[i], T[(i - 1024) & 4095]
            wr[b:e] += yr * c - yi * s
            wi[b:e] += yi * c + yr * s
    if S:
        wr, wi = (wr + (1 << (S - 1))) >> S, (wi + (1 << (S - 1))) >> S    # numpy's >> on int64 is arithmetic: floor
    out = np.empty(2 * W, np.int16)
    out[0::2], out[1::2] = np.clip(wr, -32768, 32767), np.clip(wi, -32768, 32767)
    return out


# ------------------------------------------------------------------ taps
def halved_taps(rng, L, gain_cap=1 << 21):
    """random int16 taps, halved as a whole until sum |.| <= gain_cap (the receive side's cap on a phase)"""
    h = rng.integers(-32768, 32768, L).astype(np.int64)
    while np.abs(h).sum() > gain_cap:
        h = h // 2
    return h.astype(np.int16)


def per_phase_taps(rng, L, up, cap=1 << 21):
    """random int16 taps whose EVERY phase (taps[p::up]) keeps sum |.| <= cap: halved_taps drawn per phase, phase after phase"""
    taps = np.zeros(L, np.int16)
    for p in range(min(up, L)):
        taps[p::up] = halved_taps(rng, len(taps[p::up]), cap)
    return taps


def tx_phase_taps(rng, L, U):
    """the transmit side's: ONE draw of L random int16 taps, then every phase (taps[p::U]) halved until its sum of |taps| is within 65535"""
    h = rng.integers(-32768, 32768, L).astype(np.int64)
    for p in range(min(U, L)):
        while np.abs(h[p::U]).sum() > 65535:
            h[p::U] //= 2
    return h.astype(np.int16)
