"""The integer model of the wideband scan: the arithmetic of include/opv_demod.h (opv_scan_*) restated in numpy int64, the block
count, and opv_scan_carriers' rule in python integers and floats. numpy only: importable with no device and no build. The CPU
test (tests/test_scan_host.py) holds the host code to these functions; the GPU test (tests/test_gpu_scan.py) holds the device's
rows to scan_model with ==. The increments are the rational door's: wideband_models.wbr_model_inc."""
import math

import numpy as np


def scan_segments(n_window, hop, n):
    return 0 if n < n_window else (int(n) - int(n_window)) // int(hop) + 1


def scan_blocks(n_window, hop, n_avg, n):
    return scan_segments(n_window, hop, n) // int(n_avg)


def scan_shape(n_probes, n_avg, blocks):
    """-> (run_len, runs, pgroups): how a push that completes `blocks` blocks is launched (csrc/opv_scan_rules.cpp, scan_shape: groups
    of 256 probes; a block's A segments cut into runs so that blocks x runs x groups reaches 2048 workgroups where A allows).
    Nothing of the rows depends on it; the GPU cases use it to SAY which launch shapes they run, and tests/test_scan_host.py holds
    it to the C rule."""
    pgroups = -(-int(n_probes) // 256)
    have = max(int(blocks), 1) * pgroups
    want = min(int(n_avg), -(-2048 // have))
    run_len = -(-int(n_avg) // want)
    return run_len, -(-int(n_avg) // run_len), pgroups


def scan_keep(n_window, hop, n_avg, n):
    """samples the object carries after n samples: those from the start of the first unfinished block on (0 if it has not arrived)"""
    return max(0, int(n) - scan_blocks(n_window, hop, n_avg, n) * int(n_avg) * int(hop))


def hann_window(n_window, peak=2047):
    """the integer Hann window of the end-to-end case and the cost script: lrint(peak sin^2(pi (t + 1/2) / Lw)); 1024 taps of peak
    2047 sum to 2^20, inside the 2^21 cap"""
    t = np.arange(n_window, dtype=np.float64)
    w = np.rint(peak * np.sin(np.pi * (t + 0.5) / n_window) ** 2).astype(np.int16)
    assert np.abs(w.astype(np.int64)).sum() <= 1 << 21
    return w


def scan_segment_sums(T, wide, inc, window, H, first_sample=0, n_segs=None):
    """z[p][s] = (sum_t w[t] mr_p[s H + t], sum_t w[t] mi_p[s H + t]) as two int64 arrays [P][segs], before the shift"""
    T = np.asarray(T, np.int64)
    I, Q = np.asarray(wide[0::2], np.int64), np.asarray(wide[1::2], np.int64)
    w = np.asarray(window, np.int64)
    N, Lw, H = I.size, w.size, int(H)
    assert int(np.abs(w).sum()) <= 1 << 21
    segs = scan_segments(Lw, H, N) if n_segs is None else n_segs
    P = len(inc)
    zr, zi = np.zeros((P, segs), np.int64), np.zeros((P, segs), np.int64)
    if segs == 0:
        return zr, zi
    used = (segs - 1) * H + Lw                                             # samples behind the last segment reach nothing
    # only the low 32 bits of a reach phi, and numpy's uint32 product wraps modulo 2^32: phi = (uint32)(a x inc) as the header writes it
    a = ((np.arange(used, dtype=np.uint64) + np.uint64(first_sample % (1 << 64))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    at = np.arange(segs, dtype=np.int64)[:, None] * H + np.arange(Lw, dtype=np.int64)[None, :]              # [segs][Lw] sample indices
    step = max(1, (1 << 22) // max(used, segs * Lw))                       # probes per pass: bounded memory
    T32 = T.astype(np.int32)
    Ts32 = T32[(np.arange(4096) - 1024) & 4095]                            # s = T[(i - 1024) & 4095] = Ts[i]
    I, Q = I[None, :used].astype(np.int32), Q[None, :used].astype(np.int32)
    for p0 in range(0, P, step):
        phi = a[None, :] * np.asarray(inc[p0:p0 + step], np.uint32)[:, None]
        i = phi >> np.uint32(20)
        c, s = T32[i], Ts32[i]
        mr, mi = I * c + Q * s, Q * c - I * s                              # int32: |.| <= 2 x 32768 x 32767 < 2^31
        zr[p0:p0 + step] = np.matmul(mr[:, at], w, dtype=np.int64)
        zi[p0:p0 + step] = np.matmul(mi[:, at], w, dtype=np.int64)
    return zr, zi


def scan_model(T, wide, inc, window, H, A, S, first_sample=0):
    """wide: interleaved int16 IQ of the WHOLE capture (n = 0 at its first sample). Returns uint64 [blocks][P]: the rows the object
    must deliver, whatever the split into pushes. Every product and sum is exact in int64 (|z| < 2^52, e <= 2^49, E <= 2^61)."""
    Lw, A, S = len(window), int(A), int(S)
    blocks = scan_blocks(Lw, H, A, len(wide) // 2)
    zr, zi = scan_segment_sums(T, wide, inc, window, H, first_sample, n_segs=blocks * A)
    assert max(np.max(np.abs(zr), initial=0), np.max(np.abs(zi), initial=0)) < 1 << 52
    if S:
        zr, zi = (zr + (1 << (S - 1))) >> S, (zi + (1 << (S - 1))) >> S    # numpy's >> on int64 is arithmetic: floor
    yr, yi = np.clip(zr, -(1 << 24), (1 << 24) - 1), np.clip(zi, -(1 << 24), (1 << 24) - 1)
    e = (yr * yr + yi * yi).astype(np.uint64)                              # [P][blocks A]
    return np.ascontiguousarray(e.reshape(len(inc), blocks, A).sum(axis=2, dtype=np.uint64).T)


def carriers_model(row, f0_hz, step_hz, half_width_hz, ratio_q8, cap):
    """opv_scan_carriers' rule in python integers (the boxes, the comparison) and floats (the centroid, in ascending j); returns
    [(centre_hz, probe, excess)], strongest first"""
    row = [int(v) for v in row]
    P = len(row)
    floor = sorted(row)[P // 2]
    W = max(1, math.ceil(float(half_width_hz) / float(step_hz)))
    W = min(W, P)                                                          # (beyond the row every W reaches the same probes)
    box, n = [], []
    for i in range(P):
        lo, hi = max(0, i - W), min(P - 1, i + W)
        box.append(sum(row[lo:hi + 1]))
        n.append(hi - lo + 1)
    cands = sorted((i for i in range(P) if box[i] * 256 > int(ratio_q8) * n[i] * floor), key=lambda i: (-box[i], i))
    out, taken = [], []
    for i in cands:
        if len(out) >= cap:
            break
        if any(abs(i - t) <= 2 * W for t in taken):
            continue
        num = den = 0.0
        for j in range(max(0, i - W), min(P - 1, i + W) + 1):
            e = row[j] - floor if row[j] > floor else 0
            num += float(e) * float(j - i)
            den += float(e)
        out.append((float(f0_hz) + (float(i) + (num / den if den > 0 else 0.0)) * float(step_hz), i, den))
        taken.append(i)
    return out
