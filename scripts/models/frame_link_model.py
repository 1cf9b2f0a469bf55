"""numpy model of k_frame_link's index algebra, checked against the oracle's encoder BEFORE the kernel was written: which bits of
the decoded frame trellis step t reads, which parity is G1, and which payload symbol carries which code bit.
  * the decoder's bit string is the frame XOR the LFSR table; decoded bit t is bit (1071 - t) & 7 of byte (1071 - t) >> 3
    (the packer of src/opv-demod.cpp:878-884 backwards), so bits t .. t - 6 are seven consecutive bits from position
    p = 1071 - t of that string read little-endian; two zero bytes behind byte 133 are the zeros in front of t = 0
  * v = those seven bits (bit 0 = bit t); the reference's f (:819) = ((v & 1) << 6) | (v >> 1); e1 = parity(f & 0x4F) is code
    bit 2 t, e2 = parity(f & 0x6D) code bit 2 t + 1 (:820-824)
  * code bit j is payload symbol deinterleave_addr(j) (:792-795)
  * backwards (an on-air-order variant of the kernel, measured and not kept): symbol a carries code bit
    j = (pos % 67) * 32 + pos / 67, pos = a with its low three bits reversed
usage: python scripts/models/frame_link_model.py [n_trials]"""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[2]
sys.path.insert(0, str(ROOT / "tests"))


def deint(i):
    p = (i & 31) * 67 + (i >> 5)
    return (p & ~7) + (7 - (p & 7))


def par(x):
    return bin(x).count("1") & 1


def window(rb, t):
    p = 1071 - t
    w = int(rb[p >> 3]) | (int(rb[(p >> 3) + 1]) << 8)
    v = (w >> (p & 7)) & 0x7F
    return ((v & 1) << 6) | (v >> 1)


def main():
    from oracle_lib import Oracle
    o = Oracle()
    lfsr = o.lfsr_table()
    rng = np.random.default_rng(1)
    for trial in range(int(sys.argv[1]) if len(sys.argv) > 1 else 5):
        fr = rng.integers(0, 256, 134, dtype=np.uint8) if trial else o.bert_frames(1)[0]
        rb = np.zeros(136, np.uint8)
        rb[:134] = fr ^ lfsr
        ref = o.encode_frame(fr)
        by_step = np.zeros(2144, np.uint8)
        for t in range(1072):
            f = window(rb, t)
            by_step[deint(2 * t)] = par(f & 0x4F)
            by_step[deint(2 * t + 1)] = par(f & 0x6D)
        on_air = np.zeros(2144, np.uint8)
        for a in range(2144):
            pos = (a & ~7) + 7 - (a & 7)
            j = (pos % 67) * 32 + pos // 67
            assert deint(j) == a
            on_air[a] = par(window(rb, j >> 1) & (0x6D if j & 1 else 0x4F))
        ok = np.array_equal(by_step, ref) and np.array_equal(on_air, ref)
        print("trial", trial, "by step", int((by_step != ref).sum()), "on air", int((on_air != ref).sum()), "differences")
        assert ok


if __name__ == "__main__":
    main()
