"""Made branch logs for receive diversity: a test INPUT generator on top of soft_log_inputs.py, nothing here is a reference.

A branch log carries the same transmitted frames 0 .. N-1 as its group's other branches, moved by a few symbols, with its own
noise on the PAYLOADS only (sync words stay clean unless a case erases one, so every tracker decision is exact), and a tail of
silence long enough for every tracker to lose lock: behind it every branch's earliest future payload lies beyond every frame,
and every group frame is final.

    groups = main_groups(oracle)       # [[Branch, ...], ...]: the three groups of the main parity test (3, 2 and 1 branches)
    Branch.soft / .shift / .note"""
from dataclasses import dataclass

import numpy as np

import soft_log_inputs as S

N_FRAMES = 6
LEAD = 10
TAIL = 5 * S.FSYMS + 40                         # five missed sync words: LOST_LOCK, then HUNTING to the log's end
SEED = 21                                       # (chosen so that test_diversity_host.py's non-vacuity checks hold)
QUIET, LOUD = 150.0, 560.0                      # payload noise: an easy frame, and one a single branch decodes wrongly (A = 500)
LOUD_FRAMES = (2, 4)


@dataclass
class Branch:
    soft: np.ndarray
    shift: int
    note: str = ""


def branch_log(o, rng, shift=0, first=0, last=N_FRAMES, erased=(), loud=LOUD_FRAMES, amp=S.A, nan_at=None, n_frames=N_FRAMES,
               quiet=QUIET, loud_sigma=LOUD, tail=TAIL):
    """frames first .. last-1 of the transmission (the others are silence), sync words of `erased` frames zeroed"""
    parts = [S.zeros(LEAD + shift)]
    for k in range(n_frames):
        if not first <= k < last:
            parts.append(S.zeros(S.FSYMS))
            continue
        sigma = loud_sigma if k in loud else quiet
        p = S.payload(o, k, amp, sigma * amp / S.A, rng)
        if nan_at is not None and nan_at[0] == k:
            p = p.copy()
            p[nan_at[1]] = np.nan
        parts += [S.zeros(S.SYNC_BITS) if k in erased else S.sync(amp), p]
    parts.append(S.zeros(tail - shift))
    return S.cat(*parts)


def main_groups(o, seed=SEED):
    """group 0: three branches at 0 / +3 / -2 symbols - the second HUNTING through the first two frames (sync words erased), the
    third ending two frames early; group 1: two branches, one with a flywheel frame (frame 3's sync word erased while LOCKED) and
    a NaN in frame 1's payload; group 2: one branch"""
    rng = np.random.default_rng(seed)
    g0 = [Branch(branch_log(o, rng, 0), 0, "whole"),
          Branch(branch_log(o, rng, 3, erased=(0, 1)), 3, "HUNTING through frames 0 and 1"),
          Branch(branch_log(o, rng, -2, last=4), -2, "ends two frames early")]
    g1 = [Branch(branch_log(o, rng, 0, erased=(3,)), 0, "flywheel frame 3"),
          Branch(branch_log(o, rng, 3, nan_at=(1, 777)), 3, "NaN in frame 1")]
    g2 = [Branch(branch_log(o, rng, -2), -2, "alone")]
    return [g0, g1, g2]
