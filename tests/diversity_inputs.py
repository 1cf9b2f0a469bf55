"""Made branch logs for receive diversity: a test INPUT generator on top of soft_log_inputs.py, nothing here is a reference.

A branch log carries the same transmitted frames 0 .. N-1 as its group's other branches, moved by a few symbols, with its own
noise on the PAYLOADS only (sync words stay clean unless a case erases one, so every tracker decision is exact), and a tail of
silence long enough for every tracker to lose lock: behind it every branch's earliest future payload lies beyond every frame,
and every group frame is final.

    groups = main_groups(oracle)       # [[Branch, ...], ...]: the three groups of the main parity test (3, 2 and 1 branches)
    Branch.soft / .shift / .note
    eight_groups, window_pair, many_recipes + prefixed, backlog_pair, ahead_group, normalised_eight, two_receptions (int16 IQ):
    the inputs of tests/test_gpu_diversity_limits.py"""
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


# ---- the limits (tests/test_gpu_diversity_limits.py; their non-vacuity is shown on the CPU by tests/test_diversity_host.py) ----
EIGHT_STREAMS = [11, 2, 9, 4, 13, 0, 7, 6]      # branch b's stream in a 16-stream context: branch order is not stream order
EIGHT_SHIFTS = [0, 8, 1, 7, 2, 6, 3, 5]         # every offset of the window of 8, the largest next to the anchor
EIGHT_WEIGHTS = [1e-3, 1e3, 1.0, 3.0, 0.1, 30.0, 7.0, 0.5]      # six decades: the order of the additions shows in the low bits
EIGHT_LOUD = (1, 2, 3, 4)
EIGHT_SIGMA = 800.0                             # a single branch decodes such a frame wrongly, eight of them together do not
FIVE_STREAMS = [14, 1, 10, 3, 12]
FIVE_SHIFTS = [0, 3, -2, 5, 1]
NEIGHBOUR = 5                                   # an ungrouped stream of the same context
WINDOW_CASES = [(0, (0, 0)), (0, (0, 1)), (64, (0, 64)), (64, (0, 65)), (64, (65, 0))]
MANY_GROUPS = 65                                # one more than a k_div_scale block
MANY_COUNTS = (1, 2, 3, 5, 8)                   # group g has MANY_COUNTS[g % 5] branches ...
MANY_PREFIX = 311                               # ... and every log of it (g % 7) * 311 zero symbols in front


def eight_groups(o, seed=31):
    """-> ([g8, g5], neighbour log). g8: eight branches of the whole transmission, frames 1-4 loud on every one of them; g5: five
    branches, the second HUNTING through the first two frames, the third ending two frames early (as main_groups does for three);
    and an ordinary log for a stream of no group"""
    rng = np.random.default_rng(seed)
    g8 = [Branch(branch_log(o, rng, sh, loud=EIGHT_LOUD, loud_sigma=EIGHT_SIGMA), sh) for sh in EIGHT_SHIFTS]
    kw = [dict(), dict(erased=(0, 1)), dict(last=4), dict(), dict()]
    g5 = [Branch(branch_log(o, rng, sh, **k), sh, str(k)) for sh, k in zip(FIVE_SHIFTS, kw)]
    return [g8, g5], branch_log(o, rng, 4)


def window_pair(o, shifts, seed=3):
    """two quiet branches `shifts` symbols behind the grid: for the windows of 0 and 64 symbols"""
    rng = np.random.default_rng(seed)
    return [Branch(branch_log(o, rng, sh, loud=()), sh) for sh in shifts]


def many_recipes(o, seed=41):
    """{branch count: group} for MANY_COUNTS: the groups of one count share their logs but for the prefix. In the group of two the
    second branch lies 9 symbols behind the first, one outside the window of 8: every transmitted frame gives that group two
    frames, so a round of it can emit two where another group emits one or none."""
    rng = np.random.default_rng(seed)
    shifts = {1: [0], 2: [0, 9], 3: [0, 3, -2], 5: FIVE_SHIFTS, 8: EIGHT_SHIFTS}
    out = {}
    for n in MANY_COUNTS:
        out[n] = [Branch(branch_log(o, rng, sh, erased=(0, 1) if (n, b) == (3, 1) else (), last=4 if (n, b) == (5, 2) else N_FRAMES), sh)
                  for b, sh in enumerate(shifts[n])]
    return out


def prefixed(group, prefix):
    return [Branch(S.cat(S.zeros(prefix), b.soft), b.shift + prefix, b.note) for b in group]


def backlog_pair(o, seed=13, n_frames=18):
    """two quiet branches of 18 frames: more than two output rings of eight"""
    rng = np.random.default_rng(seed)
    return [Branch(branch_log(o, rng, sh, last=n_frames, loud=(), n_frames=n_frames), sh) for sh in (0, 5)]


# (last, tail) of the eight branches that ran ahead: 16 frame slots each, the transmission ending at `last`; tail 40 leaves a
# tracker that still has its lock LOCKED at the log's end, 2040 more symbols make that log longer than its soft ring by one payload more
AHEAD = [(16, 40), (16, 2040), (10, 40), (13, 40), (12, 2040), (9, 40), (11, 40), (16, 2040)]


def ahead_group(o, seed=17):
    rng = np.random.default_rng(seed)
    return [Branch(branch_log(o, rng, sh, last=last, loud=(), n_frames=16, tail=tail + sh), sh)
            for sh, (last, tail) in zip(EIGHT_SHIFTS, AHEAD)]


def normalised_eight(o, seed=19):
    """eight branches for normalised mode: branch 2 ten times louder, branch 5 with a NaN in EVERY payload (its scale is not
    finite: matched, never summed)"""
    rng = np.random.default_rng(seed)
    g = []
    for b, sh in enumerate(EIGHT_SHIFTS):
        log = branch_log(o, rng, sh, amp=10 * S.A if b == 2 else S.A)
        if b == 5:
            for k in range(N_FRAMES):
                log[LEAD + sh + S.FSYMS * k + S.SYNC_BITS + 100 + k] = np.nan
        g.append(Branch(log, sh))
    return g


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


RECEPTION_DELAY = 120                           # samples: 3 symbols
RECEPTION_LEAD = 40                             # one symbol of silence in front of both: payloads then start at 1 and 0 mod 4, so
#                                                 a shift by a multiple of 4 can put symbol 2^32 between the two members of a frame


def two_receptions(o, n_frames=8, ebn0_db=14.0):
    """two noisy receptions (int16 IQ) of one transmission of eight frames, the second RECEPTION_DELAY samples late: the inputs
    of the imported-branch cases, at a level where the oracle decodes every frame of both"""
    from oracle_lib import impair
    clean = o.modulate(o.bert_frames(n_frames))
    pad = lambda n: np.concatenate([np.zeros(2 * n, clean.dtype), clean])
    return [impair(pad(RECEPTION_LEAD), amp=2000.0, ebn0_db=ebn0_db, seed=5),
            impair(pad(RECEPTION_LEAD + RECEPTION_DELAY), amp=2000.0, ebn0_db=ebn0_db, seed=6)]
