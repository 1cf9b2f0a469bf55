"""What receive diversity (opv_div_round: k_div_match, k_div_combine, k_div_scale, k_div_decode, k_div_link) costs, at two shapes:

  --bulk   64 groups x 2 branches x 1000 frames released, decoded per branch and then combined in ONE round
  --live   64 groups x 2 branches x 1 frame per round, 24 rounds: a live round

Every branch is handed a made soft log of noisy frames through opv_tap_push_soft (the second branch of a group three symbols
late), then one opv_process and one opv_div_round. Per repetition:
  per-branch decoder  opv_kernel_times[3] of the round's opv_process (HIP events around k_frame_scale + k_frame_decode)
  diversity round     host clock around opv_div_round + opv_sync, behind an opv_sync of the opv_process in front of it: the five
                      launches and nothing else are in the bracket, which ends in a device synchronise
The first repetition is warm-up and is left out of the medians. k_div_combine's own duration - and so its bytes/s against the
(B + 1) x 17 152 bytes per frame it must move - comes from a separate run of the same command under the profiler:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 scripts/diversity_cost.py --bulk --reps 2

usage: diversity_cost.py (--bulk | --live) [--reps 4] [--groups N] [--frames N]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "tests"))
import soft_log_inputs as S  # noqa: E402
from amd_lib import load  # noqa: E402
from oracle_lib import Oracle  # noqa: E402

B = 2
BYTES_PER_FRAME = (B + 1) * 2144 * 8

ap = argparse.ArgumentParser()
ap.add_argument("--bulk", action="store_true")
ap.add_argument("--live", action="store_true")
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--groups", type=int, default=64)
ap.add_argument("--frames", type=int, default=0)
a = ap.parse_args()
if a.bulk == a.live:
    ap.error("one of --bulk / --live")
amd = load()
o = Oracle()
rng = np.random.default_rng(7)
G = a.groups
n_frames = a.frames or (1000 if a.bulk else 24)
LEAD, LATE = 10, 3


def made_log(late):
    return S.cat(S.zeros(LEAD + late), *[S.cat(S.sync(S.A), S.payload(o, k % 50, sigma=400.0, rng=rng)) for k in range(n_frames)],
                 S.zeros(40 - late))


logs = [made_log(0), made_log(LATE)]
d = amd.Demod(B * G, max_samples=(n_frames + 8) * 2168 * 38, streaming=True)
d.enable_timing()
div = amd.Diversity(d, [[B * g, B * g + 1] for g in range(G)])


def one_round(lo, hi):
    """symbols [lo, hi) of its log to every branch, the context's round, then the timed diversity round -> (decoder bracket ms,
    diversity round ms)"""
    for s in range(B * G):
        d.push_soft(s, logs[s % B][lo:hi])
    d.process()
    d.sync()
    dec = d.kernel_times()["frame_decode"]
    t0 = time.perf_counter()
    div.round()
    d.sync()
    return dec, (time.perf_counter() - t0) * 1e3


def drain(expect):
    """pops every branch and every group; the group frames must all be there, both branches in each"""
    for s in range(B * G):
        d.pop_frames(s)
    for g in range(G):
        fr, meta = div.pop_frames(g)
        assert len(fr) == expect and np.all(meta["members"] == 3) and np.all(meta["summed"] == 3), (g, len(fr), expect)


res = []
n = len(logs[0])
if a.bulk:
    for rep in range(a.reps + 1):
        if rep:
            d.reset(-1)
        dec, rnd = one_round(0, n)
        drain(n_frames)
        if rep:
            res.append((dec, rnd))
        print(f"rep {rep}: per-branch decoder bracket {dec:8.3f} ms, diversity round {rnd:8.3f} ms" + ("" if rep else " (warm-up, left out)"), flush=True)
    frames_per_round = G * n_frames
else:
    # one frame per branch and round: round r hands every branch the symbols up to the release of frame r on the later branch
    cuts = [0] + [LEAD + LATE + 2168 * (k + 1) for k in range(n_frames)]
    for rep in range(a.reps + 1):
        if rep:
            d.reset(-1)
        per = []
        for r in range(n_frames):
            per.append(one_round(cuts[r], cuts[r + 1]))
            drain(1)
        per = per[4:]                                        # (the first rounds of a fresh context warm the launch paths)
        m = (statistics.median(p[0] for p in per), statistics.median(p[1] for p in per))
        if rep:
            res.append(m)
        print(f"rep {rep}: median of {len(per)} rounds: per-branch decoder bracket {m[0]:8.4f} ms, diversity round {m[1]:8.4f} ms"
              + ("" if rep else " (warm-up, left out)"), flush=True)
    frames_per_round = G
div.close()
d.close()
print(f"shape: {G} groups x {B} branches x {n_frames if a.bulk else 1} frame(s) per round = {frames_per_round} group frames, "
      f"{frames_per_round * BYTES_PER_FRAME / 1e6:.3f} MB for k_div_combine")
for name, k in (("per-branch decoder bracket (opv_kernel_times[3])", 0), ("diversity round (five launches, host clock)", 1)):
    v = [x[k] for x in res]
    print(f"{name}: median {statistics.median(v):.4f} ms (min {min(v):.4f}, max {max(v):.4f}) over {len(v)} repetitions")
