"""What the link report (opv_enable_link_report: k_frame_link behind the decoder) costs, at two shapes:

  --bulk   512 streams x 1000 frames released and decoded in ONE round (the shape behind "512 000 frames decode in 9.9 ms"):
           every stream is handed the same made soft log of 1000 noisy frames through opv_tap_push_soft, then one opv_process
  --live   64 streams x 1 frame per round, 24 rounds: a live round

Per repetition, alternating report off / on on the same context and the same log:
  decoder bracket  opv_kernel_times[3] (HIP events of opv_enable_timing around k_frame_scale + k_frame_decode): must not move
  round            host clock around opv_process + opv_sync (the work ends in a device synchronise)
The first repetition of each kind is warm-up and is left out of the medians. on - off of the round is the report's cost IN the
round. The library has no event pair of its own around the link launch (opv_kernel_times keeps its four brackets), so the
kernel's own duration comes from a separate run of the same command under the profiler:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 scripts/link_report_cost.py --bulk --reps 2

Bytes the kernel needs per frame, from the shapes: 2144 x 8 of soft symbols + 134 of frame in, 40 of record out = 17 326 B.
usage: link_report_cost.py (--bulk | --live) [--reps 4] [--streams N] [--frames N]"""
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

BYTES_PER_FRAME = 2144 * 8 + 134 + 40

ap = argparse.ArgumentParser()
ap.add_argument("--bulk", action="store_true")
ap.add_argument("--live", action="store_true")
ap.add_argument("--reps", type=int, default=4)
ap.add_argument("--streams", type=int, default=0)
ap.add_argument("--frames", type=int, default=0)
a = ap.parse_args()
if a.bulk == a.live:
    ap.error("one of --bulk / --live")
amd = load()
o = Oracle()
rng = np.random.default_rng(7)
n_streams = a.streams or (512 if a.bulk else 64)
n_frames = a.frames or (1000 if a.bulk else 24)
log = S.cat(S.zeros(10), *[S.cat(S.sync(S.A), S.payload(o, k % 50, sigma=250.0, rng=rng)) for k in range(n_frames)], S.zeros(30))
d = amd.Demod(n_streams, max_samples=(n_frames + 8) * 2168 * 38, streaming=True)
d.enable_timing()


def med(v):
    return statistics.median(v), min(v), max(v)


def one_round(pieces):
    """pushes pieces[s] to stream s, then the timed round; returns (decoder bracket ms, round ms)"""
    for s, p in enumerate(pieces):
        d.push_soft(s, p)
    d.sync()
    t0 = time.perf_counter()
    d.process()
    d.sync()
    dt = (time.perf_counter() - t0) * 1e3
    return d.kernel_times()["frame_decode"], dt


res = {False: [], True: []}
errors = 0
if a.bulk:
    for rep in range(2 * (a.reps + 1)):
        on = rep % 2 == 1
        d.reset(-1)
        d.enable_link_report(on)
        dec, rnd = one_round([log] * n_streams)
        rel = [d.state(s).frames_released for s in (0, n_streams - 1)]
        assert rel == [n_frames, n_frames], rel
        if on:
            _, _, rec = d.pop_frames(0, link=True)
            assert len(rec) == n_frames and rec["valid"].all()
            errors = int(rec["bit_errors"].sum())
        if rep >= 2:
            res[on].append((dec, rnd))
        print(f"rep {rep} report {'on ' if on else 'off'}: decoder bracket {dec:8.3f} ms, round {rnd:8.3f} ms" + ("" if rep >= 2 else " (warm-up, left out)"), flush=True)
    frames_per_round = n_streams * n_frames
else:
    # one frame per stream and round: round r hands every stream the symbols up to the release of frame r
    cuts = [0] + [10 + 2168 * (k + 1) for k in range(n_frames)]
    for rep in range(2 * (a.reps + 1)):
        on = rep % 2 == 1
        d.reset(-1)
        d.enable_link_report(on)
        per = []
        for r in range(n_frames):
            per.append(one_round([log[cuts[r]:cuts[r + 1]]] * n_streams))
            for s in range(n_streams):
                got = d.pop_frames(s, link=True) if on else d.pop_frames(s)
                assert len(got[0]) == 1, (r, s, len(got[0]))
                if on:
                    errors += int(got[2]["bit_errors"].sum())
        per = per[4:]                                        # (the first rounds of a fresh context warm the launch paths)
        m = (statistics.median(p[0] for p in per), statistics.median(p[1] for p in per))
        if rep >= 2:
            res[on].append(m)
        print(f"rep {rep} report {'on ' if on else 'off'}: median of {len(per)} rounds: decoder bracket {m[0]:8.4f} ms, round {m[1]:8.4f} ms"
              + ("" if rep >= 2 else " (warm-up, left out)"), flush=True)
    frames_per_round = n_streams
d.close()
print(f"shape: {n_streams} streams x {n_frames if a.bulk else 1} frame(s) per round = {frames_per_round} frames, "
      f"{frames_per_round * BYTES_PER_FRAME / 1e6:.3f} MB for the link kernel; bit_errors seen {errors}")
for on in (False, True):
    dm, rm = med([x[0] for x in res[on]]), med([x[1] for x in res[on]])
    print(f"report {'on ' if on else 'off'}: decoder bracket median {dm[0]:.4f} ms (min {dm[1]:.4f}, max {dm[2]:.4f}); "
          f"round median {rm[0]:.4f} ms (min {rm[1]:.4f}, max {rm[2]:.4f}) over {len(res[on])} repetitions")
delta = statistics.median(x[1] for x in res[True]) - statistics.median(x[1] for x in res[False])
print(f"round on - off: {delta:.4f} ms" + (f" = {frames_per_round * BYTES_PER_FRAME / (delta * 1e-3) / 1e12:.2f} TB/s if all of it is the link kernel" if delta > 0 else ""))
