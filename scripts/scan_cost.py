"""What one push of the wideband scan (opv_scan_push_device: one k_scan_probe launch, one k_scan_reduce, one wait) costs for 40 ms
of signal, at the two ends of the doors' wide rates and the two ends of the fast range of P:

  D = 4        8.672 MS/s (down / up = 4 / 1)        346 880 wide samples
  61.44 MS/s   down / up = 7680 / 271              2 457 600 wide samples
  P = 256 and 1024 probes across the wide rate, a 1024-tap integer Hann window, hop 1024 and 512,
  A = all segments of the push where a block's span (A - 1) H + Lw fits the 2^20 limit (D = 4: one block), else the push's segments
  in the fewest equal blocks (61.44 MS/s: three), whose rows a caller adds

Figures: the median of --reps timed repetitions after one warm-up, host clock (time.perf_counter) around opv_scan_push_device,
which returns when the device has read the block - the object's launches go to the context's own copy stream, which no event of
the caller's reaches (as scripts/wideband_rational_cost.py). The object is reset before every push (outside the clock), so every
push does the same work. The kernels' own durations come from a second run of the same command under the profiler, and --trace
turns its per-dispatch table into the same rows:

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 scripts/scan_cost.py --reps 5
  python3 scripts/scan_cost.py --reps 5 --trace OUT/.../*_kernel_trace.csv

Each row also gives the multiple of real time (the signal's own 40 ms over the figure) and the ratio to the DDC bank's push of
the same D = 4 capture for 64 channels as recorded in profiles/wideband_tx_cost.txt (opv_wb_push_device, k_wb_ddc: 1.24 ms).
Work per push, from the shapes: segments x Lw x P lane-steps of one LDS gather and four 32 x 32 + 64-bit multiply-adds each.
Inputs are random int16 (seeded); out_shift 22.

usage: scan_cost.py [--reps 5] [--trace kernel_trace.csv]"""
import argparse
import csv
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", default=None)
a = ap.parse_args()

N_OUT, WIDE_RATE, LW, SIGNAL_MS, DDC_64_MS = 86720, 2168000.0, 1024, 40.0, 1.24
RATES = [("D = 4      ", 4, 1), ("61.44 MS/s ", 7680, 271)]
SHAPES = [(name, M, U, P, H) for name, M, U in RATES for P in (256, 1024) for H in (1024, 512)]


def blocks_of(n_wide, H):
    """(A, blocks): every segment of the push in the fewest equal blocks whose span fits 2^20"""
    segs = (n_wide - LW) // H + 1
    a_max = ((1 << 20) - LW) // H + 1
    nb = -(-segs // a_max)
    return segs // nb, nb


def row(name, P, H, A, nb, v):
    m = statistics.median(v)
    print(f"{name} P = {P:4d}  H = {H:4d}  A = {A:4d} x {nb} block(s)   median {m:7.3f} ms  (min {min(v):7.3f}, max {max(v):7.3f}, {len(v)} repetitions after a warm-up)"
          f"   {SIGNAL_MS / m:6.1f} x real time   {m / DDC_64_MS:5.2f} of the 64-channel DDC push", flush=True)
    return m


if a.trace:
    # the profiler's dispatches of k_scan_probe, in launch order: per shape one warm-up and --reps timed ones (k_scan_reduce beside it)
    rows = [r for r in csv.DictReader(open(a.trace)) if r["Kernel_Name"].startswith(("k_scan_probe", "k_scan_reduce"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = {k: [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6 for r in rows if r["Kernel_Name"].startswith(k)] for k in ("k_scan_probe", "k_scan_reduce")}
    assert len(ms["k_scan_probe"]) == len(ms["k_scan_reduce"]) == len(SHAPES) * (a.reps + 1), (len(ms["k_scan_probe"]), a.reps)
    for k in ("k_scan_probe", "k_scan_reduce"):
        print(f"{k}: durations from the profiler's trace (ms):")
        for i, (name, M, U, P, H) in enumerate(SHAPES):
            A, nb = blocks_of(N_OUT * M // U, H)
            row(name, P, H, A, nb, ms[k][i * (a.reps + 1) + 1: (i + 1) * (a.reps + 1)])
    sys.exit(0)

import torch  # noqa: E402

from __graft_entry__ import load_opv_amd  # noqa: E402
from scan_model import hann_window  # noqa: E402

assert torch.cuda.is_available(), "needs the GPU: there is no other way to take these figures"
amd = load_opv_amd()
g = torch.Generator(device="cpu").manual_seed(5)
window = hann_window(LW)
print("host clock around opv_scan_push_device (ms):")
for name, M, U, P, H in SHAPES:
    fw = M * WIDE_RATE / U
    n_wide = N_OUT * M // U
    A, nb = blocks_of(n_wide, H)
    wide = torch.randint(-32768, 32768, (2 * n_wide,), generator=g, dtype=torch.int16).cuda()
    d = amd.Demod(1, max_samples=1 << 16, streaming=True)
    sc = amd.Scan(d, M, U, -fw / 2 + fw / P * np.arange(P), window, H, A, 22, ring_blocks=nb)
    assert amd.scan_blocks(LW, H, A, n_wide, M, U) == nb
    out = []
    for rep in range(a.reps + 1):
        sc.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        sc.push_device(wide.data_ptr(), n_wide)
        dt = (time.perf_counter() - t0) * 1e3
        if rep:
            out.append(dt)
    rows, _ = sc.pop()
    assert len(rows) == nb and rows.min() > 0
    row(name, P, H, A, nb, out)
    sc.close()
    d.close()
    del wide
