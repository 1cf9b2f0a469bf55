"""What one push of the rational wideband front door (opv_wb_create_rational: one k_wbr_ddc launch and one wait) costs, beside the
integer door's push (opv_wb_create: k_wb_ddc) at nearly the same wide rate. Every push makes one
frame of output per channel (86 720 samples = 40 ms of signal), for K = 64 and 256 channels:

  30.72 MS/s  down / up = 3840 / 271, J = 23 taps per phase (L = 6233)   1 228 800 wide samples
  61.44 MS/s  down / up = 7680 / 271, J = 46 taps per phase (L = 12466)  2 457 600 wide samples
  yardstick   decim = 14 (30.352 MS/s), L = 322                          1 214 080 wide samples, k_wb_ddc
  equal work  decim = 14, L = 23                                         the same, k_wb_ddc

The yardstick is a filter of the same length in TIME as the 30.72 MS/s row (23 wide samples of the prototype per phase against 322
wide samples at nearly the same rate), but a decimator weighs every one of its L taps into every output: 322 int64 multiply-adds
per output and component, where the rational door's output weighs only its phase's J = 23 (46). The fourth row is k_wb_ddc at
the same multiply-adds per output as the 30.72 MS/s row.

Figures: the median of --reps timed repetitions after one warm-up, host clock (time.perf_counter) around opv_wb_push_device, which
returns when the device has read the block - the object's launches go to the context's own copy stream, which no event of the
caller's reaches. The kernels' own durations come from a second run of the same command under the profiler, and --trace turns its
per-dispatch table into the same rows:

  rocprofv3 --kernel-trace --output-format csv -d OUT -- python3 scripts/wideband_rational_cost.py --reps 5
  python3 scripts/wideband_rational_cost.py --reps 5 --trace OUT/.../*_kernel_trace.csv

Inputs are random int16 (seeded); the taps are Hamming-windowed sincs with a 200 kHz cut-off, every phase's sum 2^15, out_shift 30.

usage: wideband_rational_cost.py [--reps 5] [--trace kernel_trace.csv]"""
import argparse
import csv
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", default=None)
a = ap.parse_args()

N_OUT, WIDE_RATE = 86720, 2168000.0
SHAPES = [("30.72 MS/s  3840/271 J=23", "r", 3840, 271, 23), ("61.44 MS/s  7680/271 J=46", "r", 7680, 271, 46), ("yardstick   D=14 L=322    ", "i", 14, 1, 322),
          ("equal work  D=14 L=23     ", "i", 14, 1, 23)]
KS = (64, 256)


def summary(name, K, v):
    m = statistics.median(v)
    print(f"{name}  K = {K:3d}   median {m:8.3f} ms   (min {min(v):8.3f}, max {max(v):8.3f}, {len(v)} repetitions after a warm-up)", flush=True)
    return m


def ratios(res):
    for K in KS:
        for name, *_ in SHAPES[:2]:
            print(f"K = {K:3d}: {name.strip()} / yardstick = {res[name, K] / res[SHAPES[2][0], K]:.2f}, / equal work = {res[name, K] / res[SHAPES[3][0], K]:.2f}")
    worst = res[SHAPES[1][0], 256]
    print(f"61.44 MS/s, 256 channels: {worst:.3f} ms for 40 ms of signal ({40.0 / worst:.1f} x real time)")


if a.trace:
    # the profiler's dispatches of the two kernels, in launch order: per K, per shape, one warm-up and --reps timed ones
    rows = [r for r in csv.DictReader(open(a.trace)) if r["Kernel_Name"].startswith(("k_wbr_ddc", "k_wb_ddc"))]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    ms = [(r["Kernel_Name"].split("(")[0], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6) for r in rows]
    assert len(ms) == len(KS) * len(SHAPES) * (a.reps + 1), (len(ms), a.reps)
    print("kernel durations from the profiler's trace (ms):")
    res, at = {}, 0
    for K in KS:
        for name, kind, *_ in SHAPES:
            part = ms[at: at + a.reps + 1]
            at += a.reps + 1
            assert {n for n, _ in part} == {"k_wbr_ddc" if kind == "r" else "k_wb_ddc"}, part
            res[name, K] = summary(name, K, [t for _, t in part[1:]])
    ratios(res)
    sys.exit(0)

import torch  # noqa: E402

from __graft_entry__ import load_opv_amd  # noqa: E402

assert torch.cuda.is_available(), "needs the GPU: there is no other way to take these figures"
amd = load_opv_amd()


def sinc_taps(L, fs, gain):
    t = np.arange(L) - (L - 1) / 2
    h = np.sinc(2 * 200000.0 / fs * t) * np.hamming(L)
    return np.rint(h / h.sum() * gain * (1 << 15)).astype(np.int16)


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


g = torch.Generator(device="cpu").manual_seed(5)
res = {}
print("host clock around opv_wb_push_device (ms):")
for K in KS:
    for name, kind, M, U, J in SHAPES:
        fw = M * WIDE_RATE / U
        centres = list(np.linspace(-0.45, 0.45, K) * fw)
        n_wide = N_OUT * M // U
        wide = torch.randint(-32768, 32768, (2 * n_wide,), generator=g, dtype=torch.int16).cuda()
        d = amd.Demod(K, max_samples=N_OUT * (a.reps + 2), streaming=True)
        if kind == "r":
            assert amd.wbr_outputs(M, U, n_wide) == N_OUT
            wb = amd.Wideband.rational(d, M, U, list(range(K)), centres, sinc_taps(J * U, U * fw, U), 30)
        else:
            wb = amd.Wideband(d, M, list(range(K)), centres, sinc_taps(J, fw, 1), 30)
        res[name, K] = summary(name, K, timed(lambda: wb.push_device(wide.data_ptr(), n_wide), a.reps))
        wb.close()
        d.close()
        del wide
ratios(res)
