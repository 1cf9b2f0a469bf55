"""What one push of the rational up-converter bank (opv_wbtx_push of an opv_wbtx_create_rational object: one k_wbtxr_duc launch and
one wait) costs, beside the integer bank's push (k_wbtx_duc) on the same channel counts. One push is one frame (86 720 input samples,
40 ms of signal) per channel:

  10 MS/s     1250 / 271, L = 73 986 (J = 60 taps per phase: the loopback plan of tests/test_gpu_wideband_tx_rational.py)  ->   400 000 wide samples
  61.44 MS/s  7680 / 271, L = 7680 x 16 (J = 16)                                                                           -> 2 457 600 wide samples
  integer     U = 4, L = 321 (81 taps of the longest phase: scripts/wideband_tx_cost.py's shape)                           ->   346 880 wide samples

for K = 64 and 256 channels. Figures, each the median of --reps pushes after one warm-up push: HIP events recorded on the context's
stream around the push (the upload of the K pointers and the kernel), and the host clock around the synchronous call beside them.
"per tap step" is the event time over wide samples x K x taps per phase: one multiply-add pair (I and Q) of one channel of one output.
Inputs are random int16 (seeded); all buffers are in device memory.

usage: wideband_tx_rational_cost.py [--reps 9]"""
import argparse
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
from __graft_entry__ import load_opv_amd  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=9)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: there is no other way to take these figures"
amd = load_opv_amd()

N_IN, WIDE_RATE, FRAME_MS = 86720, 2168000.0, 40.0


def sinc_taps(L, rate, gain):
    t = np.arange(L) - (L - 1) / 2
    h = np.sinc(2 * 200000.0 / rate * t) * np.hamming(L)
    return np.rint(h / h.sum() * gain * (1 << 15)).astype(np.int16)


SHAPES = [
    # name, down (the integer bank: interp), up, L, taps per phase
    ("10 MS/s     1250/271 J = 60", 1250, 271, 73986, 60),
    ("61.44 MS/s  7680/271 J = 16", 7680, 271, 7680 * 16, 16),
    ("integer     U = 4   L = 321", 4, 1, 321, 81),
]

g = torch.Generator(device="cpu").manual_seed(5)
for K in (64, 256):
    narrow = torch.randint(-32768, 32768, (K, 2 * N_IN), generator=g, dtype=torch.int16).cuda()
    ptrs = [narrow[k].data_ptr() for k in range(K)]
    d = amd.Demod(1, max_samples=1 << 16)
    stream = torch.cuda.ExternalStream(d.hip_stream())
    for name, M, U, L, J in SHAPES:
        n_out = -(-N_IN * M // U)
        taps = sinc_taps(L, M * WIDE_RATE, M)
        centres = list(np.linspace(-0.45, 0.45, K) * M * WIDE_RATE / U)
        out = torch.empty(2 * n_out, dtype=torch.int16, device="cuda")
        up = amd.WidebandTx(d, M, centres, taps, 40) if name.startswith("integer") else amd.WidebandTx.rational(d, M, U, centres, taps, 40)
        ev, host = [], []
        for r in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record(stream)
            up.push(ptrs, N_IN, out.data_ptr())
            e1.record(stream)
            e1.synchronize()
            t1 = time.perf_counter()
            if r:                                                         # (the first push is the warm-up)
                ev.append(e0.elapsed_time(e1))
                host.append((t1 - t0) * 1e3)
        assert up.samples() == (a.reps + 1) * N_IN
        up.close()
        m = statistics.median(ev)
        print(f"K = {K:3d}  {name}  {n_out:8d} wide samples   events median {m:8.3f} ms (min {min(ev):8.3f}, max {max(ev):8.3f})   "
              f"host clock median {statistics.median(host):8.3f} ms   {len(ev)} pushes after a warm-up   "
              f"{m * 1e12 / (n_out * K * J):7.1f} fs per tap step   {m / FRAME_MS * 100:5.1f} % of the frame's 40 ms", flush=True)
    d.close()
