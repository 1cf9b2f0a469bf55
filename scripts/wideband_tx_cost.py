"""What one push of the wideband transmit bank (opv_wbtx_push: one k_wbtx_duc launch and one wait) costs, beside the DDC bank's
push of the mirror-image shape (opv_wb_push_device: one k_wb_ddc launch and one wait). Figures, each the median of --reps timed
repetitions after one warm-up, host clock (time.perf_counter) around a synchronous call - both calls end in a device synchronise:

  up   K = 64 / 256 channels x 86 720 input samples (one frame each), U = 4, L = 321  ->  346 880 wide samples
  down the same 346 880 wide samples, D = 4, K = 64 / 256, L = 321                    ->  86 720 samples per stream

Inputs are random int16 (seeded), the taps the 321-tap Hamming sinc of tests/wideband_device.py (PLAN_D4). The HBM bytes each direction
has to move are printed beside the times: 4 K n_in read + 4 n_in U written going up, 4 n_in U read + 4 K n_in written coming down.
The kernels' own durations come from a separate run of the same command under the profiler:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 scripts/wideband_tx_cost.py --reps 3

usage: wideband_tx_cost.py [--reps 5]"""
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
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: there is no other way to take these figures"
amd = load_opv_amd()

N_IN, U, L, WIDE_RATE = 86720, 4, 321, 2168000.0
t = np.arange(L) - (L - 1) / 2
h = np.sinc(2 * 200000.0 / (U * WIDE_RATE) * t) * np.hamming(L)
taps_up = np.rint(h / h.sum() * 4 * (1 << 15)).astype(np.int16)
taps_down = np.rint(h / h.sum() * (1 << 15)).astype(np.int16)


def timed(fn, reps):
    """ms of each of `reps` calls after one warm-up call"""
    fn(-1)
    torch.cuda.synchronize()
    out = []
    for r in range(reps):
        t0 = time.perf_counter()
        fn(r)
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def line(name, v, nbytes):
    m = statistics.median(v)
    print(f"{name:<22s} median {m:8.3f} ms   (min {min(v):8.3f}, max {max(v):8.3f}, {len(v)} repetitions after a warm-up)   "
          f"{nbytes / 1e6:7.1f} MB to move: {nbytes / m / 1e6:7.1f} GB/s", flush=True)
    return m


g = torch.Generator(device="cpu").manual_seed(5)
res = {}
for K in (64, 256):
    centres = list(np.linspace(-0.45, 0.45, K) * U * WIDE_RATE)
    nbytes = 4 * K * N_IN + 4 * N_IN * U
    narrow = torch.randint(-32768, 32768, (K, 2 * N_IN), generator=g, dtype=torch.int16).cuda()
    wide = torch.randint(-32768, 32768, (2 * N_IN * U,), generator=g, dtype=torch.int16).cuda()
    out = torch.empty(2 * N_IN * U, dtype=torch.int16, device="cuda")
    d = amd.Demod(K, max_samples=N_IN * (a.reps + 2), streaming=True)
    up = amd.WidebandTx(d, U, centres, taps_up, 40)
    ptrs = [narrow[k].data_ptr() for k in range(K)]
    res["up", K] = line(f"up   K = {K:3d} (wbtx)", timed(lambda r: up.push(ptrs, N_IN, out.data_ptr()), a.reps), nbytes)
    up.close()
    down = amd.Wideband(d, U, list(range(K)), centres, taps_down, 30)
    res["down", K] = line(f"down K = {K:3d} (wb)", timed(lambda r: down.push_device(wide.data_ptr(), N_IN * U), a.reps), nbytes)
    down.close()
    d.close()
    print(f"K = {K}: up / down = {res['up', K] / res['down', K]:.2f}")
