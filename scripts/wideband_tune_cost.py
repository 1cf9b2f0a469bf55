"""What an LO schedule costs (opv_wb_retune / opv_wbtx_retune: the scheduled kernels k_wb_ddc_tuned, k_wbr_ddc_tuned,
k_wbtx_duc_tuned, k_wbtxr_duc_tuned) beside the unscheduled kernels on the same input, on the README's shapes. One push is one frame
per channel (86 720 samples at 2.168 MS/s, 40 ms of signal), for K = 64 and 256 channels:

  door   D = 4, L = 321                          346 880 wide samples in   k_wb_ddc    / k_wb_ddc_tuned
  door   61.44 MS/s 7680 / 271, J = 46         2 457 600 wide samples in   k_wbr_ddc   / k_wbr_ddc_tuned
  up     U = 4, L = 321                          346 880 wide samples out  k_wbtx_duc  / k_wbtx_duc_tuned
  up     61.44 MS/s 7680 / 271, J = 16         2 457 600 wide samples out  k_wbtxr_duc / k_wbtxr_duc_tuned

Per shape two objects are made on the same input, one never retuned and one with EVERY channel on a ramp from its first sample, and
their pushes alternate in one process after a warm-up push of each. Figures are the median of --reps pushes:
  up-converters: HIP events recorded on the context's stream around the push (the uploads and the kernel);
  doors: the host clock around opv_wb_push_device, which returns when the device has read the block - the door launches on the
    context's own copy stream, which no event of the caller's reaches. The host's share (the call, building K schedule tables) is
    inside the figure, for both objects.

--plain-only times the unscheduled object alone, and --tree PATH loads the package of another checkout (the parent commit's, which
has no schedule): alternating the two trees in one visit shows whether the unscheduled kernels cost what they cost before.

usage: wideband_tune_cost.py [--reps 7] [--plain-only] [--tree PATH]"""
import argparse
import importlib.util
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--plain-only", action="store_true")
ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[1]))
a = ap.parse_args()
assert torch.cuda.is_available(), "needs the GPU: there is no other way to take these figures"
spec = importlib.util.spec_from_file_location("opv_amd", Path(a.tree) / "opv-cxx-demod_amd" / "opv_amd.py")
amd = importlib.util.module_from_spec(spec)
sys.modules["opv_amd"] = amd
spec.loader.exec_module(amd)

N, WIDE_RATE = 86720, 2168000.0


def sinc_taps(L, fs, gain):
    t = np.arange(L) - (L - 1) / 2
    h = np.sinc(2 * 200000.0 / fs * t) * np.hamming(L)
    return np.rint(h / h.sum() * gain * (1 << 15)).astype(np.int16)


def ramps(K):
    """every channel on a ramp from the object's first sample: a few hundred kHz/s, both signs"""
    return [(k, 0, 0.0, (1 if k % 2 else -1) * 1.0e5 * (1 + k % 7)) for k in range(K)]


def report(name, K, plain, tuned):
    p = statistics.median(plain)
    line = f"K = {K:3d}  {name}  unscheduled median {p:7.3f} ms (min {min(plain):7.3f}, max {max(plain):7.3f})"
    if tuned:
        t = statistics.median(tuned)
        line += f"   scheduled median {t:7.3f} ms (min {min(tuned):7.3f}, max {max(tuned):7.3f})   scheduled / unscheduled = {t / p:5.3f}"
    print(line + f"   {len(plain)} pushes each after a warm-up", flush=True)


g = torch.Generator(device="cpu").manual_seed(5)
DOORS = [("door  D = 4  L = 321           ", 4, 1, 321), ("door  61.44 MS/s 7680/271 J = 46", 7680, 271, 46)]
UPS = [("up    U = 4  L = 321           ", 4, 1, 321), ("up    61.44 MS/s 7680/271 J = 16", 7680, 271, 16)]
for K in (64, 256):
    # ---- the doors: host clock around the synchronous push
    for name, M, U, J in DOORS:
        fw = M * WIDE_RATE / U
        centres = list(np.linspace(-0.45, 0.45, K) * fw)
        n_wide = N * M // U
        wide = torch.randint(-32768, 32768, (2 * n_wide,), generator=g, dtype=torch.int16).cuda()
        objs = []
        for tuned in (False, True)[: 1 if a.plain_only else 2]:
            d = amd.Demod(K, max_samples=N * (a.reps + 2), streaming=True)
            if U == 1:
                wb = amd.Wideband(d, M, list(range(K)), centres, sinc_taps(J, fw, 1), 30)
            else:
                wb = amd.Wideband.rational(d, M, U, list(range(K)), centres, sinc_taps(J * U, U * fw, U), 30)
            if tuned:
                wb.retune([(k, at, centres[k], r) for k, at, _, r in ramps(K)])
            objs.append((d, wb, []))
        for r in range(a.reps + 1):
            for d, wb, ms in objs:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                wb.push_device(wide.data_ptr(), n_wide)
                t1 = time.perf_counter()
                if r:
                    ms.append((t1 - t0) * 1e3)
        report(name, K, objs[0][2], objs[1][2] if len(objs) > 1 else None)
        for d, wb, _ in objs:
            wb.close()
            d.close()
    # ---- the up-converters: events on the context's stream
    narrow = torch.randint(-32768, 32768, (K, 2 * N), generator=g, dtype=torch.int16).cuda()
    ptrs = [narrow[k].data_ptr() for k in range(K)]
    d = amd.Demod(1, max_samples=1 << 16)
    stream = torch.cuda.ExternalStream(d.hip_stream())
    for name, M, U, J in UPS:
        n_out = -(-N * M // U)
        centres = list(np.linspace(-0.45, 0.45, K) * M * WIDE_RATE / U)
        taps = sinc_taps(J if U == 1 else J * M, M * WIDE_RATE, M)
        out = torch.empty(2 * n_out, dtype=torch.int16, device="cuda")
        objs = []
        for tuned in (False, True)[: 1 if a.plain_only else 2]:
            up = amd.WidebandTx(d, M, centres, taps, 40) if U == 1 else amd.WidebandTx.rational(d, M, U, centres, taps, 40)
            if tuned:
                up.retune([(k, at, centres[k], r) for k, at, _, r in ramps(K)])
            objs.append((up, []))
        for r in range(a.reps + 1):
            for up, ms in objs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(stream)
                up.push(ptrs, N, out.data_ptr())
                e1.record(stream)
                e1.synchronize()
                if r:
                    ms.append(e0.elapsed_time(e1))
        report(name, K, objs[0][1], objs[1][1] if len(objs) > 1 else None)
        for up, _ in objs:
            up.close()
    d.close()
