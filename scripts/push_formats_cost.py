#!/usr/bin/env python3
"""What a typed push costs and buys (profiles/push_formats_cost.txt is this script's output; include/opv_demod.h, "typed IQ pushes").

  python3 scripts/push_formats_cost.py gather            the gather microbenchmark
  python3 scripts/push_formats_cost.py live [fmt ...]    the live capacity per format (default: cs16 cs8 cf32)

gather: ONE batch of 1536 pinned blocks of 86 720 samples (a serving round of 1536 streams), opv_push_iq_batch (k_push_gather,
int16) against opv_push_iq_batch_fmt in cs8, cu8 and cf32 (k_push_convert): the median over 12 timed batches after 3 of warm-up of
the host's time around the call, which returns when the blocks have landed. Two sets of blocks alternate, so that no batch reads
what the batch before it read; the streams are reset between batches (untimed).

live: bin/opv-live-capacity at bench.py's criterion (extras.live_capacity: the largest N on a grid of 256 whose p99 round stays
under 40 ms with every frame right, found by bench.py's secant search), serial and pipelined, for the int16 calls and with
--format cs8 / cf32."""
import ctypes as C
import json
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
CHUNK = 86720


def gather():
    import torch
    from __graft_entry__ import load_opv_amd
    amd = load_opv_amd()
    L = amd.lib()
    S, timed, warm = 1536, 12, 3
    rng = np.random.default_rng(1)
    d = amd.Demod(S, max_samples=CHUNK + 64, streaming=True)
    ids = (C.c_int * S)(*range(S))
    lens = (C.c_size_t * S)(*([CHUNK] * S))
    print(f"gather microbenchmark: one batch of {S} pinned blocks of {CHUNK} samples, median of {timed} batches after {warm} of warm-up")
    print(f"{'format':<6} {'call':<26} {'ms':>8} {'GB/s over the link':>20} {'Msamples/s':>12}")
    try:
        for fmt, (code, dtype) in amd.IQ_FORMATS.items():
            per = 2 * np.dtype(dtype).itemsize
            pools, tables = [], []
            for _ in range(2):
                t = torch.empty(S * CHUNK * per, dtype=torch.uint8).pin_memory()
                a = t.numpy()
                pat = rng.uniform(-1, 1, 1 << 18).astype(np.float32).view(np.uint8) if fmt == "cf32" else rng.integers(0, 256, 1 << 20, dtype=np.uint8)
                for i in range(0, a.size, pat.size):       # (a link does not care what the bytes are)
                    a[i: i + pat.size] = pat[: a.size - i]
                pools.append(t)
                tables.append((C.c_void_p * S)(*[a.ctypes.data + k * CHUNK * per for k in range(S)]))
            ms = []
            for b in range(warm + timed):
                d.reset()
                d.sync()
                t0 = time.perf_counter()
                rc = L.opv_push_iq_batch(d.h, S, ids, tables[b % 2], lens) if fmt == "cs16" else L.opv_push_iq_batch_fmt(d.h, code, S, ids, tables[b % 2], lens)
                t1 = time.perf_counter()
                assert rc == 0, L.opv_last_error()
                if b >= warm:
                    ms.append((t1 - t0) * 1e3)
            m = float(np.median(ms))
            call = "opv_push_iq_batch" if fmt == "cs16" else "opv_push_iq_batch_fmt"
            print(f"{fmt:<6} {call:<26} {m:8.3f} {S * CHUNK * per / m / 1e6:20.2f} {S * CHUNK / m / 1e3:12.1f}   (min {min(ms):.3f}, max {max(ms):.3f} ms)")
            del pools, tables
    finally:
        d.close()


def live(formats):
    exe = ROOT / "opv-cxx-demod_amd" / "bin" / "opv-live-capacity"
    rounds = 60

    def probe(n, pipelined, fmt):
        cmd = [str(exe), str(n), str(rounds), "6", "0"] + (["--pipelined"] if pipelined else []) + ([] if fmt == "cs16" else ["--format", fmt])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=150)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        r = json.loads(line[-1]) if p.returncode == 0 and line else {"streams": n, "error": (p.stderr or p.stdout)[-200:], "rc": p.returncode}
        print("  $ " + " ".join(["bin/opv-live-capacity"] + cmd[1:]))
        print("    " + json.dumps(r), flush=True)
        return r

    def secant(start, pipelined, fmt, grid=256, most=4):      # bench.py's search (live_capacity)
        lo, hi, n, seen = 0, None, start, {}
        for _ in range(most):
            r = seen[n] = probe(n, pipelined, fmt)
            if "error" in r:
                break
            ok = r["round_ms_p99"] < 40.0 and r["frames_wrong"] == 0
            if ok:
                lo = max(lo, n)
            else:
                hi = n if hi is None else min(hi, n)
            if hi is not None and hi - lo <= grid:
                break
            p99 = r["round_ms_p99"]
            nxt = int(n * 40.0 / p99 * (0.985 if ok else 1.0)) // grid * grid
            nxt = max(nxt, lo + grid)
            if hi is not None:
                nxt = min(nxt, hi - grid)
            if nxt <= lo or nxt > 16384 or nxt in seen:
                break
            n = nxt
        return lo, hi, seen.get(lo)

    print(f"live capacity: bin/opv-live-capacity, {rounds} rounds per probe, the largest N (grid 256) with p99 round < 40 ms and no wrong frame")
    rows = []
    for fmt in formats:
        start = {"cs16": 5120, "cs8": 8192, "cu8": 8192, "cf32": 2816}[fmt]
        lo, hi, best = secant(start, False, fmt)
        plo, phi, pbest = secant(max(lo, 256) + 512, True, fmt)
        rows.append((fmt, lo, hi, best, plo, phi, pbest))
    print(f"{'format':<6} {'serial N':>9} {'p99 ms':>8} {'first N over':>13} {'pipelined N':>12} {'p99 ms':>8} {'first N over':>13} {'GB/s at N (pipelined)':>22}")
    for fmt, lo, hi, best, plo, phi, pbest in rows:
        print(f"{fmt:<6} {lo:9d} {best['round_ms_p99'] if best else float('nan'):8.2f} {str(hi):>13} {plo:12d} "
              f"{pbest['round_ms_p99'] if pbest else float('nan'):8.2f} {str(phi):>13} {pbest['pcie_GBps_p50'] if pbest else float('nan'):22.2f}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "gather":
        gather()
    elif len(sys.argv) > 1 and sys.argv[1] == "live":
        live(sys.argv[2:] or ["cs16", "cs8", "cf32"])
    else:
        sys.exit(__doc__)
