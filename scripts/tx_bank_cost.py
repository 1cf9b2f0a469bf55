"""What a round of the transmit bank (opv_txb_round: k_txb_encode, k_txb_scan, k_txb_phases, k_txb_modulate, one wait) costs,
against what a caller had before it. Figures, each the median of --reps timed repetitions after one warm-up, host clock
(time.perf_counter) around a synchronous call - every one of these calls ends in a device synchronise:

  bank 1000x1   one round of 1000 streams x 1 frame   (1000 frames: 346.9 MB of samples written)
  bank 64x16    one round of   64 streams x 16 frames (1024 frames: 355.2 MB)
  (a)           opv_tx_modulate_device on ONE run of 1000 frames: the same bytes written, the same sincos count, but its
                symbol-start phases expanded once per context (the warm-up pays that) where a round replays them every time
  (b)           a loop of 1000 one-frame opv_tx_modulate_device calls: what a caller with 1000 channels had to do (and each
                call restarts its run: a silent symbol 0, a reset sign)

(a) and (b) need nothing of the bank, so `--lib PATH` measures them on any build of the library - the parent commit's for the
record in profiles/tx_bank_cost.txt; the bank's figures are left out when the library has no opv_txb_round. The streams of a
bank keep their state from repetition to repetition (a live bank is not reset): repetition r modulates frame r of every run.
The kernels' own durations come from a separate run of the same command under the profiler:

  rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python3 scripts/tx_bank_cost.py --only bank --reps 3

usage: tx_bank_cost.py [--lib PATH] [--reps 5] [--only bank|calls]"""
import argparse
import ctypes as C
import statistics
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parents[1]
FB, FSAMP = 134, 86720

ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=str(ROOT / "opv-cxx-demod_amd" / "libopv_demod_hip.so"))
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--only", choices=("bank", "calls"), default=None)
a = ap.parse_args()
assert a.reps >= 5 or a.only == "bank", "medians of at least 5"
assert torch.cuda.is_available(), "needs the GPU: there is no other way to take these figures"


class Cfg(C.Structure):
    _fields_ = [("streaming", C.c_int32), ("have_init_offset", C.c_int32), ("init_offset_hz", C.c_double), ("afc_alpha", C.c_double),
                ("device", C.c_int32), ("coherent", C.c_int32), ("max_samples", C.c_uint64), ("pll_bw_hz", C.c_double)]


L = C.CDLL(a.lib)
L.opv_last_error.restype = C.c_char_p
L.opv_create.argtypes = [C.POINTER(C.c_void_p), C.c_int, C.POINTER(Cfg)]
L.opv_destroy.argtypes = [C.c_void_p]
L.opv_destroy.restype = None
L.opv_tx_bert_frames.restype = None
L.opv_tx_bert_frames.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_void_p]
L.opv_tx_modulate_device.restype = C.c_long
L.opv_tx_modulate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
have_bank = hasattr(L, "opv_txb_round")
if have_bank:
    L.opv_txb_create.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.c_int]
    L.opv_txb_destroy.argtypes = [C.c_void_p]
    L.opv_txb_destroy.restype = None
    L.opv_txb_round.restype = C.c_long
    L.opv_txb_round.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]


def chk(rc):
    assert rc >= 0, (rc, L.opv_last_error())
    return rc


def bert(n, k=0, first=0):
    out = np.zeros((n, FB), np.uint8)
    L.opv_tx_bert_frames(f"COST{k}".encode(), 0xC05700 + k, first, n, out.ctypes.data)
    return out


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


def line(name, v):
    print(f"{name:<14s} median {statistics.median(v):9.3f} ms   (min {min(v):9.3f}, max {max(v):9.3f}, {len(v)} repetitions after a warm-up)", flush=True)
    return statistics.median(v)


ctx = C.c_void_p()
cfg = Cfg(1, 0, 0.0, 0.001, 0, 0, 1 << 16, 50.0)
chk(L.opv_create(C.byref(ctx), 1, C.byref(cfg)))
out = torch.empty(2 * (1024 * FSAMP + 4000), dtype=torch.int16, device="cuda")      # every figure writes into the same 355 MB
print(f"library: {a.lib}{'' if have_bank else '   (no transmit bank in this build: (a) and (b) only)'}")
res = {}
if a.only != "bank":
    run = bert(1000)
    res["a"] = line("(a) 1 x 1000", timed(lambda r: chk(L.opv_tx_modulate_device(ctx, run.ctypes.data, 1000, out.data_ptr())), a.reps))

    def loop(r):
        for k in range(1000):                     # (each call writes a frame + the 4000-sample tail of its run: the next one overwrites the tail)
            chk(L.opv_tx_modulate_device(ctx, run[k:].ctypes.data, 1, out.data_ptr() + 4 * FSAMP * k))
    res["b"] = line("(b) 1000 x 1", timed(loop, a.reps))
if have_bank and a.only != "calls":
    for name, n_streams, per in (("bank 1000x1", 1000, 1), ("bank 64x16", 64, 16)):
        bank = C.c_void_p()
        chk(L.opv_txb_create(C.byref(bank), ctx, n_streams))
        frames = [bert(per * (a.reps + 1), k) for k in range(n_streams)]
        ids = (C.c_int * n_streams)(*range(n_streams))
        nf = (C.c_size_t * n_streams)(*[per] * n_streams)
        op = (C.c_void_p * n_streams)(*[out.data_ptr() + 4 * FSAMP * per * k for k in range(n_streams)])

        fps = [(C.c_void_p * n_streams)(*[f[per * (r + 1):].ctypes.data for f in frames]) for r in range(-1, a.reps)]   # (not in the timed part)

        def one(r):
            assert chk(L.opv_txb_round(bank, n_streams, ids, fps[r + 1], nf, op, 0)) == 0
        res[name] = line(name, timed(one, a.reps))
        L.opv_txb_destroy(bank)
L.opv_destroy(ctx)
if "a" in res:
    for name in ("bank 1000x1", "bank 64x16"):
        if name in res:
            print(f"{name}: {res[name] / res['a']:.2f} x (a), {res['b'] / res[name]:.1f} x faster than (b)")
