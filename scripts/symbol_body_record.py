"""Records what the one-stream-per-wave front end (csrc/k_frontend.hip) computes on a small fixed capture set, as sha256 digests:
per stream the soft-symbol log, the per-call chunk log {fo, tf, mu, leftover, nsym}, the final stream state (edge_ties included) and
the decoded frames. Run on the build whose results are to be kept (a GPU is needed):

    python scripts/symbol_body_record.py tests/golden/symbol_body_parent.json

tests/test_gpu_symbol_body.py imports this file and holds every later build to the recorded digests, bit for bit.

The set: soak_inputs.pathological_captures (8 captures of 3 chunks + 12 345 samples) and six workload.generate streams of 12 frames at
16 dB (global ids 0 and 63 carry f0 = -2000 and +2000 Hz, the AFC clamp). Three launch shapes:
  fp64    an 8-stream and a 6-stream context, k_msk_frontend_rb on the fp64 ring (128 threads)
  int16   the same two contexts with the create-time hook OPV_FRONTEND_INT16_RING (64 threads)
  wg4     516 streams x 3 frames, k_msk_frontend_rb_wg4: stream k carries the first opv_tx_modulated_samples(3) samples of capture
          k % 14; the 14 distinct digests are recorded, and every stream must reproduce its capture's
"""
import hashlib
import json
import os
import struct
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
WORKLOAD_IDS = (0, 63, 9, 27, 36, 54)
WORKLOAD_FRAMES, WORKLOAD_EBN0 = 12, 16.0
WG4_STREAMS, WG4_FRAMES = 516, 3


def capture_set(amd):
    """-> (names, [int16 IQ on the host]): 8 pathological + 6 workload captures"""
    import torch
    sys.path.insert(0, str(ROOT))
    sys.path.insert(0, str(ROOT / "tests"))
    from __graft_entry__ import load_pkg_module
    from soak_inputs import pathological_captures
    workload = load_pkg_module("workload")
    caps = [np.ascontiguousarray(c) for c in pathological_captures(amd.modulate(amd.bert_frames(10)))]
    names = [f"patho{k}" for k in range(len(caps))]
    dev = torch.device("cuda", 0)
    gen = amd.Demod(1, max_samples=1 << 16, streaming=True)
    try:
        d_iq, _tx, _n = workload.generate(amd, gen, torch, dev, list(WORKLOAD_IDS), WORKLOAD_FRAMES, WORKLOAD_EBN0)
        host = d_iq.cpu().numpy()
    finally:
        gen.close()
    caps += [np.ascontiguousarray(host[i]) for i in range(len(WORKLOAD_IDS))]
    names += [f"workload{g}" for g in WORKLOAD_IDS]
    return names, caps


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def digest(r):
    """one stream's record (a dict of Demod.receive) -> its digests; floats of the state by their bits"""
    st = r["state"]
    state = b"".join(struct.pack("<d", v) if isinstance(v, float) else struct.pack("<q", int(v)) for v in (getattr(st, f) for f, _ in st._fields_))
    return dict(soft=sha(r["soft"]), chunks=sha(r["chunks"]), state=hashlib.sha256(state).hexdigest(), frames=sha(r["frames"]),
                n_soft=int(len(r["soft"])), n_frames=int(len(r["frames"])), edge_ties=int(st.edge_ties))


def run_context(amd, caps, int16, kernel):
    """one context, one capture per stream, pushed whole (Demod.receive: rounds until nothing is stalled) -> [digest]"""
    if int16:
        os.environ["OPV_FRONTEND_INT16_RING"] = "1"
    else:
        os.environ.pop("OPV_FRONTEND_INT16_RING", None)
    try:
        d = amd.Demod(len(caps), max_samples=max(c.size // 2 for c in caps) + 64, streaming=True)
    finally:
        os.environ.pop("OPV_FRONTEND_INT16_RING", None)
    try:
        out = d.receive(caps)
        assert d.frontend_kernel() == kernel, d.frontend_kernel()
        return [digest(r) for r in out]
    finally:
        d.close()


def run_wg4(amd, caps):
    """516 streams x 3 frames -> the digests of the 14 distinct captures; every stream reproduces its capture's"""
    n3 = amd.lib().opv_tx_modulated_samples(WG4_FRAMES)
    cut = [c[: 2 * n3] for c in caps]
    got = run_context(amd, [cut[k % len(cut)] for k in range(WG4_STREAMS)], False, "k_msk_frontend_rb_wg4")
    for k, g in enumerate(got):
        assert g == got[k % len(cut)], f"stream {k} differs from stream {k % len(cut)} of the same capture"
    return got[: len(cut)]


def record_shape(amd, names, caps, shape):
    """the set on one launch shape ("fp64", "int16", "wg4") -> one digest per capture"""
    if shape == "wg4":
        return run_wg4(amd, caps)
    per = [None] * len(caps)
    for prefix in ("patho", "workload"):
        ks = [k for k, n in enumerate(names) if n.startswith(prefix)]
        for k, g in zip(ks, run_context(amd, [caps[k] for k in ks], shape == "int16", "k_msk_frontend_rb")):
            per[k] = g
    return per


def record(amd):
    names, caps = capture_set(amd)
    return {"names": names, "samples": [int(c.size // 2) for c in caps],
            "shapes": {shape: record_shape(amd, names, caps, shape) for shape in ("fp64", "int16", "wg4")}}


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    from __graft_entry__ import load_opv_amd
    amd = load_opv_amd()
    amd.lib()
    out = Path(sys.argv[1])
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record(amd), indent=1) + "\n")
    r = json.loads(out.read_text())
    print(f"{out}: {len(r['names'])} captures x {list(r['shapes'])}; frames per capture {[g['n_frames'] for g in r['shapes']['fp64']]}")
