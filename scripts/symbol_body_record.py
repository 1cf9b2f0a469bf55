"""Records what the front end (csrc/k_frontend.hip, k_frontend_x4.hip, k_frontend_x16.hip) computes on a small fixed capture set, as sha256 digests:
per stream the soft-symbol log, the per-call chunk log {fo, tf, mu, leftover, nsym}, the final stream state (edge_ties included) and
the decoded frames. Run on the build whose results are to be kept (a GPU is needed):

    python scripts/symbol_body_record.py tests/golden/symbol_body_parent.json

(shapes the file already holds are kept, not recorded again: delete the file first to record everything on a new parent)

tests/test_gpu_symbol_body.py imports this file and holds every later build to the recorded digests, bit for bit.

The set: soak_inputs.pathological_captures (8 captures of 3 chunks + 12 345 samples) and six workload.generate streams of 12 frames at
16 dB (global ids 0 and 63 carry f0 = -2000 and +2000 Hz, the AFC clamp). The launch shapes:
  fp64    an 8-stream and a 6-stream context, k_msk_frontend_rb on the fp64 ring (128 threads)
  int16   the same two contexts with the create-time hook OPV_FRONTEND_INT16_RING (64 threads)
  wg4     516 streams x 3 frames, k_msk_frontend_rb_wg4: stream k carries the first opv_tx_modulated_samples(3) samples of capture
          k % 14; the 14 distinct digests are recorded, and every stream must reproduce its capture's
  x4_wg4  one 14-stream context with set_frontend(4), k_msk_frontend_x4_wg4: one workgroup, two idle rows in its last wave
  x16     one 14-stream context with set_frontend(16), k_msk_frontend_x16: one wave with two idle quads
  x16_wg4 70 streams x 3 frames with set_frontend(16), k_msk_frontend_x16_wg4: two workgroups, the second with partly idle waves;
          stream k carries the 3-frame cut of capture k % 14 as in wg4
  x16_wg8 16 400 streams on the automatic choice, k_msk_frontend_x16_wg8, each ATTACHED to one of the 14 device-resident 3-frame
          cuts (no host push per stream); read back: the first and the last workgroup and every 64th stream (X16_WG8_READ)

A shape that is already in the output file is kept as it stands (byte for byte): only missing shapes are recorded.
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
SHAPES = ("fp64", "int16", "wg4", "x4_wg4", "x16", "x16_wg4", "x16_wg8")
# shape -> (opv_set_frontend argument, kernel) of the one-context shapes that carry the 14 captures whole
ROW_WHOLE = {"x4_wg4": (4, "k_msk_frontend_x4_wg4"), "x16": (16, "k_msk_frontend_x16")}
X16_WG4_STREAMS = 70
X16_WG8_STREAMS = 16400
X16_WG8_READ = sorted(set(range(128)) | set(range(X16_WG8_STREAMS // 128 * 128, X16_WG8_STREAMS)) | set(range(0, X16_WG8_STREAMS, 64)))


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


def run_context(amd, caps, int16, kernel, frontend=0):
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
        if frontend:
            d.set_frontend(frontend)
        out = d.receive(caps)
        assert d.frontend_kernel() == kernel, d.frontend_kernel()
        return [digest(r) for r in out]
    finally:
        d.close()


def cuts(amd, caps):
    n3 = amd.lib().opv_tx_modulated_samples(WG4_FRAMES)
    return [c[: 2 * n3] for c in caps]


def run_wg4(amd, caps, streams=WG4_STREAMS, kernel="k_msk_frontend_rb_wg4", frontend=0):
    """`streams` streams x 3 frames -> the digests of the 14 distinct captures; every stream reproduces its capture's"""
    cut = cuts(amd, caps)
    got = run_context(amd, [cut[k % len(cut)] for k in range(streams)], False, kernel, frontend)
    for k, g in enumerate(got):
        assert g == got[k % len(cut)], f"stream {k} differs from stream {k % len(cut)} of the same capture"
    return got[: len(cut)]


def run_attached(amd, caps, streams=X16_WG8_STREAMS, read=X16_WG8_READ, kernel="k_msk_frontend_x16_wg8"):
    """`streams` streams, stream k attached to the device-resident 3-frame cut of capture k % 14 (one upload of the 14 cuts, 256-byte
    aligned) -> the digests of the 14 distinct captures; every stream of `read` reproduces its capture's"""
    import torch
    cut = cuts(amd, caps)
    offs, total = [], 0
    for c in cut:
        offs.append(total)
        total += (c.size + 127) // 128 * 128 + 128            # int16 elements
    flat = np.zeros(total, np.int16)
    for o, c in zip(offs, cut):
        flat[o: o + c.size] = c
    d_flat = torch.from_numpy(flat).to(torch.device("cuda", 0))
    torch.cuda.synchronize()
    d = amd.Demod(streams, max_samples=max(c.size // 2 for c in cut) + 64, streaming=True)
    try:
        for k in range(streams):
            d.attach(k, d_flat.data_ptr() + 2 * offs[k % len(cut)], cut[k % len(cut)].size // 2, eof=True)
        d.process()
        d.sync()
        assert d.frontend_kernel() == kernel, d.frontend_kernel()
        got = {}
        for k in read:
            fr, _meta = d.pop_frames(k)
            st = d.state(k)
            assert st.stalled == 0, f"stream {k} stalled"
            got[k] = digest(dict(frames=fr, soft=d.soft(k), chunks=d.chunks(k), state=st))
        for k, g in got.items():
            assert g == got[k % len(cut)], f"stream {k} differs from stream {k % len(cut)} of the same capture"
        return [got[k] for k in range(len(cut))]
    finally:
        d.close()
        del d_flat


def record_shape(amd, names, caps, shape):
    """the set on one launch shape (SHAPES) -> one digest per capture"""
    if shape == "wg4":
        return run_wg4(amd, caps)
    if shape == "x16_wg4":
        return run_wg4(amd, caps, X16_WG4_STREAMS, "k_msk_frontend_x16_wg4", 16)
    if shape == "x16_wg8":
        return run_attached(amd, caps)
    if shape in ROW_WHOLE:
        return run_context(amd, caps, False, ROW_WHOLE[shape][1], ROW_WHOLE[shape][0])
    per = [None] * len(caps)
    for prefix in ("patho", "workload"):
        ks = [k for k, n in enumerate(names) if n.startswith(prefix)]
        for k, g in zip(ks, run_context(amd, [caps[k] for k in ks], shape == "int16", "k_msk_frontend_rb")):
            per[k] = g
    return per


def record(amd, kept=None):
    """every shape of SHAPES that `kept` (an earlier record of the same capture set) does not hold yet"""
    names, caps = capture_set(amd)
    head = {"names": names, "samples": [int(c.size // 2) for c in caps]}
    shapes = dict(kept["shapes"]) if kept else {}
    assert not kept or {k: kept[k] for k in head} == head, "the output file records another capture set"
    for shape in SHAPES:
        if shape not in shapes:
            shapes[shape] = record_shape(amd, names, caps, shape)
    return dict(head, shapes=shapes)


if __name__ == "__main__":
    sys.path.insert(0, str(ROOT))
    from __graft_entry__ import load_opv_amd
    amd = load_opv_amd()
    amd.lib()
    out = Path(sys.argv[1])
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(record(amd, json.loads(out.read_text()) if out.exists() else None), indent=1) + "\n")
    r = json.loads(out.read_text())
    print(f"{out}: {len(r['names'])} captures x {list(r['shapes'])}; frames per capture {[g['n_frames'] for g in r['shapes']['fp64']]}")
