"""dev, CPU only: where in a run does 16383 * sin / cos of an NCO phase land so close to a non-zero integer that a transmit
bank's round lists the sample as ambiguous (k_tx_common.h: within 1e-9, not on it, not a flat top)? The phases are
data-independent, so the positions are a property of (symbol, sample, tone, component) alone. Lists those whose distance lies in
[1e-11, 5e-10] with |v| <= 16382.5 - numpy over tests/tx_bank_model.py's symbol_phases, each hit re-confirmed with math.sin /
math.cos - and per block of frames the smallest distance seen. usage: tx_find_ambiguous.py [FIRST_FRAME [LAST_FRAME]]"""
import math, sys, time, numpy as np
from pathlib import Path
ROOT = Path(__file__).resolve().parents[2]
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
from __graft_entry__ import load_opv_amd
import tx_bank_model as M
amd = load_opv_amd()
LO, HI, TOP, STEP = 1e-11, 5e-10, 16382.5, 128
first = int(sys.argv[1]) if len(sys.argv) > 1 else 0
last = int(sys.argv[2]) if len(sys.argv) > 2 else 4096
hits, t0 = [], time.time()
for f0 in range(first, last, STEP):
    n = (min(f0 + STEP, last) - f0) * M.FSYMS
    p = M.symbol_phases(amd, f0 * M.FSYMS, n).copy()                 # [n][2] at the symbol starts
    near = np.inf
    for i in range(M.SPS):
        for comp, v in enumerate((16383.0 * np.sin(p), 16383.0 * np.cos(p))):
            r = np.rint(v)
            d = np.where((r != 0.0) & (np.abs(v) <= TOP), np.abs(v - r), np.inf)
            near = min(near, float(d[d > 0.0].min()))
            for k, tone in zip(*np.nonzero((d >= LO / 2) & (d <= 2 * HI))):     # (numpy's sin: generously; libm decides below)
                ph = float(p[k, tone])
                w = 16383.0 * (math.sin(ph) if comp == 0 else math.cos(ph))
                dist = abs(w - round(w))
                if round(w) != 0 and abs(w) <= TOP and LO <= dist <= HI:
                    hits.append((f0 * M.FSYMS + int(k), i, int(tone) + 1, "IQ"[comp], dist, w))
        p[:, 0] = M._wrap(p[:, 0] + M.INC1)
        p[:, 1] = M._wrap(p[:, 1] + M.INC2)
    print(f"frames {f0}..{f0 + STEP - 1}: smallest distance to a non-zero integer {near:.3e}, hits so far {len(hits)}, {time.time() - t0:.0f} s", flush=True)
for sym, i, tone, comp, dist, w in hits:
    print(f"HIT symbol {sym} (frame {sym // M.FSYMS}) sample {i} tone {tone} component {comp} distance {dist:.3e} value {w!r}")
print("frames", first, "to", last, "hits", len(hits))
