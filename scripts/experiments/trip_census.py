"""dev: census of the steady-state symbol loops of the one-wave front-end kernels, read from the device assembly the library is
built from (default: build/k_frontend.al.s; another file as first argument). Every innermost loop (a label and the conditional
backward branch to it, no other such loop between them) that holds N x 31 v_fmac_f64_dpp (thirty for the window sums, one for the soft value) is one trip loop of N symbols: its instruction
count per symbol, s_nop, v_max_f64 / v_min_f64 (two per symbol are the AFC clamp, two more the timing clamp where the nest keeps
it), backward branches; and per kernel the VGPR count and scratch. (loop_census.py takes the last loop with 124 FMACs, which
since the batches of whole trips is the batch loop around them.)"""
import collections
import re
import sys
from pathlib import Path

asm = Path(sys.argv[1]) if len(sys.argv) > 1 else Path(__file__).resolve().parents[2] / "opv-cxx-demod_amd" / "build" / "k_frontend.al.s"
L = asm.read_text().split("\n")
for fn in ("k_msk_frontend_rb", "k_msk_frontend_rb_wg4"):
    start = next(i for i, l in enumerate(L) if l.startswith(fn + ":"))
    end = next(i for i in range(start, len(L)) if L[i].startswith(".Lfunc_end"))
    labels = {m.group(1): i for i in range(start, end) if (m := re.match(r"^(\.LBB\d+_\d+):", L[i]))}
    back = []
    for i in range(start, end):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", L[i])
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            back.append((labels[m.group(1)], i))
    meta = "\n".join(L)
    vg = re.search(r"\.name:\s+" + fn + r"\n(?:.*\n)*?.*\.vgpr_count:\s+(\d+)", meta)
    sc = re.search(r"\.amdhsa_kernel " + fn + r"\n(?:.*\n)*?\s+\.amdhsa_private_segment_fixed_size (\d+)", meta)
    print(f"{fn}: vgpr_count {vg.group(1) if vg else '?'}, scratch {sc.group(1) if sc else '?'} bytes")
    for a, b in back:
        if not L[b].strip().startswith("s_cbranch") or any(a <= a2 and b2 <= b and (a2, b2) != (a, b) and L[b2].strip().startswith("s_cbranch") for a2, b2 in back):
            continue                        # the way back from an out-of-line silence block (s_branch into the loop), or not innermost
        body = [l.strip().split(";")[0].strip() for l in L[a:b + 1] if l.strip() and not l.strip().startswith(";") and not re.match(r"^\.L", l.strip())]
        c = collections.Counter(x.split()[0].replace("_e32", "").replace("_e64", "") for x in body)
        n = c["v_fmac_f64_dpp"]
        if n == 0 or n % 31:
            continue
        n //= 31
        print(f"  loop at line {a + 1}: {n} symbols, {len(body)} instructions = {len(body) / n:.2f} per symbol; s_nop {c['s_nop']}, "
              f"v_max_f64 {c['v_max_f64']}, v_min_f64 {c['v_min_f64']}, backward branches {sum(1 for a2, b2 in back if a <= a2 and b2 <= b)}")
        # the cross-row sums (two v_mfma_f64_4x4x4 per symbol, no permlane swap) and the soft log's stores (a trip of four: two
        # global_store_dwordx4; a remainder loop: one global_store_dwordx2 per symbol); AGPR traffic would be a spill
        print(f"    v_mfma_f64 {sum(v for k, v in c.items() if k.startswith('v_mfma_f64'))}, permlane swaps {sum(v for k, v in c.items() if k.startswith('v_permlane'))}, "
              f"global_store_dwordx2 {c['global_store_dwordx2']}, global_store_dwordx4 {c['global_store_dwordx4']}, "
              f"v_accvgpr {sum(v for k, v in c.items() if k.startswith('v_accvgpr'))}, forward branches {sum(1 for x in body if x.startswith(('s_cbranch', 's_branch'))) - 1}")
        # the silence test: a v_cmp_eq_f64 and the forward branch that reads its mask. Where the mask is vcc, what stands between
        # the two must neither write vcc nor copy it
        cmps = [i for i, x in enumerate(body) if x.startswith("v_cmp_eq_f64")]
        on_vcc = [i for i in cmps if re.match(r"v_cmp_eq_f64\w*\s+vcc\b", body[i])]
        gaps, touched = [], 0
        for i in on_vcc:
            j = next((k for k in range(i + 1, len(body)) if body[k].startswith("s_cbranch_vcc")), None)
            if j is None:
                touched += 1
                continue
            gaps.append(j - i - 1)
            touched += sum(1 for x in body[i + 1:j] if re.search(r"\bvcc\b", x))
        print(f"    silence test: {len(cmps)} compares, {len(on_vcc)} on vcc with an s_cbranch_vcc* {gaps} instructions later, "
              f"{touched} instructions between that name vcc, s_cmp on the mask {c['s_cmp_eq_u64'] + c['s_cmp_lg_u64']}")
