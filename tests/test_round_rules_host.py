"""CPU-only: csrc/opv_round_rules.h - the rules of one receive round (whether a stream's offset search is due, the tie passes,
the frame budget and its refusal, which front-end kernel serves S streams with which launch, the grids of the scale pre-pass and
the decoder) - compiled with g++ into a shared object (tests/round_rules_probe.cpp gives it a C face) and called through ctypes.
Every check is exact. The reference is opv_process as it stood before the rules moved (commit d553d2a, csrc/opv_capi.hip),
restated here line by line - not derived from the header."""
import ctypes
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "opv-cxx-demod_amd" / "csrc"
U64 = ctypes.c_uint64
U32 = ctypes.c_uint32
INT = ctypes.c_int

# csrc/opv_device.h
OPV_FSYMS, OPV_CHUNK = 2168, 86720
OPV_RB_LDS_I16 = 16 + 2 * 8192 + 16 + 1025 * 32
OPV_RB_LDS_F64 = 16 + 1025 * 32 + 2048 * 32 + 16
OPV_TIE_PASSES_MAX, OPV_TIE_SLOTS_MAX = 8, 512
# FrontendKernel, in the enum's order, and the streams one workgroup of each serves (k_frontend*.hip, k_coherent.hip)
KERNELS = ["k_coherent_frontend", "k_msk_frontend_rb", "k_msk_frontend_rb_wg4", "k_msk_frontend_x4_wg4", "k_msk_frontend_x16",
           "k_msk_frontend_x16_wg4", "k_msk_frontend_x16_wg8"]
PER_WG = {"k_coherent_frontend": 1, "k_msk_frontend_rb": 1, "k_msk_frontend_rb_wg4": 4, "k_msk_frontend_x4_wg4": 16, "k_msk_frontend_x16": 16,
          "k_msk_frontend_x16_wg4": 64, "k_msk_frontend_x16_wg8": 128}


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    so = tmp_path_factory.mktemp("round_rules") / "libroundrules.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-ffp-contract=off", "-shared", "-I", str(CSRC), "-o", str(so),
                    str(ROOT / "tests" / "round_rules_probe.cpp")], check=True)
    L = ctypes.CDLL(str(so))
    L.probe_search_due.argtypes = [INT, U64, INT, INT]
    L.probe_round_searches.restype = U64
    L.probe_round_searches.argtypes = [INT, INT, U64]
    L.probe_tie_passes.restype = U32
    L.probe_tie_passes.argtypes = [U64, U32]
    L.probe_round_frames.restype = U64
    L.probe_round_frames.argtypes = [U64, U64, U32]
    L.probe_round_fits_grid.argtypes = [U64, INT]
    L.probe_frontend_choice.argtypes = [INT] * 6 + [ctypes.POINTER(U32)]
    L.probe_frontend_sweep.argtypes = [INT] * 7 + [ctypes.c_void_p]
    L.probe_back_half.argtypes = [U64, INT, ctypes.POINTER(U32)]
    L.probe_constant.restype = U32
    L.probe_constant.argtypes = [INT]
    return L


def test_the_constants_this_file_restates(rules):
    assert [rules.probe_constant(k) for k in range(7)] == [len(KERNELS), OPV_RB_LDS_I16, OPV_RB_LDS_F64, OPV_TIE_PASSES_MAX, OPV_TIE_SLOTS_MAX,
                                                           OPV_FSYMS, OPV_CHUNK]
    assert (OPV_RB_LDS_I16, OPV_RB_LDS_F64) == (49216, 98368)


# ---- the parent's opv_process (commit d553d2a, csrc/opv_capi.hip:21-28 and :340-366), constants and ladder as written there
kFrontendWg4MinStreams = 512
kFrontendX16MinStreams = 8192
kFrontendX16Wg8MinStreams = 16384
kFrontendX4MinStreams = 2049
kScaleWaveMaxFrames = 4096


def parent_frontend(S, frontend, coherent, streaming, rb_fp64_ring, n_cu):
    """-> (kernel name, grid, threads, dynamic LDS bytes) of the launch the parent's if / else-if ladder makes"""
    x4 = frontend == 4 or (frontend == 0 and S >= kFrontendX4MinStreams)
    if coherent and not streaming:
        return "k_coherent_frontend", S, 64, 0
    elif frontend == 16 or (frontend == 0 and S > kFrontendX16MinStreams):
        if S > kFrontendX16Wg8MinStreams:
            return "k_msk_frontend_x16_wg8", (S + 127) // 128, 512, 0
        elif S > 16:
            return "k_msk_frontend_x16_wg4", (S + 63) // 64, 256, 0
        else:
            return "k_msk_frontend_x16", 1, 64, 0
    elif x4:
        return "k_msk_frontend_x4_wg4", (S + 15) // 16, 256, 0
    elif S > kFrontendWg4MinStreams:
        return "k_msk_frontend_rb_wg4", (S + 3) // 4, 256, 0
    elif rb_fp64_ring and S <= n_cu:
        return "k_msk_frontend_rb", S, 128, OPV_RB_LDS_F64
    else:
        return "k_msk_frontend_rb", S, 64, OPV_RB_LDS_I16


def parent_frontend_sweep(S, frontend, coherent, streaming, rb_fp64_ring, n_cu):
    """parent_frontend over an array of stream counts, branch for branch (np.select takes the first condition that holds, as the
    ladder does): -> (kernel id, grid, threads, LDS) arrays; test_frontend_sweep_restatement_is_the_scalar_ladder holds it to the scalar"""
    one = np.ones_like(S, bool)
    x4 = one & (frontend == 4) | ((frontend == 0) & (S >= kFrontendX4MinStreams))
    x16 = one & (frontend == 16) | ((frontend == 0) & (S > kFrontendX16MinStreams))
    conds = [one & bool(coherent and not streaming), x16 & (S > kFrontendX16Wg8MinStreams), x16 & (S > 16), x16, x4, S > kFrontendWg4MinStreams,
             bool(rb_fp64_ring) & (S <= n_cu), one]
    ids = [0, 6, 5, 4, 3, 2, 1, 1]
    grids = [S, (S + 127) // 128, (S + 63) // 64, 1 * one, (S + 15) // 16, (S + 3) // 4, S, S]
    threads = [64, 512, 256, 64, 256, 256, 128, 64]
    lds = [0, 0, 0, 0, 0, 0, OPV_RB_LDS_F64, OPV_RB_LDS_I16]
    return tuple(np.select(conds, [v * one if np.isscalar(v) else v for v in col]) for col in (ids, grids, threads, lds))


COMBOS = [(forced, coherent, streaming, fp64, n_cu) for forced in (0, 1, 4, 16) for coherent in (0, 1) for streaming in (0, 1)
          for fp64 in (0, 1) for n_cu in (1, 64, 256, 304)]
S_EDGES = [1, 2, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257, 303, 304, 305, 511, 512, 513, 2047, 2048, 2049, 2050, 8191, 8192, 8193,
           16383, 16384, 16385, 16386, 32768, 40000]


def test_frontend_sweep_restatement_is_the_scalar_ladder():
    S = np.array(S_EDGES, np.int64)
    for combo in COMBOS:
        ids, grid, threads, lds = parent_frontend_sweep(S, *combo)
        for k, s in enumerate(S_EDGES):
            name, g, t, l = parent_frontend(s, *combo)
            assert (KERNELS[ids[k]], grid[k], threads[k], lds[k]) == (name, g, t, l), (s, combo)


def test_frontend_choice_is_the_parents_ladder_for_every_stream_count(rules):
    """S = 1 .. 40 000 x forced x (coherent, streaming) x fp64 ring x CU count: kernel, grid, threads and LDS bytes == the parent's
    launch; every grid serves all S streams and has no workgroup to spare; the LDS size is one of the three the kernels know"""
    S = np.arange(1, 40001, dtype=np.int64)
    out = np.zeros((S.size, 4), np.uint32)
    per_wg = np.array([PER_WG[k] for k in KERNELS], np.int64)
    for forced, coherent, streaming, fp64, n_cu in COMBOS:
        rules.probe_frontend_sweep(1, 40000, forced, coherent, streaming, fp64, n_cu, out.ctypes.data)
        exp = parent_frontend_sweep(S, forced, coherent, streaming, fp64, n_cu)
        for col, name in enumerate(("kernel", "grid", "threads", "lds")):
            bad = np.nonzero(out[:, col] != exp[col])[0]
            assert bad.size == 0, (name, forced, coherent, streaming, fp64, n_cu, int(S[bad[0]]), int(out[bad[0], col]), int(exp[col][bad[0]]))
        grid, per = out[:, 1].astype(np.int64), per_wg[out[:, 0]]
        assert np.all(grid * per >= S) and np.all(S > (grid - 1) * per), (forced, coherent, streaming, fp64, n_cu)
        assert set(np.unique(out[:, 3])) <= {0, OPV_RB_LDS_I16, OPV_RB_LDS_F64}
        rb = out[:, 0] == KERNELS.index("k_msk_frontend_rb")
        assert np.all((out[:, 3] != 0) == rb)
        assert np.all(out[rb, 3] == np.where(out[rb, 2] == 128, OPV_RB_LDS_F64, OPV_RB_LDS_I16))


def choice(rules, S, forced=0, coherent=0, streaming=1, fp64=1, n_cu=256):
    o = (U32 * 4)()
    rules.probe_frontend_choice(S, forced, coherent, streaming, fp64, n_cu, o)
    assert tuple(o) == tuple(x if k else KERNELS.index(x) for k, x in enumerate(parent_frontend(S, forced, coherent, streaming, fp64, n_cu)))
    return KERNELS[o[0]], o[1], o[2], o[3]


def test_frontend_choice_at_every_edge_by_name(rules):
    """each threshold as a literal pair: a shifted one fails here by name"""
    c = lambda *a, **k: choice(rules, *a, **k)   # noqa: E731
    assert c(512) == ("k_msk_frontend_rb", 512, 64, OPV_RB_LDS_I16)
    assert c(513) == ("k_msk_frontend_rb_wg4", 129, 256, 0)
    assert c(2048) == ("k_msk_frontend_rb_wg4", 512, 256, 0)
    assert c(2049) == ("k_msk_frontend_x4_wg4", 129, 256, 0)
    assert c(8192) == ("k_msk_frontend_x4_wg4", 512, 256, 0)
    assert c(8193) == ("k_msk_frontend_x16_wg4", 129, 256, 0)
    assert c(16384) == ("k_msk_frontend_x16_wg4", 256, 256, 0)
    assert c(16385) == ("k_msk_frontend_x16_wg8", 129, 512, 0)
    # the fp64 ring up to one stream per CU, the int16 ring beyond - and at any count where the ring is switched off
    for n_cu in (1, 64, 256, 304):
        assert c(n_cu, n_cu=n_cu) == ("k_msk_frontend_rb", n_cu, 128, OPV_RB_LDS_F64)
        assert c(n_cu + 1, n_cu=n_cu) == ("k_msk_frontend_rb", n_cu + 1, 64, OPV_RB_LDS_I16)
        assert c(n_cu, n_cu=n_cu, fp64=0) == ("k_msk_frontend_rb", n_cu, 64, OPV_RB_LDS_I16)
    assert c(512, n_cu=1024) == ("k_msk_frontend_rb", 512, 128, OPV_RB_LDS_F64) and c(513, n_cu=1024)[0] == "k_msk_frontend_rb_wg4"
    # forced mappings: sixteen per wave is one wave up to 16 streams; four per wave and one per wave at any count
    assert c(16, forced=16) == ("k_msk_frontend_x16", 1, 64, 0)
    assert c(17, forced=16) == ("k_msk_frontend_x16_wg4", 1, 256, 0)
    assert c(16384, forced=16)[0] == "k_msk_frontend_x16_wg4" and c(16385, forced=16) == ("k_msk_frontend_x16_wg8", 129, 512, 0)
    assert c(1, forced=16) == ("k_msk_frontend_x16", 1, 64, 0)
    assert c(17, forced=4) == ("k_msk_frontend_x4_wg4", 2, 256, 0) and c(1, forced=4) == ("k_msk_frontend_x4_wg4", 1, 256, 0)
    assert c(40000, forced=4) == ("k_msk_frontend_x4_wg4", 2500, 256, 0)
    assert c(2049, forced=1) == ("k_msk_frontend_rb_wg4", 513, 256, 0) and c(40000, forced=1) == ("k_msk_frontend_rb_wg4", 10000, 256, 0)
    assert c(16, forced=1) == ("k_msk_frontend_rb", 16, 128, OPV_RB_LDS_F64)
    # -c is batch only: whatever is forced, however many streams; in streaming mode it changes nothing
    for S in (1, 513, 2049, 16385):
        for forced in (0, 1, 4, 16):
            assert c(S, forced=forced, coherent=1, streaming=0) == ("k_coherent_frontend", S, 64, 0)
            assert c(S, forced=forced, coherent=1, streaming=1) == c(S, forced=forced)


# ---- the parent's arithmetic (commit d553d2a, csrc/opv_capi.hip:264, :279-283, :306, :322-323, :373-375)
def parent_search_due(streaming, n_avail, eof, search_seen):
    return (not search_seen) and ((n_avail >= OPV_CHUNK) if streaming else (eof != 0))


def parent_n_search(streaming, have_init_offset, n_due):
    return 0 if (streaming and have_init_offset) else n_due


def parent_passes(n_search, K):
    passes = (n_search + K - 1) // K
    if passes > OPV_TIE_PASSES_MAX:
        passes = OPV_TIE_PASSES_MAX
    return passes


def parent_fr(max_new, max_tapped, cap_frames):
    fr = max_new // (OPV_FSYMS * 38)
    if max_tapped // OPV_FSYMS > fr:
        fr = max_tapped // OPV_FSYMS
    fr += 4
    if fr > cap_frames:
        fr = cap_frames
    return fr


def parent_refused(fr, S):
    return fr * S > 0x7FFFFFFF


def parent_back_half(fr, S):
    """-> (k_frame_scale_wave?, its or k_frame_scale's grid, k_frame_decode's grid, its second argument)"""
    if fr * S <= kScaleWaveMaxFrames:
        wave, grid = 1, fr * S
    else:
        wave, grid = 0, (fr * S + 63) // 64
    return wave, grid & 0xFFFFFFFF, (((fr + 1) // 2) * S) & 0xFFFFFFFF, ((fr + 1) // 2) & 0xFFFFFFFF


def test_search_due_and_round_searches(rules):
    for streaming in (0, 1):
        for n_avail in (0, 1, OPV_CHUNK - 1, OPV_CHUNK, OPV_CHUNK + 1, 2**31 - 1, 2**40):
            for eof in (0, 1):
                for seen in (0, 1):
                    assert bool(rules.probe_search_due(streaming, n_avail, eof, seen)) == parent_search_due(streaming, n_avail, eof, seen)
        for have in (0, 1):
            for n_due in (0, 1, 512, 32768):
                assert rules.probe_round_searches(streaming, have, n_due) == parent_n_search(streaming, have, n_due)
    assert rules.probe_search_due(1, OPV_CHUNK - 1, 1, 0) == 0 and rules.probe_search_due(1, OPV_CHUNK, 0, 0) == 1
    assert rules.probe_search_due(0, 2**40, 0, 0) == 0 and rules.probe_search_due(0, 0, 1, 0) == 1 and rules.probe_search_due(0, 0, 1, 1) == 0
    assert rules.probe_round_searches(1, 1, 7) == 0 and rules.probe_round_searches(0, 1, 7) == 7 and rules.probe_round_searches(1, 0, 7) == 7


def test_tie_passes(rules):
    for slots in (1, 2, 17, 511, OPV_TIE_SLOTS_MAX):
        for n_search in (0, 1, slots - 1, slots, slots + 1, 8 * slots - 1, 8 * slots, 8 * slots + 1, 32768, 2**40):
            assert rules.probe_tie_passes(n_search, slots) == parent_passes(n_search, slots), (n_search, slots)
    K = OPV_TIE_SLOTS_MAX
    assert [rules.probe_tie_passes(n, K) for n in (0, 1, K, K + 1, 8 * K, 8 * K + 1)] == [0, 1, 1, 2, 8, 8]
    assert rules.probe_tie_passes(1, 1) == 1 and rules.probe_tie_passes(32768, 1) == 8


def test_round_frames_and_the_grid_refusal(rules):
    per = OPV_FSYMS * 38                                       # samples per frame, lower estimate (the parent's divisor)
    news = [0, 1, per - 1, per, per + 1, 10 * per - 1, 10 * per, 10 * per + 1, 2**31 - 1, 2**64 - 1]
    taps = [0, 1, OPV_FSYMS - 1, OPV_FSYMS, OPV_FSYMS + 1, 11 * OPV_FSYMS - 1, 11 * OPV_FSYMS, 2**28, 2**64 - 1]
    caps = [1, 3, 4, 5, 14, 15, 26070, 2**32 - 1]
    for max_new in news:
        for max_tapped in taps:
            for cap in caps:
                fr = rules.probe_round_frames(max_new, max_tapped, cap)
                assert fr == parent_fr(max_new, max_tapped, cap), (max_new, max_tapped, cap)
                for S in (1, 2, 4096, 32768, 2**31 - 1):
                    assert bool(rules.probe_round_fits_grid(fr, S)) == (not parent_refused(fr, S)), (fr, S)
    assert rules.probe_round_frames(0, 0, 14) == 4 and rules.probe_round_frames(per, 0, 14) == 5 and rules.probe_round_frames(per - 1, 0, 14) == 4
    assert rules.probe_round_frames(0, OPV_FSYMS, 14) == 5 and rules.probe_round_frames(3 * per, 7 * OPV_FSYMS, 14) == 11
    assert rules.probe_round_frames(10 * per, 0, 14) == 14 and rules.probe_round_frames(11 * per, 0, 14) == 14           # cap_frames
    assert rules.probe_round_fits_grid(65535, 32768) == 1 and rules.probe_round_fits_grid(65536, 32768) == 0             # 2^31 - 32768 | 2^31
    assert rules.probe_round_fits_grid(2**31 - 1, 1) == 1 and rules.probe_round_fits_grid(2**31, 1) == 0
    assert rules.probe_round_fits_grid(2**32 - 1, 2**31 - 1) == 0


def test_scale_shape_and_decode_grid(rules):
    o = (U32 * 4)()
    frs = [1, 2, 3, 4, 5, 14, 63, 64, 65, 4095, 4096, 4097, 65535]
    for S in (1, 2, 3, 64, 1024, 1025, 4096, 4097, 32768):
        for fr in frs + [4096 // S, 4096 // S + 1]:
            if fr == 0 or parent_refused(fr, S):
                continue
            rules.probe_back_half(fr, S, o)
            assert tuple(o) == parent_back_half(fr, S), (fr, S)
    rules.probe_back_half(4096, 1, o)
    assert tuple(o) == (1, 4096, 2048, 2048)                   # one wave per frame up to 4096 frames per round ...
    rules.probe_back_half(4097, 1, o)
    assert tuple(o) == (0, 65, 2049, 2049)                     # ... one frame per lane beyond; the decoder: two frames per wave
    rules.probe_back_half(4, 1024, o)
    assert tuple(o) == (1, 4096, 2048, 2)
    rules.probe_back_half(4, 1025, o)
    assert tuple(o) == (0, 65, 2050, 2)
    rules.probe_back_half(5, 32768, o)
    assert tuple(o) == (0, 2560, 3 * 32768, 3)
