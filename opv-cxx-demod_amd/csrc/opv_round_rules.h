// opv_round_rules.h — the rules of one receive round (opv_capi.hip: opv_process), once each, in plain C++ (no HIP header: like
// opv_stream_rules.h it compiles with the host compiler and runs under sanitizers without a GPU - tests/test_round_rules_host.py,
// tests/round_rules_probe.cpp). The shim launches what these say; the thresholds of the stream-to-wave mapping live here only.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/opv_demod.h"
#include "opv_device.h"

// ---- the offset search: k_offset_search's own condition (first full chunk in streaming mode, EOF in batch mode), once per stream
inline bool search_due(int streaming, uint64_t n_avail, int eof, bool search_seen) {
    return !search_seen && (streaming ? n_avail >= (uint64_t)OPV_CHUNK : eof != 0);
}
// searches that can run this round: none under a streaming -o (ref :1031)
inline size_t round_searches(int streaming, int have_init_offset, size_t n_due) { return (streaming && have_init_offset) ? 0 : n_due; }
// passes of the host's tie decision: at most n_search streams can be listed, `slots` of them per pass - but never more than
// OPV_TIE_PASSES_MAX (8 x 512 = 4096 listed streams per round): a pass nobody is listed for costs the stream ~30 us
// (scripts/microbench/hostfunc.hip), a 32 768-stream round would pay for 64 of them, and a last-place tie that is NOT an exact
// mirror happens to about one stream in ten thousand (exact mirrors - real-valued captures, the one systematic source - come out
// the same on the device: test_offset_search_ties_decided_like_the_reference runs both paths). Streams listed beyond that keep
// the device's decision and are counted (opv_offset_ties_left_to_device).
inline uint32_t tie_passes(size_t n_search, uint32_t slots) {
    const size_t passes = (n_search + slots - 1) / slots;
    return passes > OPV_TIE_PASSES_MAX ? OPV_TIE_PASSES_MAX : (uint32_t)passes;
}

// ---- frames a stream can release this round: new symbols / 2168 plus what was pending (staged soft symbols count as what they
// are: one frame per 2168 of them); and the refusal: streams x frames is a grid dimension
inline uint64_t round_frames(uint64_t max_new, uint64_t max_tapped, uint32_t cap_frames) {
    const uint64_t by_iq = max_new / (uint64_t)(OPV_FSYMS * 38), by_soft = max_tapped / (uint64_t)OPV_FSYMS, fr = (by_soft > by_iq ? by_soft : by_iq) + 4;
    return fr > cap_frames ? cap_frames : fr;
}
inline bool round_fits_grid(uint64_t fr, int S) { return fr * (uint64_t)S <= 0x7FFFFFFFull; }

// ---- the front-end: which kernel serves S streams, and its launch
enum FrontendKernel { FE_COHERENT, FE_RB, FE_RB_WG4, FE_X4_WG4, FE_X16, FE_X16_WG4, FE_X16_WG8, FE_N };
// streams and threads of a workgroup: one wave per stream (alone, or four to a workgroup = one per SIMD of a CU by construction),
// four per wave x four waves, sixteen per wave x one, four or eight waves (FE_RB: 128 threads in its fp64-ring shape, below)
struct FrontendShape { int streams; uint32_t threads; };
constexpr FrontendShape kFrontendShape[FE_N] = {{1, 64}, {1, 64}, {4, 256}, {16, 256}, {16, 64}, {64, 256}, {128, 512}};

// One wave per stream has the shortest per-symbol latency (what counts while SIMDs are idle); four streams per wave issue fewer
// instructions per symbol and stream, which pays once there are more streams than the one-wave kernel's two rounds of 1024 hold.
// `forced`: opv_set_frontend's 1 / 4 / 16 (0: by stream count).
inline FrontendKernel frontend_kernel(int S, int forced, bool coherent, bool streaming) {
    if (coherent && !streaming) return FE_COHERENT;        // -c, batch only (ref :1144-1161)
    // sixteen per wave. Measured on MI355X (NOTEBOOK.md §3.1): 8192 streams x 16 frames: four per wave 260 GS/s, sixteen per wave
    // 247 (512 waves: half the SIMDs idle; with 7 frames per stream, bench.py's sweep, 221 / 255: the cross-over IS about 8192);
    // 16 384 x 8: 187 / 478; 32 768 x 8: 204 / 574
    if (forced == 16 || (forced == 0 && S > 8192)) {
        if (S > 16384) return FE_X16_WG8;                  // 1024 waves of sixteen streams = one per SIMD; beyond that eight waves (two per SIMD) per workgroup
        return S > 16 ? FE_X16_WG4 : FE_X16;               // four waves (64 streams) per workgroup; a context of one wave: that wave
    }
    // four per wave, four waves per workgroup whatever the stream count. Measured on MI355X (NOTEBOOK.md §3.1): one wave per stream
    // runs 1024 streams at a time (46 ms per 2048 x 30 frames, 69 ms from 2049 on), four per wave 4096 (47.5 ms)
    if (forced == 4 || (forced == 0 && S > 2048)) return FE_X4_WG4;
    // one wave per stream, row-broadcast reduction (k_frontend.hip: symbol_r). Its 272-278 registers allow one wave per SIMD; four
    // waves per workgroup from the stream count at which single-wave workgroups start to double up on SIMDs (msk_frontend_body)
    return S > 512 ? FE_RB_WG4 : FE_RB;
}
struct FrontendChoice { FrontendKernel kernel; uint32_t grid, threads, lds; };   // lds: dynamic LDS bytes
inline FrontendChoice frontend_choice(int S, int forced, bool coherent, bool streaming, bool fp64_ring, int n_cu) {
    const FrontendKernel k = frontend_kernel(S, forced, coherent, streaming);
    FrontendChoice ch{k, (uint32_t)((S + kFrontendShape[k].streams - 1) / kFrontendShape[k].streams), kFrontendShape[k].threads, 0};
    if (k == FE_RB) {      // while S <= CUs a helper wave per stream widens the IQ to fp64 (k_frontend.hip: f64_ring_helper): one workgroup per CU
        const bool f64 = fp64_ring && S <= n_cu;
        ch.threads = f64 ? 128 : 64;
        ch.lds = f64 ? OPV_RB_LDS_F64 : OPV_RB_LDS_I16;
    }
    return ch;
}

// ---- the back half. The quantiser's scale (2144 dependent additions per frame): one frame per lane - the HBM-rate shape - for
// bulk rounds; one wave per frame while the round is so small (<= 4096 frames, upper estimate) that a wave of 64 frames would be
// the whole launch: a live round of 64 frames 46 -> 12 us. The decoder: two frames per wave.
struct ScaleShape { bool wave; uint32_t grid; };
inline ScaleShape scale_shape(uint64_t fr, int S) {
    const uint64_t n = fr * (uint64_t)S;
    return n <= 4096 ? ScaleShape{true, (uint32_t)n} : ScaleShape{false, (uint32_t)((n + 63) / 64)};
}
inline uint32_t decode_pairs(uint64_t fr) { return (uint32_t)((fr + 1) / 2); }
inline uint32_t decode_grid(uint64_t fr, int S) { return (uint32_t)(((fr + 1) / 2) * (uint64_t)S); }
