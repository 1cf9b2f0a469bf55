// round_rules_probe.cpp — test support for csrc/opv_round_rules.h (plain C++, no GPU): a C face for ctypes
// (tests/test_round_rules_host.py) and, with -DPROBE_MAIN, a stand-alone program that sweeps the same rules and prints one line
// (tests/test_sanitizers.py builds it with and without sanitizers and compares the lines).
#include <cstdio>
#include <initializer_list>

#include "opv_round_rules.h"

extern "C" {
int probe_search_due(int streaming, uint64_t n_avail, int eof, int search_seen) { return search_due(streaming, n_avail, eof, search_seen != 0); }
uint64_t probe_round_searches(int streaming, int have_init_offset, uint64_t n_due) { return round_searches(streaming, have_init_offset, (size_t)n_due); }
uint32_t probe_tie_passes(uint64_t n_search, uint32_t slots) { return tie_passes((size_t)n_search, slots); }
uint64_t probe_round_frames(uint64_t max_new, uint64_t max_tapped, uint32_t cap_frames) { return round_frames(max_new, max_tapped, cap_frames); }
int probe_round_fits_grid(uint64_t fr, int S) { return round_fits_grid(fr, S); }
// out = {kernel id, grid, threads, dynamic LDS bytes}
void probe_frontend_choice(int S, int forced, int coherent, int streaming, int fp64_ring, int n_cu, uint32_t out[4]) {
    const FrontendChoice ch = frontend_choice(S, forced, coherent != 0, streaming != 0, fp64_ring != 0, n_cu);
    out[0] = (uint32_t)ch.kernel; out[1] = ch.grid; out[2] = ch.threads; out[3] = ch.lds;
}
// the same for S = s_lo .. s_hi (one call per sweep): out[4 * (S - s_lo) ..]
void probe_frontend_sweep(int s_lo, int s_hi, int forced, int coherent, int streaming, int fp64_ring, int n_cu, uint32_t* out) {
    for (int S = s_lo; S <= s_hi; ++S) probe_frontend_choice(S, forced, coherent, streaming, fp64_ring, n_cu, out + 4 * (size_t)(S - s_lo));
}
// out = {one wave per frame (1) or one frame per lane (0), the scale pre-pass' grid, the decoder's grid, its frame pairs per stream}
void probe_back_half(uint64_t fr, int S, uint32_t out[4]) {
    const ScaleShape sc = scale_shape(fr, S);
    out[0] = sc.wave; out[1] = sc.grid; out[2] = decode_grid(fr, S); out[3] = decode_pairs(fr);
}
uint32_t probe_constant(int which) {
    const uint32_t v[] = {FE_N, OPV_RB_LDS_I16, OPV_RB_LDS_F64, OPV_TIE_PASSES_MAX, OPV_TIE_SLOTS_MAX, OPV_FSYMS, OPV_CHUNK};
    return v[which];
}
}

#ifdef PROBE_MAIN
int main() {
    unsigned long long acc = 0, n = 0;
    auto mix = [&](unsigned long long v) { acc = acc * 1000003ull + v; ++n; };
    // every launch the front-end rule can name: a grid that serves all S streams with no workgroup to spare, a known block, a known LDS size
    for (int forced : {0, 1, 4, 16})
        for (int mode = 0; mode < 4; ++mode)
            for (int f64 = 0; f64 < 2; ++f64)
                for (int n_cu : {1, 64, 256, 304})
                    for (int S = 1; S <= 40000; ++S) {
                        uint32_t o[4];
                        probe_frontend_choice(S, forced, mode & 1, mode >> 1, f64, n_cu, o);
                        if (o[0] >= FE_N || o[1] < 1 || o[2] != kFrontendShape[o[0]].threads * (o[0] == FE_RB && o[3] == OPV_RB_LDS_F64 ? 2u : 1u)) return 2;
                        const uint64_t per = (uint64_t)kFrontendShape[o[0]].streams;
                        if (o[1] * per < (uint64_t)S || (o[1] - 1) * per >= (uint64_t)S) return 3;
                        if (o[3] != 0 && o[3] != OPV_RB_LDS_I16 && o[3] != OPV_RB_LDS_F64) return 4;
                        mix(o[0]); mix(o[1]); mix(o[2]); mix(o[3]);
                    }
    // the frame budget, the refusal and the back half's grids around every divisor and limit
    const uint64_t per_frame = (uint64_t)OPV_FSYMS * 38;
    for (uint64_t max_new : {(uint64_t)0, per_frame - 1, per_frame, per_frame + 1, 10 * per_frame, ((uint64_t)1 << 31) - 1, ~(uint64_t)0})
        for (uint64_t tapped : {(uint64_t)0, (uint64_t)OPV_FSYMS - 1, (uint64_t)OPV_FSYMS, (uint64_t)OPV_FSYMS + 1, (uint64_t)1 << 28, ~(uint64_t)0})
            for (uint32_t cap : {1u, 4u, 5u, 14u, 26070u, 0xFFFFFFFFu}) {
                const uint64_t fr = probe_round_frames(max_new, tapped, cap);
                if (fr > cap || fr < 1) return 5;
                for (int S : {1, 2, 63, 64, 65, 4096, 4097, 32768, 0x7FFFFFFF}) {
                    const int fits = probe_round_fits_grid(fr, S);
                    mix(fr); mix((unsigned long long)fits);
                    if (!fits) continue;
                    uint32_t o[4];
                    probe_back_half(fr, S, o);
                    if ((uint64_t)o[1] * (o[0] ? 1 : 64) < fr * (uint64_t)S || (uint64_t)o[2] * 2 < fr * (uint64_t)S || o[2] != o[3] * (uint64_t)S) return 6;
                    mix(o[0]); mix(o[1]); mix(o[2]); mix(o[3]);
                }
            }
    for (uint32_t slots : {1u, 2u, 17u, 512u})
        for (uint64_t k : {(uint64_t)0, (uint64_t)1, (uint64_t)slots - 1, (uint64_t)slots, (uint64_t)slots + 1, (uint64_t)8 * slots, (uint64_t)8 * slots + 1, (uint64_t)1 << 40}) {
            const uint32_t p = probe_tie_passes(k, slots);
            if (p > OPV_TIE_PASSES_MAX || (uint64_t)p * slots < (k < 8ull * slots ? k : 8ull * slots)) return 7;
            mix(p);
        }
    for (int streaming = 0; streaming < 2; ++streaming)
        for (uint64_t avail : {(uint64_t)0, (uint64_t)OPV_CHUNK - 1, (uint64_t)OPV_CHUNK, (uint64_t)OPV_CHUNK + 1, ~(uint64_t)0})
            for (int eof = 0; eof < 2; ++eof)
                for (int seen = 0; seen < 2; ++seen) {
                    mix((unsigned long long)probe_search_due(streaming, avail, eof, seen));
                    mix(probe_round_searches(streaming, eof, avail));
                }
    std::printf("%llu %llx\n", n, acc);
    return 0;
}
#endif
