// opv_wbtxr_rules.h — the rules of the rational up-converter bank (include/opv_demod.h, opv_wbtxr_* / opv_wbtx_create_rational), once
// each, in plain C++ (no HIP header: with opv_wbtxr_rules.cpp it compiles with the host compiler like opv_wbr_rules.cpp, and a
// host-only test reaches it without a device): the limits of a plan, its increments (the rational door's: opv_wbr_rules.h), the
// output count, where a push's first output sits, what refuses a push, and the tap table of k_wbtxr_duc.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/opv_demod.h"

constexpr uint32_t kWbtxrTile = 256;                     // wide outputs per workgroup of k_wbtxr_duc: one lane each
constexpr uint32_t kWbtxrMaxJ = 64;                      // taps per phase at most
constexpr uint64_t kWbtxrMaxInputs = 1ull << 50;         // N at most: N M + U stays inside uint64 (M <= 2^13)

// nullptr if cfg lies inside the limits, else why not (every refusal is OPV_EINVAL)
const char* wbtxr_cfg_refusal(const opv_wbtxr_cfg* cfg);
// J = ceil(L / M), the taps per phase, and J rounded up to a multiple of 4: the row length of the phase-major table
inline uint32_t wbtxr_taps_per_phase(const opv_wbtxr_cfg& c) { return (uint32_t)(((int64_t)c.n_taps + c.down - 1) / c.down); }
inline uint32_t wbtxr_row_len(const opv_wbtxr_cfg& c) { return (wbtxr_taps_per_phase(c) + 3u) & ~3u; }

// opv_wbtxr_plan without the error text's destination: OPV_OK, or OPV_EINVAL with *why set
int wbtxr_plan(const opv_wbtxr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why);

// W(N) = ceil(N M / U) for N <= kWbtxrMaxInputs (1 <= U <= M <= 8192)
uint64_t wbtxr_outputs(uint32_t down, uint32_t up, uint64_t n_in_total);

// The first wide sample a push behind N inputs writes: n0 = W(N). Its input is q_n0 = N exactly (U <= M: n0 U - N M < U <= M), the
// first of the push, and its phase is p_n0 = n0 U - N M (< U).
struct WbtxrFirst {
    uint64_t n0;
    uint32_t phase;
};
WbtxrFirst wbtxr_first_output(uint32_t down, uint32_t up, uint64_t n_before);

// What opv_wbtx_push decides for a rational object before anything is enqueued: OPV_OK with *n_out = W(N + n_in) - W(N) (0 for
// n_in = 0: nothing to do), or the refusal's code with *why set. d_in[k] = 0 is an absent channel.
int wbtxr_push_plan(const opv_wbtxr_cfg& cfg, uint64_t n_before, const int16_t* const* d_in, size_t n_in, const int16_t* d_wide_out,
                    uint64_t* n_out, const char** why);

// tab[p * row_len + j] = taps[p + j M] (0 where p + j M >= L): down x row_len entries, at most 8192 x 64 x 2 B = 1 MB
void wbtxr_phase_table(const opv_wbtxr_cfg& cfg, const int16_t* taps, int16_t* tab);
