// opv_wbr_rules.h — the rules of the rational wideband front door (include/opv_demod.h, opv_wbr_* / opv_wb_create_rational), once
// each, in plain C++ (no HIP header: with opv_wbr_rules.cpp it compiles with the host compiler like opv_stream_rules.cpp and
// opv_txb_rules.cpp, and a host-only test reaches it without a device): the limits of a plan, its increments, the output count
// and where a push's first output sits - the only places that need 128-bit arithmetic - the tile of k_wbr_ddc and its tap table.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/opv_demod.h"

constexpr uint32_t kWbrSpan = 4096;         // wide samples a workgroup of k_wbr_ddc holds in LDS (= OPV_WB_SPAN, asserted in opv_wideband.hip)
constexpr uint32_t kWbrMaxTile = 256;       // outputs per workgroup at most: one lane each

// nullptr if cfg lies inside the limits, else why not (every refusal is OPV_EINVAL)
const char* wbr_cfg_refusal(const opv_wbr_cfg* cfg);
// J = ceil(L / U), the taps per phase, and J rounded up to a multiple of 4: the row length of the phase-major table
inline uint32_t wbr_taps_per_phase(const opv_wbr_cfg& c) { return (uint32_t)(((int64_t)c.n_taps + c.up - 1) / c.up); }
inline uint32_t wbr_row_len(const opv_wbr_cfg& c) { return (wbr_taps_per_phase(c) + 3u) & ~3u; }

// opv_wbr_plan without the error text's destination: OPV_OK, or OPV_EINVAL with *why set
int wbr_plan(const opv_wbr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why);

// The increment rule of a wide rate of 2 168 000 x down / up S/s, for both directions (the rational up-converter bank plans with it
// too, opv_wbtxr_rules.cpp): inc_out[k] for k < n_channels, or which centre it met that has no increment
enum class WbrCentre { Ok, NotFinite, OutOfRange };
WbrCentre wbr_increments(int32_t down, int32_t up, int32_t n_channels, const double* centre_hz, uint32_t* inc_out);

// ceil(N U / M) for any uint64 N (1 <= U <= M)
uint64_t wbr_outputs(uint32_t down, uint32_t up, uint64_t n_wide_total);

// The first output a push behind N wide samples makes: r0 = ceil(N U / M), and of that output n_r0 - N (>= 0: where its newest
// wide sample lies within the push) and p_r0 = (r0 M) mod U
struct WbrFirst {
    uint64_t r0;
    uint64_t n_rel;
    uint32_t phase;
};
WbrFirst wbr_first_output(uint32_t down, uint32_t up, uint64_t n_before);

// Outputs per workgroup: as many as keep the workgroup's span - row_len - 1 samples in front, floor(tile M / U) + 1 new ones -
// inside kWbrSpan. Never below 96 (row_len <= 1024, M / U <= 32).
inline uint32_t wbr_tile(uint32_t down, uint32_t up, uint32_t row_len) {
    const uint64_t t = (uint64_t)(kWbrSpan - row_len) * up / down;
    return t > kWbrMaxTile ? kWbrMaxTile : (uint32_t)t;
}

// tab[p * row_len + j] = taps[p + j U] (0 where p + j U >= L): up x row_len entries
void wbr_phase_table(const opv_wbr_cfg& cfg, const int16_t* taps, int16_t* tab);
