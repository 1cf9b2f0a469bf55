// opv_wbr_rules.cpp — see opv_wbr_rules.h. Plain C++: no HIP, no device.
#include "opv_wbr_rules.h"

#include <cmath>
#include <numeric>

const char* wbr_cfg_refusal(const opv_wbr_cfg* cfg) {
    if (!cfg) return "opv_wbr: null configuration";
    if (cfg->up < 1 || cfg->up > 1024) return "opv_wbr: up outside 1..1024";
    if (cfg->down < cfg->up || (int64_t)cfg->down > 32 * (int64_t)cfg->up) return "opv_wbr: down outside up..32 up";
    if (std::gcd(cfg->down, cfg->up) != 1) return "opv_wbr: down and up share a factor";
    if (cfg->n_taps < 1 || ((int64_t)cfg->n_taps + cfg->up - 1) / cfg->up > 1024) return "opv_wbr: n_taps outside 1..1024 per phase";
    if (cfg->n_channels < 1 || cfg->n_channels > 256) return "opv_wbr: n_channels outside 1..256";
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return "opv_wbr: out_shift outside 0..40";
    if (cfg->reserved != 0) return "opv_wbr: reserved must be 0";
    return nullptr;
}

int wbr_plan(const opv_wbr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why) {
    auto refuse = [&](const char* text) { *why = text; return (int)OPV_EINVAL; };
    if (const char* bad = wbr_cfg_refusal(cfg)) return refuse(bad);
    if (!centre_hz || !taps || !inc_out) return refuse("opv_wbr: null pointer");
    for (int p = 0; p < cfg->up; ++p) {                                   // every phase is a filter of its own: the cap holds per phase
        int64_t gain = 0;
        for (int64_t t = p; t < cfg->n_taps; t += cfg->up) gain += taps[t] < 0 ? -(int64_t)taps[t] : (int64_t)taps[t];
        if (gain > (1ll << 21)) return refuse("opv_wbr: sum of |taps| of one phase exceeds 2^21");
    }
    switch (wbr_increments(cfg->down, cfg->up, cfg->n_channels, centre_hz, inc_out)) {
        case WbrCentre::NotFinite: return refuse("opv_wbr: non-finite centre frequency");
        case WbrCentre::OutOfRange: return refuse("opv_wbr: centre frequency out of range");
        default: return OPV_OK;
    }
}

WbrCentre wbr_increments(int32_t down, int32_t up, int32_t n_channels, const double* centre_hz, uint32_t* inc_out) {
    const double fw = (double)down * 2168000.0 / (double)up;
    for (int k = 0; k < n_channels; ++k) {
        const double f = centre_hz[k];
        if (!std::isfinite(f)) return WbrCentre::NotFinite;
        const double turns = f / fw * 4294967296.0;
        if (!(std::fabs(turns) < 9.0e18)) return WbrCentre::OutOfRange;
        inc_out[k] = (uint32_t)(uint64_t)std::llrint(turns);             // modulo 2^32: a negative centre wraps
    }
    return WbrCentre::Ok;
}

uint64_t wbr_outputs(uint32_t down, uint32_t up, uint64_t n_wide_total) {
    const unsigned __int128 t = (unsigned __int128)n_wide_total * up + (down - 1u);
    return (uint64_t)(t / down);                                          // <= N: up <= down
}

WbrFirst wbr_first_output(uint32_t down, uint32_t up, uint64_t n_before) {
    WbrFirst f;
    f.r0 = wbr_outputs(down, up, n_before);
    const unsigned __int128 t = (unsigned __int128)f.r0 * down;           // r0 M >= N U, so floor(r0 M / U) >= N
    f.n_rel = (uint64_t)(t / up - n_before);                              // < M / U + 1
    f.phase = (uint32_t)(t % up);
    return f;
}

void wbr_phase_table(const opv_wbr_cfg& cfg, const int16_t* taps, int16_t* tab) {
    const uint32_t U = (uint32_t)cfg.up, J = wbr_taps_per_phase(cfg), row = wbr_row_len(cfg);
    for (uint32_t p = 0; p < U; ++p)
        for (uint32_t j = 0; j < row; ++j) {
            const uint64_t t = (uint64_t)p + (uint64_t)j * U;
            tab[(size_t)p * row + j] = j < J && t < (uint64_t)cfg.n_taps ? taps[t] : (int16_t)0;
        }
}
