// opv_wbtxr_rules.cpp — see opv_wbtxr_rules.h. Plain C++: no HIP, no device.
#include "opv_wbtxr_rules.h"

#include <numeric>

#include "opv_wbr_rules.h"

const char* wbtxr_cfg_refusal(const opv_wbtxr_cfg* cfg) {
    if (!cfg) return "opv_wbtxr: null configuration";
    if (cfg->up < 1) return "opv_wbtxr: up below 1";
    if (cfg->down < cfg->up || cfg->down > 8192) return "opv_wbtxr: down outside up..8192";
    if ((int64_t)cfg->down > 32 * (int64_t)cfg->up) return "opv_wbtxr: down above 32 up";
    if (std::gcd(cfg->down, cfg->up) != 1) return "opv_wbtxr: down and up share a factor";
    if (cfg->n_taps < 1 || ((int64_t)cfg->n_taps + cfg->down - 1) / cfg->down > (int64_t)kWbtxrMaxJ) return "opv_wbtxr: n_taps outside 1..64 per phase";
    if (cfg->n_channels < 1 || cfg->n_channels > 256) return "opv_wbtxr: n_channels outside 1..256";
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return "opv_wbtxr: out_shift outside 0..40";
    if (cfg->reserved != 0) return "opv_wbtxr: reserved must be 0";
    return nullptr;
}

int wbtxr_plan(const opv_wbtxr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why) {
    auto refuse = [&](const char* text) { *why = text; return (int)OPV_EINVAL; };
    if (const char* bad = wbtxr_cfg_refusal(cfg)) return refuse(bad);
    if (!centre_hz || !taps || !inc_out) return refuse("opv_wbtxr: null pointer");
    for (int p = 0; p < cfg->down && p < cfg->n_taps; ++p) {             // |y| <= 65535 x 32768 < 2^31: what licenses the kernel's int32
        int64_t gain = 0;
        for (int64_t t = p; t < cfg->n_taps; t += cfg->down) gain += taps[t] < 0 ? -(int64_t)taps[t] : (int64_t)taps[t];
        if (gain > 65535) return refuse("opv_wbtxr: sum of |taps| of one phase exceeds 65535");
    }
    switch (wbr_increments(cfg->down, cfg->up, cfg->n_channels, centre_hz, inc_out)) {   // the rational door's rule: what goes up comes down
        case WbrCentre::NotFinite: return refuse("opv_wbtxr: non-finite centre frequency");
        case WbrCentre::OutOfRange: return refuse("opv_wbtxr: centre frequency out of range");
        default: return OPV_OK;
    }
}

uint64_t wbtxr_outputs(uint32_t down, uint32_t up, uint64_t n_in_total) {
    return (n_in_total * down + (up - 1u)) / up;                          // N <= 2^50, M <= 2^13, U <= 2^13: below 2^64
}

WbtxrFirst wbtxr_first_output(uint32_t down, uint32_t up, uint64_t n_before) {
    WbtxrFirst f;
    f.n0 = wbtxr_outputs(down, up, n_before);
    f.phase = (uint32_t)(f.n0 * up - n_before * down);                    // n0 U <= N M + U - 1
    return f;
}

int wbtxr_push_plan(const opv_wbtxr_cfg& cfg, uint64_t n_before, const int16_t* const* d_in, size_t n_in, const int16_t* d_wide_out,
                    uint64_t* n_out, const char** why) {
    auto refuse = [&](int code, const char* text) { *why = text; return code; };
    *n_out = 0;
    if (!d_in || !d_wide_out) return refuse(OPV_EINVAL, "opv_wbtx_push: null pointer");
    if ((uint64_t)n_in >= (1ull << 31)) return refuse(OPV_EINVAL, "opv_wbtx_push: 2^31 or more input samples in one push");
    if (n_before + n_in > kWbtxrMaxInputs) return refuse(OPV_ECAPACITY, "opv_wbtx_push: more than 2^50 input samples per channel");
    const uint32_t M = (uint32_t)cfg.down, U = (uint32_t)cfg.up;
    const uint64_t n_wide = wbtxr_outputs(M, U, n_before + n_in) - wbtxr_outputs(M, U, n_before);
    if (n_wide >= (1ull << 31)) return refuse(OPV_EINVAL, "opv_wbtx_push: 2^31 or more wide samples in one push");
    if (n_in == 0) return OPV_OK;
    const uintptr_t out_lo = (uintptr_t)d_wide_out, out_hi = out_lo + (uintptr_t)(n_wide * 4);
    if (out_lo & 3u) return refuse(OPV_EINVAL, "opv_wbtx_push: output pointer must be 4-byte aligned");
    for (int k = 0; k < cfg.n_channels; ++k) {
        const uintptr_t lo = (uintptr_t)d_in[k], hi = lo + (uintptr_t)(n_in * 4);
        if (!lo) continue;
        if (lo & 3u) return refuse(OPV_EINVAL, "opv_wbtx_push: input pointer must be 4-byte aligned");
        if (lo < out_hi && out_lo < hi) return refuse(OPV_EINVAL, "opv_wbtx_push: the output overlaps an input");
    }
    *n_out = n_wide;
    return OPV_OK;
}

void wbtxr_phase_table(const opv_wbtxr_cfg& cfg, const int16_t* taps, int16_t* tab) {
    const uint32_t M = (uint32_t)cfg.down, J = wbtxr_taps_per_phase(cfg), row = wbtxr_row_len(cfg);
    for (uint32_t p = 0; p < M; ++p)
        for (uint32_t j = 0; j < row; ++j) {
            const uint64_t t = (uint64_t)p + (uint64_t)j * M;
            tab[(size_t)p * row + j] = j < J && t < (uint64_t)cfg.n_taps ? taps[t] : (int16_t)0;
        }
}
