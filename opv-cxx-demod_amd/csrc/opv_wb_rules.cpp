// opv_wb_rules.cpp — see opv_wb_rules.h. Plain C++: no HIP, no device.
#include "opv_wb_rules.h"

#include <cmath>
#include <numeric>

namespace {

int refuse(const char** why, int code, const char* text) {
    *why = text;
    return code;
}

}  // namespace

// A plan's last step, the increment rule of a wide rate of 2 168 000 x down / up S/s: inc_out[k] = (uint32) llrint(centre_hz[k] /
// rate x 2^32). One rule for both directions - what goes up comes down - and for the integer kinds, which have up = 1. The two
// refusals come in the words of the plan that asks. (opv_scan_rules.cpp's plan ends with it too.)
int wb_plan_increments(int32_t down, int32_t up, int32_t n_channels, const double* centre_hz, uint32_t* inc_out, const char** why,
                       const char* not_finite, const char* out_of_range) {
    const double fw = (double)down * 2168000.0 / (double)up;
    for (int k = 0; k < n_channels; ++k) {
        const double f = centre_hz[k];
        if (!std::isfinite(f)) return refuse(why, OPV_EINVAL, not_finite);
        const double turns = f / fw * 4294967296.0;
        if (!(std::fabs(turns) < 9.0e18)) return refuse(why, OPV_EINVAL, out_of_range);
        inc_out[k] = (uint32_t)(uint64_t)std::llrint(turns);             // modulo 2^32: a negative centre wraps
    }
    return OPV_OK;
}

// ---- the LO schedule
int wb_seg_next(const opv_wb_seg* prev, int32_t down, int32_t up, uint64_t at, double centre_hz, double rate_hz_s, opv_wb_seg* out, const char** why) {
    if (!prev || !out) return refuse(why, OPV_EINVAL, "opv_wb_seg_next: null pointer");
    if (down < 1 || up < 1) return refuse(why, OPV_EINVAL, "opv_wb_seg_next: down or up below 1");
    if (!std::isfinite(rate_hz_s)) return refuse(why, OPV_EINVAL, "opv_wb_seg_next: non-finite rate");
    if (std::fabs(rate_hz_s) > OPV_WB_TUNE_MAX_RATE) return refuse(why, OPV_EINVAL, "opv_wb_seg_next: |rate_hz_s| above OPV_WB_TUNE_MAX_RATE");
    uint32_t inc32 = 0;
    if (int r = wb_plan_increments(down, up, 1, &centre_hz, &inc32, why, "opv_wb_seg_next: non-finite centre frequency",
                                   "opv_wb_seg_next: centre frequency out of range"))
        return r;
    const double fw = (double)down * 2168000.0 / (double)up;
    opv_wb_seg s;
    s.start = at;
    s.phase = wb_seg_phase(*prev, at);
    s.inc = (uint64_t)inc32 << 32;
    s.ramp = (int64_t)std::llrint(rate_hz_s / fw / fw * 18446744073709551616.0);   // |.| <= 1e7 / 2 168 000^2 x 2^64 < 2^46
    *out = s;
    return OPV_OK;
}

void wb_sched_reset(WbSchedule& s, int32_t down, int32_t up, uint32_t K, const uint32_t* inc) {
    s.down = down;
    s.up = up;
    s.inc.assign(inc, inc + K);
    s.seg.assign(K, std::vector<opv_wb_seg>());
    for (uint32_t k = 0; k < K; ++k) s.seg[k].push_back(opv_wb_seg{0, 0, (uint64_t)inc[k] << 32, 0});
    s.created.assign(K, 1);
}

bool wb_sched_plain(const WbSchedule& s) {
    for (size_t k = 0; k < s.seg.size(); ++k)
        if (!s.created[k] || s.seg[k].size() != 1) return false;
    return true;
}

namespace {

// one channel's list: the segments in front of the last one that starts at or before `oldest` go. A start is compared as a
// distance from `oldest`, so that a first_sample near 2^64 would wrap like every other index here.
void prune_channel(std::vector<opv_wb_seg>& seg, uint8_t& created, uint64_t oldest) {
    size_t keep = 0;
    for (size_t i = 1; i < seg.size(); ++i)
        if ((int64_t)(seg[i].start - oldest) <= 0) keep = i;
    if (keep) {
        seg.erase(seg.begin(), seg.begin() + (ptrdiff_t)keep);
        created = 0;
    }
}

}  // namespace

void wb_sched_prune(WbSchedule& s, uint64_t oldest) {
    for (size_t k = 0; k < s.seg.size(); ++k) prune_channel(s.seg[k], s.created[k], oldest);
}

int wb_sched_retune(WbSchedule& s, uint64_t A, uint64_t oldest, int count, const opv_wb_tune* tunes, const char** why) {
    if (count < 0) return refuse(why, OPV_EINVAL, "opv_wb_retune: count below 0");
    if (count == 0) return OPV_OK;
    if (!tunes) return refuse(why, OPV_EINVAL, "opv_wb_retune: null pointer");
    const int K = (int)s.seg.size();
    // ---- what is wrong with an entry by itself
    for (int i = 0; i < count; ++i) {
        const opv_wb_tune& t = tunes[i];
        if (t.channel < 0 || t.channel >= K) return refuse(why, OPV_EINVAL, "opv_wb_retune: channel out of range");
        if (!std::isfinite(t.centre_hz) || !std::isfinite(t.rate_hz_s)) return refuse(why, OPV_EINVAL, "opv_wb_retune: non-finite centre or rate");
        if (std::fabs(t.rate_hz_s) > OPV_WB_TUNE_MAX_RATE) return refuse(why, OPV_EINVAL, "opv_wb_retune: |rate_hz_s| above OPV_WB_TUNE_MAX_RATE");
    }
    for (int i = 0; i < count; ++i)
        if (tunes[i].at < A) return refuse(why, OPV_ESTATE, "opv_wb_retune: the past cannot be retuned");
    // ---- the batch on copies of the lists it touches: the object's own change only once nothing can refuse any more
    std::vector<int> touched;
    std::vector<std::vector<opv_wb_seg>> lists;
    std::vector<uint8_t> flags;
    for (int i = 0; i < count; ++i) {
        const opv_wb_tune& t = tunes[i];
        size_t at = 0;
        while (at < touched.size() && touched[at] != t.channel) ++at;
        if (at == touched.size()) {
            touched.push_back(t.channel);
            lists.push_back(s.seg[(size_t)t.channel]);
            flags.push_back(s.created[(size_t)t.channel]);
            prune_channel(lists[at], flags[at], oldest);
        }
        std::vector<opv_wb_seg>& seg = lists[at];
        const opv_wb_seg& last = seg.back();
        const bool creation = flags[at] && seg.size() == 1;
        if (!creation && t.at - last.start < (uint64_t)OPV_WB_TUNE_GAP)           // (t.at >= A >= last.start unless last lies ahead: then the difference wraps or is small)
            return refuse(why, OPV_EINVAL, "opv_wb_retune: less than OPV_WB_TUNE_GAP samples behind the channel's last segment");
        if (!creation && (int64_t)(t.at - last.start) < 0) return refuse(why, OPV_EINVAL, "opv_wb_retune: in front of the channel's last segment");
        opv_wb_seg next;
        if (int r = wb_seg_next(&last, s.down, s.up, t.at, t.centre_hz, t.rate_hz_s, &next, why)) return r;
        if (t.phase_given) next.phase = t.phase;
        seg.push_back(next);
        prune_channel(seg, flags[at], oldest);                                   // (a tune at the oldest sample replaces what was there: N = 0 and the creation segment)
        if (seg.size() > (size_t)OPV_WB_TUNE_SEGS) return refuse(why, OPV_ECAPACITY, "opv_wb_retune: more than OPV_WB_TUNE_SEGS segments on a channel");
    }
    for (size_t i = 0; i < touched.size(); ++i) {
        s.seg[(size_t)touched[i]].swap(lists[i]);
        s.created[(size_t)touched[i]] = flags[i];
    }
    return OPV_OK;
}

int wb_sched_copy(const WbSchedule& s, int channel, opv_wb_seg* out, size_t cap) {
    if (channel < 0 || channel >= (int)s.seg.size()) return OPV_EINVAL;
    const std::vector<opv_wb_seg>& seg = s.seg[(size_t)channel];
    for (size_t i = 0; i < seg.size() && i < cap && out; ++i) out[i] = seg[i];
    return (int)seg.size();
}

void wb_sched_table(const WbSchedule& s, uint64_t origin, uint64_t reach, OpvWbDevSched* out) {
    for (size_t k = 0; k < s.seg.size(); ++k) {
        const std::vector<opv_wb_seg>& seg = s.seg[k];
        OpvWbDevSched& t = out[k];
        uint32_t n = 0;
        for (size_t i = 0; i < seg.size() && n < (uint32_t)OPV_WB_TUNE_SEGS; ++i) {
            const int64_t rel = (int64_t)(seg[i].start - origin);
            if (i + 1 < seg.size() && (int64_t)(seg[i + 1].start - origin) <= 0) continue;   // over before the origin
            if (rel > 0 && (uint64_t)rel >= reach) break;                                     // begins behind the push
            if (rel <= 0) {                                                                   // re-based to the origin
                const uint64_t d0 = origin - seg[i].start;
                t.start[n] = 0;
                t.phase[n] = wb_seg_phase(seg[i], origin);
                t.inc[n] = seg[i].inc + (uint64_t)seg[i].ramp * d0;
            } else {
                t.start[n] = (uint32_t)rel;
                t.phase[n] = seg[i].phase;
                t.inc[n] = seg[i].inc;
            }
            t.ramp[n] = seg[i].ramp;
            ++n;
        }
        for (; n < (uint32_t)OPV_WB_TUNE_SEGS; ++n) {
            t.start[n] = 0xFFFFFFFFu;
            t.phase[n] = t.inc[n] = 0;
            t.ramp[n] = 0;
        }
    }
}

extern "C" void opv_wb_lo_table(int16_t out4096[4096]) {
    if (!out4096) return;
    for (int i = 0; i < 4096; ++i) out4096[i] = (int16_t)std::lrint(32767.0 * std::cos(2.0 * 3.14159265358979323846 * (double)i / 4096.0));
}

bool wb_phase_gain_within(const int16_t* taps, int64_t n_taps, int64_t stride, int64_t cap) {
    for (int64_t p = 0; p < stride && p < n_taps; ++p) {
        int64_t gain = 0;
        for (int64_t t = p; t < n_taps; t += stride) gain += taps[t] < 0 ? -(int64_t)taps[t] : (int64_t)taps[t];
        if (gain > cap) return false;
    }
    return true;
}

void wb_phase_table(const int16_t* taps, int64_t n_taps, uint32_t stride, uint32_t J, uint32_t row_len, int16_t* tab) {
    for (uint32_t p = 0; p < stride; ++p)
        for (uint32_t j = 0; j < row_len; ++j) {
            const int64_t t = (int64_t)p + (int64_t)j * stride;
            tab[(size_t)p * row_len + j] = j < J && t < n_taps ? taps[t] : (int16_t)0;
        }
}

// ---- the front doors: |acc| <= 2^21 x 32768 x 32767 x 2 < 2^52 over the taps of a phase
int wb_plan(const opv_wb_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why) {
    if (!cfg) return refuse(why, OPV_EINVAL, "opv_wb: null configuration");
    if (cfg->decim < 1 || cfg->decim > 16) return refuse(why, OPV_EINVAL, "opv_wb: decim outside 1..16");
    if (cfg->n_channels < 1 || cfg->n_channels > 256) return refuse(why, OPV_EINVAL, "opv_wb: n_channels outside 1..256");
    if (cfg->n_taps < 1 || cfg->n_taps > 1024) return refuse(why, OPV_EINVAL, "opv_wb: n_taps outside 1..1024");
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return refuse(why, OPV_EINVAL, "opv_wb: out_shift outside 0..40");
    if (!centre_hz || !taps || !inc_out) return refuse(why, OPV_EINVAL, "opv_wb: null pointer");
    if (!wb_phase_gain_within(taps, cfg->n_taps, 1, 1ll << 21)) return refuse(why, OPV_EINVAL, "opv_wb: sum of |taps| exceeds 2^21");
    return wb_plan_increments(cfg->decim, 1, cfg->n_channels, centre_hz, inc_out, why, "opv_wb: non-finite centre frequency",
                              "opv_wb: centre frequency out of range");
}

int wbr_ratio_fault(int32_t down, int32_t up) {
    if (up < 1 || up > 1024) return 1;
    if (down < up || (int64_t)down > 32 * (int64_t)up) return 2;
    if (std::gcd(down, up) != 1) return 3;
    return 0;
}

const char* wbr_cfg_refusal(const opv_wbr_cfg* cfg) {
    if (!cfg) return "opv_wbr: null configuration";
    switch (wbr_ratio_fault(cfg->down, cfg->up)) {
        case 1: return "opv_wbr: up outside 1..1024";
        case 2: return "opv_wbr: down outside up..32 up";
        case 3: return "opv_wbr: down and up share a factor";
    }
    if (cfg->n_taps < 1 || wb_taps_per_phase(cfg->n_taps, cfg->up) > 1024) return "opv_wbr: n_taps outside 1..1024 per phase";
    if (cfg->n_channels < 1 || cfg->n_channels > 256) return "opv_wbr: n_channels outside 1..256";
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return "opv_wbr: out_shift outside 0..40";
    if (cfg->reserved != 0) return "opv_wbr: reserved must be 0";
    return nullptr;
}

int wbr_plan(const opv_wbr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why) {
    if (const char* bad = wbr_cfg_refusal(cfg)) return refuse(why, OPV_EINVAL, bad);
    if (!centre_hz || !taps || !inc_out) return refuse(why, OPV_EINVAL, "opv_wbr: null pointer");
    if (!wb_phase_gain_within(taps, cfg->n_taps, cfg->up, 1ll << 21)) return refuse(why, OPV_EINVAL, "opv_wbr: sum of |taps| of one phase exceeds 2^21");
    return wb_plan_increments(cfg->down, cfg->up, cfg->n_channels, centre_hz, inc_out, why, "opv_wbr: non-finite centre frequency",
                              "opv_wbr: centre frequency out of range");
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

// ---- the up-converter banks: |y| <= 65535 x 32768 < 2^31 over the taps of a phase, which licenses the kernels' int32
int wbtx_plan(const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why) {
    if (!cfg) return refuse(why, OPV_EINVAL, "opv_wbtx: null configuration");
    if (cfg->interp < 1 || cfg->interp > 16) return refuse(why, OPV_EINVAL, "opv_wbtx: interp outside 1..16");
    if (cfg->n_channels < 1 || cfg->n_channels > 256) return refuse(why, OPV_EINVAL, "opv_wbtx: n_channels outside 1..256");
    if (cfg->n_taps < 1 || cfg->n_taps > 1024) return refuse(why, OPV_EINVAL, "opv_wbtx: n_taps outside 1..1024");
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return refuse(why, OPV_EINVAL, "opv_wbtx: out_shift outside 0..40");
    if (!centre_hz || !taps || !inc_out) return refuse(why, OPV_EINVAL, "opv_wbtx: null pointer");
    if (!wb_phase_gain_within(taps, cfg->n_taps, cfg->interp, 65535)) return refuse(why, OPV_EINVAL, "opv_wbtx: sum of |taps| of one phase exceeds 65535");
    return wb_plan_increments(cfg->interp, 1, cfg->n_channels, centre_hz, inc_out, why, "opv_wbtx: non-finite centre frequency",
                              "opv_wbtx: centre frequency out of range");
}

const char* wbtxr_cfg_refusal(const opv_wbtxr_cfg* cfg) {
    if (!cfg) return "opv_wbtxr: null configuration";
    if (cfg->up < 1) return "opv_wbtxr: up below 1";
    if (cfg->down < cfg->up || cfg->down > 8192) return "opv_wbtxr: down outside up..8192";
    if ((int64_t)cfg->down > 32 * (int64_t)cfg->up) return "opv_wbtxr: down above 32 up";
    if (std::gcd(cfg->down, cfg->up) != 1) return "opv_wbtxr: down and up share a factor";
    if (cfg->n_taps < 1 || wb_taps_per_phase(cfg->n_taps, cfg->down) > kWbtxrMaxJ) return "opv_wbtxr: n_taps outside 1..64 per phase";
    if (cfg->n_channels < 1 || cfg->n_channels > 256) return "opv_wbtxr: n_channels outside 1..256";
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return "opv_wbtxr: out_shift outside 0..40";
    if (cfg->reserved != 0) return "opv_wbtxr: reserved must be 0";
    return nullptr;
}

int wbtxr_plan(const opv_wbtxr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why) {
    if (const char* bad = wbtxr_cfg_refusal(cfg)) return refuse(why, OPV_EINVAL, bad);
    if (!centre_hz || !taps || !inc_out) return refuse(why, OPV_EINVAL, "opv_wbtxr: null pointer");
    if (!wb_phase_gain_within(taps, cfg->n_taps, cfg->down, 65535)) return refuse(why, OPV_EINVAL, "opv_wbtxr: sum of |taps| of one phase exceeds 65535");
    return wb_plan_increments(cfg->down, cfg->up, cfg->n_channels, centre_hz, inc_out, why, "opv_wbtxr: non-finite centre frequency",
                              "opv_wbtxr: centre frequency out of range");
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

int wbtx_push_plan(const WbtxShape& shape, uint64_t n_before, const int16_t* const* d_in, size_t n_in, const int16_t* d_wide_out,
                   uint64_t* n_out, const char** why) {
    *n_out = 0;
    if (!d_in || !d_wide_out) return refuse(why, OPV_EINVAL, "opv_wbtx_push: null pointer");
    // ---- the kind's own limits, and the wide samples the push writes
    const uint32_t M = shape.down, U = shape.up;
    uint64_t n_wide;
    if (shape.kind == WbtxKind::Integer) {
        if ((uint64_t)n_in >= (1ull << 31) || (uint64_t)n_in * M >= (1ull << 31)) return refuse(why, OPV_EINVAL, "opv_wbtx_push: 2^31 or more wide samples in one push");
        n_wide = (uint64_t)n_in * M;
    } else {
        if ((uint64_t)n_in >= (1ull << 31)) return refuse(why, OPV_EINVAL, "opv_wbtx_push: 2^31 or more input samples in one push");
        if (n_before + n_in > kWbtxrMaxInputs) return refuse(why, OPV_ECAPACITY, "opv_wbtx_push: more than 2^50 input samples per channel");
        n_wide = wbtxr_outputs(M, U, n_before + n_in) - wbtxr_outputs(M, U, n_before);
        if (n_wide >= (1ull << 31)) return refuse(why, OPV_EINVAL, "opv_wbtx_push: 2^31 or more wide samples in one push");
    }
    if (n_in == 0) return OPV_OK;
    // ---- the pointers, for both kinds
    const uintptr_t out_lo = (uintptr_t)d_wide_out, out_hi = out_lo + (uintptr_t)(n_wide * 4);
    if (out_lo & 3u) return refuse(why, OPV_EINVAL, "opv_wbtx_push: output pointer must be 4-byte aligned");
    for (uint32_t k = 0; k < shape.K; ++k) {
        const uintptr_t lo = (uintptr_t)d_in[k], hi = lo + (uintptr_t)(n_in * 4);
        if (!lo) continue;
        if (lo & 3u) return refuse(why, OPV_EINVAL, "opv_wbtx_push: input pointer must be 4-byte aligned");
        if (lo < out_hi && out_lo < hi) return refuse(why, OPV_EINVAL, "opv_wbtx_push: the output overlaps an input");
    }
    *n_out = n_wide;
    return OPV_OK;
}
