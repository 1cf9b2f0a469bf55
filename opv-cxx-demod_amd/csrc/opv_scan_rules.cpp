// opv_scan_rules.cpp — see opv_scan_rules.h. Plain C++: no HIP, no device.
#include "opv_scan_rules.h"

#include <algorithm>
#include <cmath>
#include <vector>

#include "opv_wb_rules.h"

namespace {

int refuse(const char** why, int code, const char* text) {
    *why = text;
    return code;
}

typedef unsigned __int128 u128;

}  // namespace

const char* scan_cfg_refusal(const opv_scan_cfg* cfg) {
    if (!cfg) return "opv_scan: null configuration";
    switch (wbr_ratio_fault(cfg->down, cfg->up)) {
        case 1: return "opv_scan: up outside 1..1024";
        case 2: return "opv_scan: down outside up..32 up";
        case 3: return "opv_scan: down and up share a factor";
    }
    if (cfg->n_probes < 1 || cfg->n_probes > (int32_t)kScanMaxProbes) return "opv_scan: n_probes outside 1..1024";
    if (cfg->n_window < 1 || cfg->n_window > (int32_t)kScanMaxWindow) return "opv_scan: n_window outside 1..4096";
    if (cfg->hop < 1 || cfg->hop > 65536) return "opv_scan: hop outside 1..65536";
    if (cfg->n_avg < 1 || cfg->n_avg > 4096) return "opv_scan: n_avg outside 1..4096";
    if ((int64_t)(cfg->n_avg - 1) * cfg->hop + cfg->n_window > (int64_t)kScanMaxSpan) return "opv_scan: block span (n_avg - 1) hop + n_window exceeds 2^20";
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return "opv_scan: out_shift outside 0..40";
    if (cfg->ring_blocks < 1 || cfg->ring_blocks > 4096) return "opv_scan: ring_blocks outside 1..4096";
    return nullptr;
}

// |z| <= 2^21 x 32768 x 32767 x 2 < 2^52 over a segment, like a door's phase
int scan_plan(const opv_scan_cfg* cfg, const double* probe_hz, const int16_t* window, uint32_t* inc_out, const char** why) {
    if (const char* bad = scan_cfg_refusal(cfg)) return refuse(why, OPV_EINVAL, bad);
    if (!probe_hz || !window || !inc_out) return refuse(why, OPV_EINVAL, "opv_scan: null pointer");
    if (!wb_phase_gain_within(window, cfg->n_window, 1, 1ll << 21)) return refuse(why, OPV_EINVAL, "opv_scan: sum of |window| exceeds 2^21");
    return wb_plan_increments(cfg->down, cfg->up, cfg->n_probes, probe_hz, inc_out, why, "opv_scan: non-finite probe frequency",
                              "opv_scan: probe frequency out of range");
}

uint64_t scan_segments(const opv_scan_cfg* cfg, uint64_t n_wide_total) {
    const uint64_t Lw = (uint64_t)cfg->n_window;
    return n_wide_total < Lw ? 0 : (n_wide_total - Lw) / (uint64_t)cfg->hop + 1;
}

uint64_t scan_blocks(const opv_scan_cfg* cfg, uint64_t n_wide_total) { return scan_segments(cfg, n_wide_total) / (uint64_t)cfg->n_avg; }

ScanPush scan_push_plan(const opv_scan_cfg* cfg, uint64_t n_before, uint64_t n_new) {
    const uint64_t stride = (uint64_t)cfg->n_avg * (uint64_t)cfg->hop;    // samples from a block's start to the next one's (<= 2^28)
    const uint64_t n_after = n_before + n_new;                            // (the caller keeps N within 2^63: b1 x stride cannot wrap)
    ScanPush p;
    p.b0 = scan_blocks(cfg, n_before);
    p.b1 = scan_blocks(cfg, n_after);
    p.start = p.b0 * stride;
    const uint64_t next = p.b1 * stride;
    p.keep = n_after > next ? (uint32_t)(n_after - next) : 0u;            // block b1 is unfinished: fewer than its span
    return p;
}

ScanShape scan_shape(const opv_scan_cfg* cfg, uint64_t blocks) {
    const uint32_t A = (uint32_t)cfg->n_avg;
    ScanShape s;
    s.pgroups = ((uint32_t)cfg->n_probes + kScanLanes - 1) / kScanLanes;
    const uint64_t have = (blocks ? blocks : 1) * s.pgroups;
    uint64_t want = (kScanTargetGroups + have - 1) / have;                // runs per block that would reach the target
    if (want > A) want = A;
    s.run_len = (A + (uint32_t)want - 1) / (uint32_t)want;
    s.runs = (A + s.run_len - 1) / s.run_len;
    return s;
}

long scan_carriers(const uint64_t* row, int n_probes, double f0_hz, double step_hz, double half_width_hz, uint32_t ratio_q8,
                   opv_scan_carrier* out, size_t cap, const char** why) {
    if (n_probes < 1 || n_probes > (int)kScanMaxProbes) return refuse(why, OPV_EINVAL, "opv_scan_carriers: n_probes outside 1..1024");
    if (!row || (!out && cap)) return refuse(why, OPV_EINVAL, "opv_scan_carriers: null pointer");
    if (!std::isfinite(f0_hz) || !std::isfinite(step_hz) || !(step_hz > 0.0)) return refuse(why, OPV_EINVAL, "opv_scan_carriers: f0_hz / step_hz not finite, or step_hz not positive");
    if (!std::isfinite(half_width_hz) || half_width_hz < 0.0) return refuse(why, OPV_EINVAL, "opv_scan_carriers: half_width_hz not finite or negative");
    const int P = n_probes;
    // ---- the floor: the row's median
    std::vector<uint64_t> sorted(row, row + P);
    std::sort(sorted.begin(), sorted.end());
    const uint64_t floor = sorted[(size_t)P / 2];
    // ---- the boxes. (a W beyond the row reaches all of it from everywhere, like W = P: the double is cut there before it is an int)
    const double wd = std::ceil(half_width_hz / step_hz);
    const int W = wd >= (double)P ? P : wd < 1.0 ? 1 : (int)wd;
    std::vector<u128> prefix((size_t)P + 1, 0);
    for (int j = 0; j < P; ++j) prefix[(size_t)j + 1] = prefix[(size_t)j] + row[j];
    struct Cand {
        u128 box;
        int i;
    };
    std::vector<Cand> cands;
    for (int i = 0; i < P; ++i) {
        const int lo = i - W < 0 ? 0 : i - W, hi = i + W > P - 1 ? P - 1 : i + W;
        const u128 box = prefix[(size_t)hi + 1] - prefix[(size_t)lo];
        const u128 n_i = (u128)(hi - lo + 1);
        if (box * 256u > (u128)ratio_q8 * n_i * floor) cands.push_back({box, i});      // < 2^82 against < 2^107
    }
    std::sort(cands.begin(), cands.end(), [](const Cand& a, const Cand& b) { return a.box != b.box ? a.box > b.box : a.i < b.i; });
    // ---- the strongest first, none within 2 W of one taken; the centroid of the excess over the floor inside the box
    size_t n_out = 0;
    std::vector<int> taken;
    for (const Cand& cd : cands) {
        if (n_out >= cap) break;
        bool near = false;
        for (int t : taken) near = near || (cd.i > t ? cd.i - t : t - cd.i) <= 2 * W;
        if (near) continue;
        const int i = cd.i;
        const int lo = i - W < 0 ? 0 : i - W, hi = i + W > P - 1 ? P - 1 : i + W;
        double num = 0.0, den = 0.0;
        for (int j = lo; j <= hi; ++j) {
            const uint64_t e = row[j] > floor ? row[j] - floor : 0;
            num += (double)e * (double)(j - i);
            den += (double)e;
        }
        opv_scan_carrier& c = out[n_out++];
        c.centre_hz = f0_hz + ((double)i + (den > 0.0 ? num / den : 0.0)) * step_hz;
        c.excess = den;
        c.probe = i;
        c.reserved = 0;
        taken.push_back(i);
    }
    return (long)n_out;
}
