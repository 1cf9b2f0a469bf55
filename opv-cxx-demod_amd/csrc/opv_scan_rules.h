// opv_scan_rules.h — the rules of the wideband scan (include/opv_demod.h, opv_scan_*), once each, in plain C++ (no HIP header: with
// opv_scan_rules.cpp it compiles with the host compiler like opv_wb_rules.cpp, and a host-only test or a sanitized stand-alone
// program reaches it without a device): the limits and the plan, the segment and block counts, what a push completes and what it
// carries on, the launch shape of k_scan_probe, and opv_scan_carriers. The increment rule and the limits of (down, up) are
// opv_wb_rules.h's.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/opv_demod.h"

constexpr uint32_t kScanMaxProbes = 1024;
constexpr uint32_t kScanMaxWindow = 4096;                // Lw at most: a segment's products live in the workgroup's LDS
constexpr uint32_t kScanMaxSpan = 1u << 20;              // (A - 1) H + Lw at most: bounds the carry
constexpr uint32_t kScanLanes = 256;                     // probes per workgroup of k_scan_probe: one lane each
constexpr uint32_t kScanTargetGroups = 2048;             // workgroups a push is cut into at least, where its segments allow

// nullptr if cfg lies inside the limits, else why not (every refusal is OPV_EINVAL)
const char* scan_cfg_refusal(const opv_scan_cfg* cfg);
int scan_plan(const opv_scan_cfg* cfg, const double* probe_hz, const int16_t* window, uint32_t* inc_out, const char** why);

// segs = N < Lw ? 0 : (N - Lw) / H + 1, and segs / A (cfg inside the limits)
uint64_t scan_segments(const opv_scan_cfg* cfg, uint64_t n_wide_total);
uint64_t scan_blocks(const opv_scan_cfg* cfg, uint64_t n_wide_total);
inline uint32_t scan_span(const opv_scan_cfg* cfg) { return (uint32_t)(cfg->n_avg - 1) * (uint32_t)cfg->hop + (uint32_t)cfg->n_window; }

// What a push of n_new samples behind N does: it completes blocks [b0, b1), the first of which starts at sample `start` of the
// object (which may lie in front of the push, inside the carry, or - with H > Lw - behind its first sample), and leaves `keep`
// samples for the next push: those from the start of block b1 on (0 if that start has not arrived yet). keep < the block span.
struct ScanPush {
    uint64_t b0, b1;
    uint64_t start;
    uint32_t keep;
};
ScanPush scan_push_plan(const opv_scan_cfg* cfg, uint64_t n_before, uint64_t n_new);

// The launch: a block's A segments are cut into `runs` runs of run_len (the last may be shorter), one workgroup per (run, group of
// kScanLanes probes); few blocks are cut finer so that the device still fills, many are not cut at all.
struct ScanShape {
    uint32_t run_len, runs, pgroups;
};
ScanShape scan_shape(const opv_scan_cfg* cfg, uint64_t blocks);

long scan_carriers(const uint64_t* row, int n_probes, double f0_hz, double step_hz, double half_width_hz, uint32_t ratio_q8,
                   opv_scan_carrier* out, size_t cap, const char** why);
