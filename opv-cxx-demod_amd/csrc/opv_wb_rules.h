// opv_wb_rules.h — the rules of the four wideband converters (include/opv_demod.h: the integer and the rational front door, opv_wb_* /
// opv_wbr_*; the integer and the rational up-converter bank, opv_wbtx_* / opv_wbtxr_*), once each, in plain C++ (no HIP header: with
// opv_wb_rules.cpp it compiles with the host compiler like opv_stream_rules.cpp and opv_txb_rules.cpp, and a host-only test reaches
// it without a device): the LO table, the increments, the limits of each plan, the cap on a phase's tap gain, the output counts and
// where a push's first output sits, what refuses a transmit push, the tile of k_wbr_ddc and the phase-major tap table,
// and the LO schedule of a channel: a segment's phase and successor, what refuses a retune, pruning, the per-push device table.
// A plan or a push plan returns OPV_OK, or the refusal's code with *why set to its text.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/opv_demod.h"

constexpr uint32_t kWbrSpan = 4096;                      // wide samples a workgroup of k_wbr_ddc holds in LDS (= OPV_WB_SPAN, asserted in opv_wideband.hip)
constexpr uint32_t kWbrMaxTile = 256;                    // outputs per workgroup at most: one lane each
constexpr uint32_t kWbtxrTile = 256;                     // wide outputs per workgroup of k_wbtxr_duc: one lane each
constexpr uint32_t kWbtxrMaxJ = 64;                      // taps per phase at most
constexpr uint64_t kWbtxrMaxInputs = 1ull << 50;         // N at most: N M + U stays inside uint64 (M <= 2^13)

// ---- what all four kinds share (and, inside opv_wb_rules.cpp, the increment rule that ends every plan)
// Every phase p < stride (taps p, p + stride, ...) is a filter of its own: does the sum of |taps| of each stay within cap?
bool wb_phase_gain_within(const int16_t* taps, int64_t n_taps, int64_t stride, int64_t cap);
// tab[p * row_len + j] = taps[p + j stride] for j < J (0 where p + j stride >= n_taps, and from J on): stride x row_len entries
void wb_phase_table(const int16_t* taps, int64_t n_taps, uint32_t stride, uint32_t J, uint32_t row_len, int16_t* tab);
// the taps per phase of a rational kind, J = ceil(L / stride), and the row length of its table: J rounded up to a multiple of 4
inline uint32_t wb_taps_per_phase(int32_t n_taps, int32_t stride) { return (uint32_t)(((int64_t)n_taps + stride - 1) / stride); }
inline uint32_t wb_row_len(uint32_t J) { return (J + 3u) & ~3u; }
// A plan's last step: inc_out[k] = (uint32) llrint(centre_hz[k] / (2 168 000 x down / up) x 2^32), the refusals in the asking plan's words
int wb_plan_increments(int32_t down, int32_t up, int32_t n_channels, const double* centre_hz, uint32_t* inc_out, const char** why,
                       const char* not_finite, const char* out_of_range);

// ---- the LO schedule of a channel (include/opv_demod.h, "per-channel retune and Doppler ramps"), for all four kinds
// tri(d) = d (d - 1) / 2, the even factor halved first, modulo 2^64
inline uint64_t wb_tri(uint64_t d) { return (d & 1u) ? d * ((d - 1u) >> 1) : (d >> 1) * (d - 1u); }
// phi64(a) of a segment: phase + d inc + ramp tri(d) modulo 2^64, d = a - start
inline uint64_t wb_seg_phase(const opv_wb_seg& s, uint64_t a) {
    const uint64_t d = a - s.start;
    return s.phase + d * s.inc + (uint64_t)s.ramp * wb_tri(d);
}
// opv_wb_seg_next: OPV_OK with *out the segment that follows prev from `at` on, or OPV_EINVAL with *why set
int wb_seg_next(const opv_wb_seg* prev, int32_t down, int32_t up, uint64_t at, double centre_hz, double rate_hz_s, opv_wb_seg* out, const char** why);

// The schedules of an object's K channels. seg[k] is channel k's live list, oldest first, never empty; created[k] is set while
// seg[k][0] is the creation segment {0, 0, inc_k << 32, 0}, the only one that may be shorter than OPV_WB_TUNE_GAP.
struct WbSchedule {
    int32_t down = 1, up = 1;                             // the wide rate's pair: (decim, 1), (interp, 1) or the rational kind's own
    std::vector<uint32_t> inc;                            // inc_k of the plan
    std::vector<std::vector<opv_wb_seg>> seg;
    std::vector<uint8_t> created;
};
// every channel back to its creation schedule (and the first call: the object's creation)
void wb_sched_reset(WbSchedule& s, int32_t down, int32_t up, uint32_t K, const uint32_t* inc);
// true while no channel has anything but its creation segment: the object launches the unscheduled kernel
bool wb_sched_plain(const WbSchedule& s);
// drops every segment whose successor starts at or before `oldest`, the oldest absolute sample the object can still mix
void wb_sched_prune(WbSchedule& s, uint64_t oldest);
// opv_wb_retune / opv_wbtx_retune on an object whose next sample is A and whose oldest mixable sample is `oldest`: the whole batch
// or nothing. OPV_OK, or the refusal's code with *why set and s unchanged.
int wb_sched_retune(WbSchedule& s, uint64_t A, uint64_t oldest, int count, const opv_wb_tune* tunes, const char** why);
// opv_wb_segments: copies min(cap, count) segments of channel k, returns the count (OPV_EINVAL for a channel out of range)
int wb_sched_copy(const WbSchedule& s, int channel, opv_wb_seg* out, size_t cap);

// One channel's schedule as the kernels of ONE push read it. Local index j stands for absolute sample `origin + j`, j < 2^32:
// segment i serves local samples [start[i], start[i + 1]), and there phi64 = phase[i] + d inc[i] + ramp[i] tri(d) with
// d = j - start[i] < 2^32, so the device never needs more than the low 64 bits of a 32 x 64 and a 64 x 64 product. A segment that
// began before the origin is re-based to it (start 0, phase = phi64(origin), inc = inc + ramp d0: tri(d0 + j) = tri(d0) + j d0 +
// tri(j)); entries from the count on have start = 0xFFFFFFFF. start[] comes first and is 64 bytes: one scalar load finds the
// workgroup's segment.
struct OpvWbDevSched {
    uint32_t start[OPV_WB_TUNE_SEGS];
    uint64_t phase[OPV_WB_TUNE_SEGS];
    uint64_t inc[OPV_WB_TUNE_SEGS];
    int64_t ramp[OPV_WB_TUNE_SEGS];
};
// the table of a push: out[K], for local indices [0, reach) behind `origin` (reach < 2^32 - 1). Segments that begin at
// origin + reach or later are left out: the push cannot meet them.
void wb_sched_table(const WbSchedule& s, uint64_t origin, uint64_t reach, OpvWbDevSched* out);
constexpr uint32_t kWbSchedBack = 4096;                  // how far in front of a receive push's first sample its table's origin lies: a
                                                         // workgroup's span reaches back at most OPV_WB_SPAN samples (asserted in opv_wideband.hip)

// ---- the front doors
int wb_plan(const opv_wb_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why);
// the limits of a wide rate's pair (the rational door's, and the scan's): 0 if 1 <= up <= 1024, up <= down <= 32 up and the two share no
// factor; else which of the three fails (1: up, 2: down, 3: a common factor)
int wbr_ratio_fault(int32_t down, int32_t up);
// nullptr if cfg lies inside the limits, else why not (every refusal is OPV_EINVAL)
const char* wbr_cfg_refusal(const opv_wbr_cfg* cfg);
int wbr_plan(const opv_wbr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why);

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

// ---- the up-converter banks
int wbtx_plan(const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out, const char** why);
const char* wbtxr_cfg_refusal(const opv_wbtxr_cfg* cfg);
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

// An up-converter bank's kind and its ratio: down / up wide samples per input; the integer bank has down = interp, up = 1
enum class WbtxKind { Integer, Rational };
struct WbtxShape {
    WbtxKind kind;
    uint32_t down, up;
    uint32_t K;
};
// What opv_wbtx_push decides before anything is enqueued: OPV_OK with *n_out = the wide samples the push writes (n_in interp, or
// W(N + n_in) - W(N); 0 for n_in = 0: nothing to do), or a refusal. d_in[k] = 0 is an absent channel.
int wbtx_push_plan(const WbtxShape& shape, uint64_t n_before, const int16_t* const* d_in, size_t n_in, const int16_t* d_wide_out,
                   uint64_t* n_out, const char** why);
