// opv_div_rules.h — the rules of receive diversity (include/opv_demod.h: opv_div), each written ONCE as a __host__ __device__
// function: k_div_match (k_diversity.hip) runs them on the device, opv_div_match (opv_div_rules.cpp) on the host with no device at
// all (tests/test_diversity_host.py), like the round rules (opv_round_rules.h) and the wideband rules (opv_wb_rules.h).
// Also the device-resident group (OpvDivGroup) that the kernels of k_diversity.hip, k_frame_decode.hip and k_frame_link.hip share.
//
// A group is B branch streams (1 <= B <= 8) of one context that carry the same transmission. Every branch has an ordered list of
// frame records and a cursor (its next unconsumed record). One decision of the rule:
//   anchor    p0 = the smallest payload_sym among the branches' next unconsumed records (a tie: the lowest branch, same p0);
//   finality  a branch WITHOUT an unconsumed record must be unable to release a payload that starts at or before p0 + W any more:
//             E_b > p0 + W, E_b its earliest possible future payload (opv_div_earliest_of); otherwise nothing is decided yet;
//   members   every branch whose next record starts within W of p0 (payload_sym - p0 <= W); those records are consumed.
// Frames are 2168 symbols apart and W <= 64, so a branch has at most one record inside the window. The decisions are a pure
// function of the complete record lists: E_b only delays a decision, it never changes one (a record that arrives later starts at
// E_b or behind it, and the rule waits while that could still be inside the window).
#pragma once
#include <stdint.h>

#include "../../include/opv_demod.h"   // OPV_DIV_MAX_BRANCHES, OPV_DIV_MAX_WINDOW, OPV_DIV_ENDED (E_b of a branch that will never release another frame)
#include "opv_device.h"

#if defined(__HIPCC__)
#define OPV_DIV_HD __host__ __device__
#else
#define OPV_DIV_HD
#endif

// what the rule sees of one branch at one moment
struct OpvDivView {
    uint64_t sym;        // payload_sym of the next unconsumed record (valid while has != 0)
    uint64_t earliest;   // E_b (used while has == 0)
    int32_t has;         // an unconsumed record exists
    int32_t pad;
};

// E_b off the tracker's carry, as k_sync_track.hip uses it: a pending payload starts at trk_anchor + 1; a HUNTING tracker
// examines windows that end at max(trk_next, 23) or later, and the payload starts behind the window; a LOCKED one checks its next
// sync word at trk_anchor + 2168. `ended`: the stream's EOF tail is done and its tracker has seen every soft symbol.
OPV_DIV_HD inline uint64_t opv_div_earliest_of(int32_t collecting, int32_t state, uint64_t anchor, uint64_t next, int32_t ended) {
    if (ended) return OPV_DIV_ENDED;
    if (collecting) return anchor + 1u;
    if (state == 0) return (next < (uint64_t)(OPV_SYNC_BITS - 1) ? (uint64_t)(OPV_SYNC_BITS - 1) : next) + 1u;
    return anchor + (uint64_t)OPV_FSYMS + 1u;
}

// One decision. Returns 1 with *p0 and the *members mask (bit b = branch b) when a group frame is final, 0 when no branch has a
// record or a branch could still join. Overflow-free: E_b > p0 + W is tested as E_b - p0 > W behind E_b > p0.
OPV_DIV_HD inline int opv_div_decide(const OpvDivView* v, int n_branches, uint32_t window, uint64_t* p0, uint32_t* members) {
    int anchor = -1;
    for (int b = 0; b < n_branches; ++b)
        if (v[b].has && (anchor < 0 || v[b].sym < v[anchor].sym)) anchor = b;
    if (anchor < 0) return 0;
    const uint64_t a = v[anchor].sym;
    uint32_t m = 0;
    for (int b = 0; b < n_branches; ++b) {
        if (v[b].has) {
            if (v[b].sym - a <= (uint64_t)window) m |= 1u << b;
        } else if (v[b].earliest != OPV_DIV_ENDED && (v[b].earliest <= a || v[b].earliest - a <= (uint64_t)window)) {
            return 0;
        }
    }
    *p0 = a;
    *members = m;
    return 1;
}

// A record ring of `cap` slots holds records [n - cap, n): a cursor behind that has lost the difference. Returns the loss.
OPV_DIV_HD inline uint32_t opv_div_skip_lost(uint32_t n, uint32_t cap, uint32_t* cursor) {
    const uint32_t behind = n - *cursor;
    if (behind <= cap) return 0u;
    *cursor = n - cap;
    return behind - cap;
}

// a payload that starts at symbol p is still whole in a soft ring of cap_soft symbols that has received n_soft
OPV_DIV_HD inline int opv_div_soft_lost(uint64_t p, uint64_t cap_soft, uint64_t n_soft) { return p + cap_soft < n_soft; }

// The weight a member enters the sum with: w_b, or w_b / fscale_b in normalised mode (one IEEE division). 0: matched, not summed
// (w_b == 0, or a scale that is not positive and finite).
OPV_DIV_HD inline double opv_div_factor(double w, int normalise, double fscale) {
    if (!(w > 0.0)) return 0.0;
    if (!normalise) return w;
    if (!(fscale > 0.0) || !(fscale <= 1.7976931348623157e308)) return 0.0;
    return w / fscale;
}

// ---- the device-resident half of one group (opv_diversity.hip owns it; k_div_match keeps its cursors and counters) ----
struct OpvDivMetaDev {               // == opv_div_meta (include/opv_demod.h), static_assert in opv_diversity.hip
    uint64_t payload_symbol[OPV_DIV_MAX_BRANCHES];
    uint32_t members, summed;
    int32_t viterbi_metric, sync_ok;
    double sync_quality;
};

struct OpvDivGroup {
    int32_t n_branches, normalise;
    uint32_t window, cap;                       // cap: slots of the output rings (the context's cap_frames)
    int32_t stream[OPV_DIV_MAX_BRANCHES];       // branch b -> stream of the context
    uint32_t cursor[OPV_DIV_MAX_BRANCHES];      // next unconsumed frame record of branch b
    uint32_t restart[OPV_DIV_MAX_BRANCHES];     // host -> device: cursor[b] = restart[b] - 1 where non-zero (reset / import of the branch)
    double w[OPV_DIV_MAX_BRANCHES];
    uint32_t n_frames, dec_from;                // group frames emitted so far; the first one of the round being run
    uint32_t popped;                            // host -> device: the consumer's cursor (opv_div_pop_frames)
    uint32_t records_lost, softs_lost;
    int32_t stalled;
    // output rings, frame f at slot f % cap
    OpvDivMetaDev* meta;                        // [cap]
    double* factor;                             // [cap][8]: e_b of the summed members
    double* payload;                            // [cap][2144]
    double* scale;                              // [cap]
    uint8_t* frames;                            // [cap][134]
    int32_t* metrics;                           // [cap]
    void* link;                                 // [cap] opv_link
};
