// opv_div_rules.cpp — the host-only entries of receive diversity: the matching rule of opv_div_rules.h over plain record lists,
// no device involved (tests/test_diversity_host.py holds it to tests/diversity_model.py). Plain C++, like opv_stream_rules.cpp.
#include "opv_div_rules.h"

extern "C" uint64_t opv_div_earliest(int32_t collecting, int32_t sync_state, uint64_t anchor_symbol, uint64_t next_symbol, int32_t ended) {
    return opv_div_earliest_of(collecting, sync_state, anchor_symbol, next_symbol, ended);
}

extern "C" long opv_div_match(int n_branches, uint32_t window, const opv_div_rec* const* recs, const uint32_t* n_recs, const uint64_t* earliest,
                              uint32_t* cursors, opv_div_frame* out, size_t cap) {
    if (!recs || !n_recs || !earliest || !cursors || (!out && cap)) return OPV_EINVAL;
    if (n_branches < 1 || n_branches > OPV_DIV_MAX_BRANCHES || window > OPV_DIV_MAX_WINDOW) return OPV_EINVAL;
    for (int b = 0; b < n_branches; ++b)
        if ((!recs[b] && n_recs[b]) || cursors[b] > n_recs[b]) return OPV_EINVAL;
    size_t n = 0;
    while (n < cap) {
        OpvDivView v[OPV_DIV_MAX_BRANCHES];
        for (int b = 0; b < n_branches; ++b) {
            v[b].has = cursors[b] < n_recs[b];
            v[b].sym = v[b].has ? recs[b][cursors[b]].payload_symbol : 0;
            v[b].earliest = earliest[b];
            v[b].pad = 0;
        }
        uint64_t p0 = 0;
        uint32_t members = 0;
        if (!opv_div_decide(v, n_branches, window, &p0, &members)) break;
        opv_div_frame& f = out[n++];
        f.anchor = p0;
        f.members = members;
        f.reserved = 0;
        for (int b = 0; b < OPV_DIV_MAX_BRANCHES; ++b) {
            const bool m = b < n_branches && ((members >> b) & 1u);
            f.payload_symbol[b] = m ? v[b].sym : 0;
            if (m) ++cursors[b];
        }
    }
    return (long)n;
}
