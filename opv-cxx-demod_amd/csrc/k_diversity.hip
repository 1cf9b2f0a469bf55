// k_diversity.hip — receive diversity (include/opv_demod.h: opv_div): the stage between the trackers and the decoder that matches
// the frames of a group's branch streams and sums their payloads. Two kernels, enqueued by opv_div_round (opv_diversity.hip) behind
// the rounds launched so far; scale, decoder and link record of the combined payload follow from k_frame_decode.hip / k_frame_link.hip.
// No counterpart in the reference, which decodes every stream alone.
//
// k_div_match: one wave per group. The rule is opv_div_rules.h's (the host entry opv_div_match runs the same functions): lanes
// 0..B-1 each read their branch's view - cursor, next record, E_b off the tracker's carry - lane 0 decides and writes the meta
// record, the members' factors e_b and the group's counters. It runs from the group's cursors up to the free slots of the output
// ring and leaves the round's dec_from / n_frames for the kernels behind it. O(frames) work, a few hundred bytes per frame.
//
// k_div_combine: one workgroup of 256 threads per emitted frame (strided over the host's estimate, like k_frame_scale_wave and
// k_frame_decode, so that a released backlog is covered). payload[i] = e_b0 soft_b0[p_b0 + i], then + e_b soft_b[p_b + i] for the
// other summed members in ascending branch order: __dmul_rn / __dadd_rn, never contracted, so a numpy model reproduces the bits.
// Access: thread t takes i = t, t + 256, ...: every load and store instruction of a wave is 512 contiguous bytes of ONE ring (the
// soft rings are only 8-byte aligned at a payload's first symbol, so 8 bytes per lane; the wrap is the ring's mask on the index).
// All loads of a trip - up to eight branches - are requested before the first product is formed. Bytes: (B + 1) x 17 152 per
// frame, nothing reused, no LDS, no scratch: bandwidth-bound. 105 registers (the nine trips are unrolled, so a thread has up to 72
// loads in flight): four waves per SIMD.
#include <hip/hip_runtime.h>
#include <math.h>

#include "opv_device.h"
#include "opv_div_rules.h"

extern "C" __global__ __launch_bounds__(64) void k_div_match(OpvDivGroup* __restrict__ groups, const OpvStream* __restrict__ streams) {
    OpvDivGroup& g = groups[blockIdx.x];
    const int lane = threadIdx.x, B = g.n_branches;
    const bool mine = lane < B;
    const OpvStream* st = mine ? streams + g.stream[lane] : nullptr;
    // this lane's branch: the cursor (restarted where the host says so), what the ring has lost, E_b
    uint32_t cur = 0, n = 0, cap = 1, lost = 0;
    uint64_t earliest = OPV_DIV_ENDED;
    if (mine) {
        cur = g.cursor[lane];
        if (g.restart[lane]) { cur = g.restart[lane] - 1u; g.restart[lane] = 0u; }
        n = st->n_frames;
        cap = st->cap_frames;
        if (cur > n) cur = n;                                     // (a restart beyond what the stream holds: nothing to consume)
        lost = opv_div_skip_lost(n, cap, &cur);
        const int ended = st->tail_done && !(st->stalled & 2);
        earliest = opv_div_earliest_of(st->trk_collecting, st->trk_state, st->trk_anchor, st->trk_next, ended);
    }
#pragma unroll
    for (int off = 4; off > 0; off >>= 1) lost += __shfl_xor(lost, off, 64);   // (lanes 0..7 hold the branches)
    uint32_t n_frames = g.n_frames, softs_lost = 0;
    const uint32_t first = n_frames, popped = g.popped, ring = g.cap, window = g.window;
    int stalled = 0;
    for (;;) {
        OpvDivView v{0, earliest, mine && cur < n ? 1 : 0, 0};
        OpvFrameRec rec{};
        if (v.has) { rec = st->frec[cur % cap]; v.sym = rec.payload_sym; }
        OpvDivView all[OPV_DIV_MAX_BRANCHES];
#pragma unroll
        for (int b = 0; b < OPV_DIV_MAX_BRANCHES; ++b) {
            all[b].sym = __shfl(v.sym, b, 64); all[b].earliest = __shfl(v.earliest, b, 64); all[b].has = __shfl(v.has, b, 64); all[b].pad = 0;
        }
        uint64_t p0 = 0;
        uint32_t members = 0;
        if (!opv_div_decide(all, B, window, &p0, &members)) break;       // (wave-uniform: every lane decides on the same views)
        if (n_frames - popped >= ring) { stalled = 1; break; }           // a frame is final and the output ring is full: nothing consumed
        // the members: what each enters the sum with, in its own lane
        const bool member = mine && ((members >> lane) & 1u);
        double e = 0.0;
        int soft_gone = 0;
        if (member) {
            soft_gone = opv_div_soft_lost(rec.payload_sym, st->cap_soft, st->n_soft);
            if (!soft_gone) e = opv_div_factor(g.w[lane], g.normalise, st->fscale[cur % cap]);
            ++cur;
        }
        const uint32_t summed = (uint32_t)(__ballot(member && e != 0.0) & 0xFFu);
        softs_lost += (uint32_t)__popcll(__ballot(soft_gone != 0));
        const uint32_t slot = n_frames % ring;
        const bool sums = (summed >> lane) & 1u;
        int ok = 0;
        double q = 0.0;
        bool have_q = false;
#pragma unroll
        for (int b = 0; b < OPV_DIV_MAX_BRANCHES; ++b) {                  // OR of sync_ok, max of quality over the summed members, in branch order
            const int ob = __shfl(rec.sync_ok, b, 64);
            const double oq = __shfl(rec.quality, b, 64);
            if ((summed >> b) & 1u) {
                ok |= ob;
                if (!have_q || oq > q) q = oq;
                have_q = true;
            }
        }
        if (lane < OPV_DIV_MAX_BRANCHES) {
            g.meta[slot].payload_symbol[lane] = member ? rec.payload_sym : 0;
            g.factor[(size_t)slot * OPV_DIV_MAX_BRANCHES + lane] = sums ? e : 0.0;
        }
        if (lane == 0) {
            OpvDivMetaDev& m = g.meta[slot];
            m.members = members; m.summed = summed;
            m.viterbi_metric = INT32_MIN;                                 // "emitted, not decoded yet"
            m.sync_ok = ok != 0; m.sync_quality = have_q ? q : 0.0;
            g.metrics[slot] = INT32_MIN;
        }
        ++n_frames;
    }
    if (mine) g.cursor[lane] = cur;
    if (lane == 0) {
        g.dec_from = first; g.n_frames = n_frames;
        g.records_lost += lost; g.softs_lost += softs_lost; g.stalled = stalled;
    }
}

// grid = n_groups x per_group, flattened: frames dec_from + blockIdx.x % per_group, + per_group, ... of group blockIdx.x / per_group
extern "C" __global__ __launch_bounds__(256) void k_div_combine(const OpvDivGroup* __restrict__ groups, const OpvStream* __restrict__ streams,
                                                               uint32_t per_group) {
    const OpvDivGroup& g = groups[blockIdx.x / per_group];
    const uint32_t n_frames = g.n_frames, ring = g.cap;
    const int t = threadIdx.x;
    constexpr int kTrips = (OPV_CODED + 255) / 256;                      // 9 (the last one for threads < 96)
    for (uint32_t f = g.dec_from + blockIdx.x % per_group; f < n_frames; f += per_group) {
        const uint32_t slot = f % ring;
        const OpvDivMetaDev& m = g.meta[slot];
        const uint32_t summed = m.summed;
        double* __restrict__ out = g.payload + (size_t)slot * OPV_CODED;
        const double* soft[OPV_DIV_MAX_BRANCHES];
        uint32_t first[OPV_DIV_MAX_BRANCHES], mask[OPV_DIV_MAX_BRANCHES];
        double e[OPV_DIV_MAX_BRANCHES];
#pragma unroll
        for (int b = 0; b < OPV_DIV_MAX_BRANCHES; ++b) {
            const bool on = (summed >> b) & 1u;
            const OpvStream& st = streams[on ? g.stream[b] : g.stream[0]];
            soft[b] = st.soft; mask[b] = (uint32_t)(st.cap_soft - 1);
            first[b] = (uint32_t)m.payload_symbol[b];                     // the soft log is a power-of-two ring: the low 32 bits index it
            e[b] = g.factor[(size_t)slot * OPV_DIV_MAX_BRANCHES + b];
        }
#pragma unroll
        for (int k = 0; k < kTrips; ++k) {
            const int i = t + 256 * k;
            if (i < OPV_CODED) {
                double v[OPV_DIV_MAX_BRANCHES];
#pragma unroll
                for (int b = 0; b < OPV_DIV_MAX_BRANCHES; ++b)
                    if ((summed >> b) & 1u) v[b] = soft[b][(first[b] + (uint32_t)i) & mask[b]];
                double acc = 0.0;
                bool started = false;
#pragma unroll
                for (int b = 0; b < OPV_DIV_MAX_BRANCHES; ++b)
                    if ((summed >> b) & 1u) {
                        const double p = __dmul_rn(e[b], v[b]);
                        acc = started ? __dadd_rn(acc, p) : p;
                        started = true;
                    }
                out[i] = acc;                                             // (summed == 0: a zero payload, which the decoder drops)
            }
        }
    }
}
