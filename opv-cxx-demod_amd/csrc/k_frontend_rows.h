// k_frontend_rows.h — what the two several-streams-per-wave mappings of the MSK front-end share word for word
// (k_frontend_x4.hip: a stream per DPP row, k_frontend_x16.hip: a stream per DPP quad; "row" below means either): the
// row-uniform carry of a stream with its load from OpvStream and its store back, the state of the demodulate() call a row
// is in with the scheduler that picks the next one, the soft value a lane holds until the next refill point, the batch
// quota of a row, and the tail of a symbol from the on-time sums P1..P4 to the hand-over of the previous sums. Each
// mapping keeps its lane geometry, its rings and refill rules, its taps, LO and gate accumulation, its reductions, the
// minimum of the quota over the wave and the loop's refill rhythm. Device-only; everything has internal linkage
// (k_frontend_common.h). k_frontend.hip is NOT a user: its scheduler (housekeeping, soft_advance, fo_settle) has another shape.
#pragma once
#include "k_frontend_common.h"

namespace {

struct RowTone { double soft, nsg; };   // soft value of one symbol and -1 / +1: tone 1 / tone 2 dominates (RowStream::tone)

// Every member is row-uniform and lives in VGPRs, replicated over the lanes of its row; rows run their own chunk schedule
// under exec masks.
struct RowStream {
    // ---- carry ----------------------------------------------------------------------------------
    double fo, tf, mu, fo_sum;
    PrevSums pv;
    uint32_t origin, n_avail, n_chunks, edge_ties, soft_bmask, cap_chunks;
    uint64_t n_soft, total_samples, cap_soft, soft_keep, n_bytes;
    int tail_done, overflow, stalled, eof;
    gbyte* soft_base;
    const gbyte* iq_bytes;
    double* chunk_log;
    // ---- call state -----------------------------------------------------------------------------
    bool done, in_call, first, last;
    uint32_t N, soft_off, soft_off0;
    double Nd, pos;
    // ---- held soft value ------------------------------------------------------------------------
    // Soft symbols are written four at a time: lane t < 4 of a row keeps the value of the symbol with
    // iter % 4 == t and stores it at the next refill point, right AFTER that point's s_waitcnt - a store
    // per symbol would put a fresh store in front of every vmcnt(0) and make the wave wait out its latency.
    double held;
    uint32_t held_off;   // (byte offset into the soft ring)
    bool held_valid;

    // `have`: the row carries a stream (idle rows read a valid record, start no call and never write)
    __device__ __forceinline__ void load(const OpvStream& st, bool have) {
        fo = st.freq_offset; tf = st.timing_freq; mu = st.mu; fo_sum = st.fo_sum;
        pv = PrevSums{st.p1r, st.p1i, st.p2r, st.p2i, st.x40c, st.x40s};
        origin = (uint32_t)st.origin;
        n_avail = (uint32_t)st.n_avail;
        n_soft = st.n_soft; total_samples = st.total_samples;
        n_chunks = st.n_chunks;
        tail_done = st.tail_done; overflow = st.overflow; stalled = 0;
        edge_ties = st.edge_ties;
        eof = st.eof;
        cap_soft = st.cap_soft;
        if (cap_soft > (1ull << 28)) overflow = 1;
        soft_keep = st.trk_next >= 24 ? st.trk_next - 24 : 0;
        if (st.trk_state != 0 && st.trk_anchor < soft_keep) soft_keep = st.trk_anchor;
        soft_bmask = (uint32_t)(cap_soft * 8u - 1u) & ~7u;
        soft_base = (gbyte*)st.soft;
        iq_bytes = (const gbyte*)st.iq;
        n_bytes = (uint64_t)n_avail * 4u;
        chunk_log = st.chunk_log;
        cap_chunks = st.cap_chunks;
        done = !have; in_call = false; first = false; last = false;
        N = 0; soft_off = 0; soft_off0 = 0; Nd = 0.0; pos = 0.0;
        held = 0.0; held_off = 0; held_valid = false;
    }

    // one lane of the row, at the end of the launch; dbg_t0 / dbg_r0: s_memtime / s_memrealtime at the kernel's start
    __device__ __forceinline__ void store(OpvStream& st, uint64_t dbg_t0, uint64_t dbg_r0) const {
        st.freq_offset = fo; st.timing_freq = tf; st.mu = mu;
        st.p1r = pv.a; st.p1i = pv.b; st.p2r = pv.c; st.p2i = pv.d; st.x40c = pv.x40c; st.x40s = pv.x40s;
        st.fo_sum = fo_sum;
        st.origin = origin; st.n_soft = n_soft; st.total_samples = total_samples;
        st.n_chunks = n_chunks; st.tail_done = tail_done; st.overflow = overflow;
        st.stalled = stalled; st.edge_ties = edge_ties;
        // where and at which clock the wave that carried this stream (and its wave-mates) ran (opv_tap_wave_info)
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        st.dbg_hw_id = hw; st.dbg_xcc_id = xcc;
        st.dbg_cycles = __builtin_amdgcn_s_memtime() - dbg_t0;
        st.dbg_ticks = __builtin_amdgcn_s_memrealtime() - dbg_r0;
    }

    __device__ __forceinline__ void flush_soft() {
        if (held_valid) *(gdouble*)(soft_base + held_off) = held;
        held_valid = false;
    }

    // ---- which demodulate() call comes next (ref :1026 / :1088 / :1173) ---------------------
    __device__ __forceinline__ void begin_call(const OpvGlobalCfg& cfg) {
        const uint32_t remaining = n_avail - origin;
        bool go = true;
        last = false;
        if (cfg.streaming) {
            if (remaining >= OPV_CHUNK) N = OPV_CHUNK;
            else if (eof && !tail_done && remaining > 0) { N = remaining; last = true; }
            else { if (eof) tail_done = 1; go = false; }
        } else {
            if (!eof || tail_done) go = false;
            else { N = n_avail; last = true; }
        }
        if (go && overflow) go = false;
        if (go && (n_soft - soft_keep) + (uint64_t)(N / 38u + 2u) > cap_soft) { stalled = 1; go = false; }  // back-pressure, see k_frontend.hip
        if (go) {
            in_call = true;
            first = true;
            Nd = (double)N;
            pos = mu;                                          // ref :217
            soft_off0 = ((uint32_t)n_soft * 8u) & soft_bmask;
            soft_off = soft_off0;
        } else {
            done = true;
        }
    }

    // the next symbol of the call exists (ref :221); otherwise the call ends (end_call)
    __device__ __forceinline__ bool has_symbol() const { return pos + 40.0 + 10.0 < Nd; }

    // ---- end of this demodulate() call (ref :318-328, :1067-1076); writer_lane: one lane of the row ----
    __device__ __forceinline__ void end_call(bool writer_lane) {
        const uint32_t nsym_call = ((soft_off - soft_off0) & soft_bmask) >> 3;
        const uint32_t used = (uint32_t)pos;
        mu = pos - (double)used;
        const uint32_t leftover = N - used;
        if (writer_lane) {
            double* c = chunk_log + 5 * (size_t)(n_chunks % cap_chunks);
            c[0] = fo; c[1] = tf; c[2] = mu; c[3] = (double)leftover; c[4] = (double)nsym_call;
        }
        ++n_chunks;
        n_soft += nsym_call;
        total_samples += N;
        origin += (leftover > 0u && leftover < N) ? used : N;
        in_call = false;
        if (last) { tail_done = 1; done = true; }
    }

    // Batch quota: as many symbols as this row can take without its end-of-call test, its first-symbol rules or an
    // out-of-range -o (pos advances by at most 42 samples per symbol). A row outside a call is a finished stream here (one
    // that could start a call has just done so and asks for 0): it sits the batch out under the exec mask, limiting nobody.
    __device__ __forceinline__ int quota() const {
        int krow = 0x7fffffff;
        if (in_call) {
            krow = 0;
            const double room = Nd - 51.0 - pos;
            if (!first && !(fabs(fo) > 2000.0) && room > 0.0) krow = (int)(room * (1.0 / 42.0));
        }
        return krow;
    }

    // ---- symbol tail, first half: on-time gate: soft value, dominant tone (ref :264-272) ----
    static __device__ __forceinline__ RowTone tone(double P1o, double P2o, double P3o, double P4o) {
        const double s1r_ = P1o + P2o, s1i_ = P3o - P4o;
        const double s2r_ = P1o - P2o, s2i_ = P3o + P4o;
        const double en1 = fma(s1r_, s1r_, s1i_ * s1i_);
        const double en2 = fma(s2r_, s2r_, s2i_ * s2i_);
        const double soft = en2 - en1;                      // ref :268
        const double nsg = mkd((dhi(soft) & (int)0x80000000) | 0x3ff00000, 0);  // -1 iff tone 1 dominates
        return RowTone{soft, nsg};
    }

    // ---- symbol tail, second half: from the early / late sums of the dominant tone (ref :271-280), reduced over the row by
    // the mapping, to the hand-over. Generic (here and in the mappings' symbol_body): with the tests the first symbols of a
    // call need (early gate before the chunk, no AFC on the first symbol, an out-of-range -o still in force). Fast: the same
    // statements without them - bit-identical where both apply (no contraction, no re-association) - for the batches.
    // x40c / x40s: X[40] = exp(j 40 d) of THIS symbol, for the next one's phase detector; atab: the angle table in LDS;
    // kgain: afc_alpha * symbol rate / 2 pi; keeps: this lane is the one of the row's four soft-log lanes that keeps this
    // symbol's value until the next flush.
    template <bool kGeneric>
    __device__ __forceinline__ void finish_symbol(double P1o, double P2o, double P3o, double P4o, double soft, double sg,
                                                  double Ere, double Eim, double Lre, double Lim, double x40c, double x40s,
                                                  const double* atab, double kgain, bool keeps) {
        const double ee = fma(Ere, Ere, Eim * Eim), el = fma(Lre, Lre, Lim * Lim);
        const double num = el - ee, den = el + ee + 1e-10;
        // ---- phase detector operands: dom * conj(prev) (ref :289-299, see k_frontend.hip) -----
        const double dr = fma(sg, P2o, P1o), di = fma(-sg, P4o, P3o);
        const double prs = fma(sg, pv.a, pv.b), pis = fma(sg, pv.c, -pv.d);
        const double ar = fma(dr, prs, di * pis), ai = fma(di, prs, -(dr * pis));
        const double cy = fma(ar, pv.x40c, ai * pv.x40s);   // Im z
        const double cx = fma(ar, pv.x40s, -(ai * pv.x40c)); // Re z
        // the angle without an octant fix-up (opv_atan2.h: opv_atan2_q): atan(|cy| / |cx|) = pi/4 + atan(q),
        // q = (|cy| - |cx|) / (|cy| + |cx|) in [-1, 1]
        const double sum = fabs(cx) + fabs(cy), dif = fabs(cy) - fabs(cx);
        // ---- the two divides on one reciprocal ------------------------------------------------
        const double dm = sum + 1e-100;                     // the guard against digital silence: IS sum unless sum is 0 (k_frontend.hip)
        const double tt = den * dm;
        double y = __builtin_amdgcn_rcp(tt);
        y = fma(fma(-tt, y, 1.0), y, y);                    // one Newton step (2^-24.4 -> 2^-48.7, scripts/microbench/rcp_accuracy.hip)
        const double iden = y * dm, idm = y * den;
        const double ratio = dif * idm;                     // good to 2^-48: 3.5e-15 rad on the angle
        // the angle's table row is requested here and used after the timing loop: with one wave per SIMD nothing else
        // covers the LDS round trip (the row index is in range on every path: |ratio| <= 1)
        // nearest expansion point k/128 by the 1.5 * 2^52 trick: the sum's low word is the row index k + 128
        const double kt = fma(ratio, 128.0, 6755399441055744.0 + 128.0);
        const double h = fma(kt - (6755399441055744.0 + 128.0), -1.0 / 128.0, ratio);   // |h| <= 1/256
        const double2* trow = reinterpret_cast<const double2*>(atab + (unsigned)dlo(kt) * 6u);
        const double2 c45 = trow[2], c23 = trow[1], c01 = trow[0];
        __builtin_amdgcn_sched_barrier(0);
        double ted = num * iden;
        ted = fma(fma(-den, ted, num), iden, ted);
        // ---- timing loop (ref :283-286, :313) ------------------------------------------------
        tf = clampd(fma(0.00001, ted, tf), -0.1, 0.1);
        const double adj = fma(0.005, ted, tf);   // |adj| <= 0.105: the reference's clamp to +/-2 (:286) cannot act, see k_frontend.hip
        double pos_next = pos + (40.0 + adj);
        if (keeps) { held = soft; held_off = soft_off; held_valid = true; }
        asm volatile("" : "+v"(pos_next), "+v"(tf), "+v"(held));   // (keeps these statements HERE: hipcc otherwise sinks them below the AFC block)
        __builtin_amdgcn_sched_barrier(0);
        // ---- AFC (ref :289-306): not on the first symbol of a call -------------------------------
        if (!kGeneric || !first) {
            double pd = fma(c45.y, h, c45.x);                   // degree 5: pi/4 + atan(q)
            pd = fma(pd, h, c23.y);
            pd = fma(pd, h, c23.x);
            pd = fma(pd, h, c01.y);
            pd = fma(pd, h, c01.x);
            const double sx = mkd((dhi(cx) & (int)0x80000000) | 0x3ff00000, 0);
            pd = fma(sx, pd, fma(-sx, 1.57079632679489661923, 1.57079632679489661923));
            pd = mkd((dhi(pd) & 0x7fffffff) | (dhi(cy) & (int)0x80000000), dlo(pd));
            if (sum == 0.0) {                                // digital silence on either side
                const double2 sp = silence_pd(dr, di, pv, soft < 0.0, fo_sum,
                                              (uint32_t)n_soft + (((soft_off - soft_off0) & soft_bmask) >> 3),
                                              P1o, P2o, P3o, P4o);
                pd = sp.x;
                edge_ties += (uint32_t)sp.y;
            }
            const double fo_used = fo;
            fo = clampd(fma(kgain, pd, fo), -2000.0, 2000.0);
            fo_sum += fo_used;
        } else {
            fo_sum += fo;
        }
        soft_off = (soft_off + 8u) & soft_bmask;
        pv.a = P1o; pv.b = P2o; pv.c = P3o; pv.d = P4o; pv.x40c = x40c; pv.x40s = x40s;
        pos = pos_next;
        first = false;
    }
};

}  // namespace
