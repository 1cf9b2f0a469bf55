// opv_wideband.hip — the host half of the wideband front door (include/opv_demod.h, opv_wb_*): the object that carries the last
// L - 1 wide samples and the count N from push to push, and the push itself: every channel's output count is computed here, room
// is reserved in all K streams under push_enqueue's rules (opv_int_push_reserve) before anything is launched, then ONE k_wb_ddc
// launch on the context's copy stream writes all K streams. An object is of one of two kinds: the integer door (opv_wb_create:
// decim wide samples per output, k_wb_ddc) or the rational one (opv_wb_create_rational: down / up wide samples per output,
// k_wbr_ddc). They differ in how a push's outputs are counted and in the launch; staging, the destination-table ring, the
// reservation and the lifetime rules are the same code. Plans and every other rule that needs no device are opv_wb_rules.h's.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/opv_demod.h"
#include "opv_iq_format.h"
#include "opv_wb_internal.h"
#include "opv_wb_rules.h"

static_assert(kWbrSpan == OPV_WB_SPAN && kWbrMaxTile == OPV_WB_THREADS, "opv_wb_rules.h sizes k_wbr_ddc's tile for this span");
static_assert(kWbSchedBack == OPV_WB_SPAN && OPV_WB_TUNE_GAP == OPV_WB_SPAN, "a workgroup's span reaches no further back than a schedule table's origin, and meets at most two segments");

namespace {

constexpr int kTabSlots = 8;             // pushes whose destination tables may be in flight before the host waits for the oldest

}  // namespace

enum class WbKind { Integer, Rational };

struct opv_wb {
    opv_ctx* ctx = nullptr;
    WbKind kind = WbKind::Integer;
    opv_wb_cfg cfg{};                    // Integer
    opv_wbr_cfg rcfg{};                  // Rational
    uint32_t K = 0;
    uint32_t carry = 0;                  // wide samples carried from push to push: L - 1 (Integer), J - 1 (Rational)
    OpvCtxDoor door{};
    std::vector<int> streams;
    uint64_t n_total = 0;                // N: wide samples pushed so far
    uint32_t hist_len = 0;               // min(N, carry)
    int cur = 0;                         // which carry buffer holds the history
    int* d_hist[2] = {nullptr, nullptr};
    int16_t* d_lo = nullptr;
    void* d_taps = nullptr;              // Integer: h[L] widened to int32; Rational: the phase-major int16 table
    uint32_t* d_inc = nullptr;
    OpvStage stage;                      // pageable sources: the block is copied here first (grow-only)
    int** h_tab = nullptr;               // pinned: kTabSlots x K destination pointers, read in place by the kernel
    WbSchedule sched;                    // the LO schedule of every channel (opv_wb_retune); plain until the first retune
    OpvWbDevSched* h_sched = nullptr;    // pinned: kTabSlots x K schedule tables, a slot per push like h_tab's, read in place by the kernel
    hipEvent_t tab_ev[kTabSlots] = {};
    unsigned pushes = 0;
    uint32_t tile = 0, lpad = 0, rowlen = 0;
};

namespace {

// What both kinds of object are made of: the checks of the K streams, the object, its device memory and the uploads. `taps` is
// the kind's own tap table (taps_bytes of it), w_init sets the kind's fields before anything is allocated.
template <class Init>
int make_object(opv_wb** out, opv_ctx* ctx, const char* who, int K, uint32_t carry, const int* streams, const uint32_t* inc,
                const void* taps, size_t taps_bytes, Init w_init) {
    auto fail = [&](const char* what) {
        char text[160];
        snprintf(text, sizeof text, "%s: %s", who, what);
        return opv_int_fail(OPV_EINVAL, text);
    };
    OpvCtxDoor door;
    if (int r = opv_int_door(ctx, &door)) return r;
    {
        std::vector<char> seen((size_t)door.n_streams, 0);
        for (int k = 0; k < K; ++k) {
            const int s = streams[k];
            if (s < 0 || s >= door.n_streams) return fail("stream index out of range");
            if (seen[s]) return fail("a stream is named twice");
            if (door.shared->owned[s]) return fail("a stream is already fed by another wideband object");
            seen[s] = 1;
        }
    }
    opv_wb* w = new (std::nothrow) opv_wb;
    if (!w) return opv_int_fail(OPV_ENOMEM, who);
    w->ctx = ctx;
    w->door = door;
    w->K = (uint32_t)K;
    w->carry = carry;
    w_init(w);
    if (w->kind == WbKind::Rational) wb_sched_reset(w->sched, w->rcfg.down, w->rcfg.up, (uint32_t)K, inc);
    else wb_sched_reset(w->sched, w->cfg.decim, 1, (uint32_t)K, inc);
    int16_t lo[4096];
    opv_wb_lo_table(lo);
    auto undo = [&](hipError_t e, const char* what) { opv_wb_destroy(w); return opv_int_fail(OPV_EHIP, what, e); };
    HIPCHK_OR(undo, hipSetDevice(door.device));
    const size_t hist_bytes = (size_t)(carry ? carry : 1) * 4;
    HIPCHK_OR(undo, hipMalloc(&w->d_hist[0], hist_bytes));
    HIPCHK_OR(undo, hipMalloc(&w->d_hist[1], hist_bytes));
    HIPCHK_OR(undo, hipMalloc(&w->d_lo, sizeof lo));
    HIPCHK_OR(undo, hipMalloc(&w->d_taps, taps_bytes));
    HIPCHK_OR(undo, hipMalloc(&w->d_inc, (size_t)K * 4));
    HIPCHK_OR(undo, hipHostMalloc((void**)&w->h_tab, (size_t)kTabSlots * K * sizeof(int*), hipHostMallocDefault));
    HIPCHK_OR(undo, hipHostMalloc((void**)&w->h_sched, (size_t)kTabSlots * K * sizeof(OpvWbDevSched), hipHostMallocDefault));
    HIPCHK_OR(undo, hipMemcpy(w->d_lo, lo, sizeof lo, hipMemcpyHostToDevice));
    HIPCHK_OR(undo, hipMemcpy(w->d_taps, taps, taps_bytes, hipMemcpyHostToDevice));
    HIPCHK_OR(undo, hipMemcpy(w->d_inc, inc, (size_t)K * 4, hipMemcpyHostToDevice));
    w->streams.assign(streams, streams + K);
    for (int s : w->streams) door.shared->owned[s] = 1;
    *out = w;
    return OPV_OK;
}

}  // namespace

extern "C" int opv_wb_plan(const opv_wb_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out) {
    const char* why = nullptr;
    if (int r = wb_plan(cfg, centre_hz, taps, inc_out, &why)) return opv_int_fail(r, why);
    return OPV_OK;
}

extern "C" size_t opv_wb_outputs(const opv_wb_cfg* cfg, uint64_t n_wide_total) {
    if (!cfg || cfg->decim < 1) return 0;
    const uint64_t d = (uint64_t)cfg->decim;
    return (size_t)(n_wide_total / d + (n_wide_total % d ? 1 : 0));
}

extern "C" void opv_wb_destroy(opv_wb* w) {
    if (!w) return;
    (void)hipSetDevice(w->door.device);
    if (w->door.shared && w->door.shared->ctx_alive) {                  // (a context destroyed first waited for its copy stream itself)
        if (w->door.copy_stream) (void)hipStreamSynchronize(w->door.copy_stream);
        for (int s : w->streams) w->door.shared->owned[s] = 0;
    }
    for (auto& e : w->tab_ev)
        if (e) (void)hipEventDestroy(e);
    if (w->h_tab) (void)hipHostFree(w->h_tab);
    if (w->h_sched) (void)hipHostFree(w->h_sched);
    void* ptrs[] = {w->d_hist[0], w->d_hist[1], w->d_lo, w->d_taps, w->d_inc, w->stage.d};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete w;
}

extern "C" int opv_wb_create(opv_wb** out, opv_ctx* ctx, const opv_wb_cfg* cfg, const int* streams, const double* centre_hz, const int16_t* taps) {
    if (!out) return opv_int_fail(OPV_EINVAL, "opv_wb_create: null out");
    *out = nullptr;
    if (!ctx || !streams) return opv_int_fail(OPV_EINVAL, "opv_wb_create: null pointer");
    std::vector<uint32_t> inc(256);
    if (int r = opv_wb_plan(cfg, centre_hz, taps, inc.data())) return r;
    const int K = cfg->n_channels, L = cfg->n_taps, D = cfg->decim;
    std::vector<int> taps32((size_t)L);
    for (int t = 0; t < L; ++t) taps32[t] = taps[t];
    return make_object(out, ctx, "opv_wb_create", K, (uint32_t)(L - 1), streams, inc.data(), taps32.data(), (size_t)L * 4, [&](opv_wb* w) {
        w->kind = WbKind::Integer;
        w->cfg = *cfg;
        w->lpad = (uint32_t)((L - 1 + D - 1) / D * D);
        w->tile = (OPV_WB_SPAN - w->lpad) / (uint32_t)D;
        if (w->tile > OPV_WB_THREADS) w->tile = OPV_WB_THREADS;
        w->rowlen = w->tile + w->lpad / (uint32_t)D;                    // D * rowlen = tile * D + lpad <= OPV_WB_SPAN
    });
}

// ---- the rational door
extern "C" int opv_wbr_plan(const opv_wbr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out) {
    const char* why = nullptr;
    if (int r = wbr_plan(cfg, centre_hz, taps, inc_out, &why)) return opv_int_fail(r, why);
    return OPV_OK;
}

extern "C" size_t opv_wbr_outputs(const opv_wbr_cfg* cfg, uint64_t n_wide_total) {
    if (wbr_cfg_refusal(cfg)) return 0;
    return (size_t)wbr_outputs((uint32_t)cfg->down, (uint32_t)cfg->up, n_wide_total);
}

extern "C" int opv_wb_create_rational(opv_wb** out, opv_ctx* ctx, const opv_wbr_cfg* cfg, const int* streams, const double* centre_hz,
                                      const int16_t* taps) {
    if (!out) return opv_int_fail(OPV_EINVAL, "opv_wb_create_rational: null out");
    *out = nullptr;
    if (!ctx || !streams) return opv_int_fail(OPV_EINVAL, "opv_wb_create_rational: null pointer");
    std::vector<uint32_t> inc(256);
    if (int r = opv_wbr_plan(cfg, centre_hz, taps, inc.data())) return r;
    const uint32_t J = wb_taps_per_phase(cfg->n_taps, cfg->up), rowlen = wb_row_len(J);
    std::vector<int16_t> tab((size_t)cfg->up * rowlen);
    wb_phase_table(taps, cfg->n_taps, (uint32_t)cfg->up, J, rowlen, tab.data());
    return make_object(out, ctx, "opv_wb_create_rational", cfg->n_channels, J - 1, streams, inc.data(), tab.data(), tab.size() * 2, [&](opv_wb* w) {
        w->kind = WbKind::Rational;
        w->rcfg = *cfg;
        w->rowlen = rowlen;
        w->tile = wbr_tile((uint32_t)cfg->down, (uint32_t)cfg->up, rowlen);
    });
}

namespace {

using Src = OpvSrc;

// fmt != OPV_IQ_CS16 (a host block in another format): converted into the object's stage on the copy stream, then as a device push
int wb_push(opv_wb* w, const void* iq, size_t n_new, Src kind, bool wait, int fmt = OPV_IQ_CS16) {
    if (!w) return opv_int_fail(OPV_EINVAL, "opv_wb_push: null object");
    if (!w->door.shared->ctx_alive) return opv_int_fail(OPV_ESTATE, "opv_wb_push: the object's context has been destroyed");
    if (int r = opv_int_push_begin(w->ctx)) return r;
    if (n_new == 0) return OPV_OK;
    if (!iq) return opv_int_fail(OPV_EINVAL, "opv_wb_push: null IQ pointer");
    const bool typed = fmt != OPV_IQ_CS16;
    if (typed && ((uintptr_t)iq & (opv_iq_align_of(fmt) - 1)) != 0)
        return opv_int_fail(OPV_EINVAL, "opv_wb_push_fmt: the block is not aligned for its format (2 bytes for cs8 / cu8, 4 for cf32)");
    if (!typed && ((uintptr_t)iq & 3u) != 0) return opv_int_fail(OPV_EINVAL, "opv_wb_push: IQ pointer must be 4-byte aligned");
    if (n_new >= (1ull << 31)) return opv_int_fail(OPV_EINVAL, "opv_wb_push: more than 2^31 - 1 samples in one push");
    const uint32_t K = w->K;
    const bool rational = w->kind == WbKind::Rational;
    // ---- the push's outputs [r0, r1) by the kind's rule: ceil(N / D), or ceil(N U / M) with where output r0 sits (opv_wb_rules.h)
    WbrFirst first{};
    uint64_t r0, r1;
    if (rational) {
        const uint32_t M = (uint32_t)w->rcfg.down, U = (uint32_t)w->rcfg.up;
        first = wbr_first_output(M, U, w->n_total);
        r0 = first.r0;
        r1 = wbr_outputs(M, U, w->n_total + n_new);
    } else {
        const uint32_t D = (uint32_t)w->cfg.decim;
        r0 = (w->n_total + D - 1) / D;
        r1 = (w->n_total + n_new + D - 1) / D;
    }
    const uint32_t n_out = (uint32_t)(r1 - r0);
    // ---- the source as the device sees it (a staging buffer grown at most so far: nothing enqueued, nothing of the object's state changed)
    const int* src = nullptr;
    bool stage = false;
    OpvTypedSrc tsrc;
    if (typed) {
        if (int r = opv_int_source_fmt(iq, n_new, opv_iq_bytes_of(fmt), w->door.device, w->door.copy_stream, &w->stage, &tsrc)) return r;
        src = w->stage.d;
    } else if (int r = opv_int_source((const int16_t*)iq, n_new, kind, w->door.device, w->door.copy_stream, &w->stage, &src, &stage)) {
        return r;
    }
    // ---- this push's destination table: a slot of the pinned ring, free once the launch that read it last has finished
    const unsigned slot = w->pushes % kTabSlots;
    if (w->tab_ev[slot]) HIPCHK(hipEventSynchronize(w->tab_ev[slot]));
    else HIPCHK(hipEventCreateWithFlags(&w->tab_ev[slot], hipEventDisableTiming));
    // ---- what can refuse the push, before anything is launched: room in all K streams, or nothing changes
    std::vector<uint32_t> counts(K, n_out);
    std::vector<int*> dst(K);
    if (int r = opv_int_push_reserve(w->ctx, (int)K, w->streams.data(), counts.data(), dst.data())) return r;
    if (stage) HIPCHK(hipMemcpyAsync(w->stage.d, iq, n_new * 4, hipMemcpyHostToDevice, w->door.copy_stream));
    if (typed)
        if (int r = opv_int_convert_enqueue(iq, n_new, fmt, tsrc, &w->stage, w->door.copy_stream)) return r;
    int** tab = w->h_tab + (size_t)slot * K;
    std::memcpy(tab, dst.data(), (size_t)K * sizeof(int*));
    void* d_tab = nullptr;
    HIPCHK(hipHostGetDevicePointer(&d_tab, tab, 0));
    // ---- the LO: an object never retuned launches the unscheduled kernel; any other one this push's schedule tables, in the slot
    // beside its destinations (a retune between two asynchronous pushes changes the lists, never a table in flight)
    const uint64_t first_sample = rational ? w->rcfg.first_sample : w->cfg.first_sample;
    const bool tuned = !wb_sched_plain(w->sched);
    void* d_sched = nullptr;
    if (tuned) {
        OpvWbDevSched* st = w->h_sched + (size_t)slot * K;
        wb_sched_table(w->sched, first_sample + w->n_total - kWbSchedBack, (uint64_t)n_new + kWbSchedBack, st);
        HIPCHK(hipHostGetDevicePointer(&d_sched, st, 0));
    }
    // few output tiles (a short push, a large ratio): the channels are shared out over blockIdx.y so that the device still fills
    const uint32_t tiles = n_out ? (n_out + w->tile - 1) / w->tile : 1;
    uint32_t ky = tiles >= 512 ? 1 : (512 + tiles - 1) / tiles;
    if (ky > K) ky = K;
    const uint32_t kper = (K + ky - 1) / ky;
    ky = (K + kper - 1) / kper;
    OpvWbHead h{};
    h.src = src;
    h.hist_in = w->d_hist[w->cur];
    h.hist_out = w->d_hist[w->cur ^ 1];
    h.lo = w->d_lo;
    h.taps = w->d_taps;
    h.inc = w->d_inc;
    h.dst = (int* const*)d_tab;
    h.n_before = w->n_total;
    h.a0_lo = (uint32_t)(first_sample + w->n_total);
    h.n_new = (uint32_t)n_new;
    h.hist_len = w->hist_len;
    h.n_out = n_out;
    h.K = K; h.S = (uint32_t)(rational ? w->rcfg.out_shift : w->cfg.out_shift); h.kper = kper;
    if (rational) {
        OpvWbrArgs a{h};
        a.nrel0 = (uint32_t)first.n_rel;                                // (< n_new whenever n_out > 0; not read otherwise)
        a.p0 = first.phase;
        a.M = (uint32_t)w->rcfg.down; a.U = (uint32_t)w->rcfg.up; a.J = w->carry + 1;
        a.rowlen = w->rowlen; a.tile = w->tile;
        if (tuned) k_wbr_ddc_tuned<<<dim3(tiles, ky), OPV_WB_THREADS, 0, w->door.copy_stream>>>(a, (const OpvWbDevSched*)d_sched);
        else k_wbr_ddc<<<dim3(tiles, ky), OPV_WB_THREADS, 0, w->door.copy_stream>>>(a);
    } else {
        OpvWbArgs a{h};
        a.r0 = r0;
        a.D = (uint32_t)w->cfg.decim; a.L = (uint32_t)w->cfg.n_taps;
        a.tile = w->tile; a.lpad = w->lpad; a.rowlen = w->rowlen;
        if (tuned) k_wb_ddc_tuned<<<dim3(tiles, ky), OPV_WB_THREADS, 0, w->door.copy_stream>>>(a, (const OpvWbDevSched*)d_sched);
        else k_wb_ddc<<<dim3(tiles, ky), OPV_WB_THREADS, 0, w->door.copy_stream>>>(a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(w->tab_ev[slot], w->door.copy_stream));
    ++w->pushes;
    w->cur ^= 1;
    w->n_total += n_new;
    w->hist_len = w->n_total < (uint64_t)w->carry ? (uint32_t)w->n_total : w->carry;
    wb_sched_prune(w->sched, first_sample + w->n_total - w->hist_len);  // what no later push can mix any more
    return opv_int_push_end(w->ctx, wait);
}

}  // namespace

extern "C" int opv_wb_push(opv_wb* w, const int16_t* iq_wide, size_t n_wide) { return wb_push(w, iq_wide, n_wide, Src::Host, true); }
extern "C" int opv_wb_push_async(opv_wb* w, const int16_t* iq_wide, size_t n_wide) { return wb_push(w, iq_wide, n_wide, Src::Host, false); }
extern "C" int opv_wb_push_device(opv_wb* w, const int16_t* d_iq_wide, size_t n_wide) { return wb_push(w, d_iq_wide, n_wide, Src::Device, true); }

static int wb_push_fmt(opv_wb* w, int fmt, const void* wide, size_t n_wide, bool wait) {
    if (!opv_iq_align_of(fmt)) return opv_int_fail(OPV_EINVAL, "opv_wb_push_fmt: unknown sample format");
    return wb_push(w, wide, n_wide, Src::Host, wait, fmt);
}
extern "C" int opv_wb_push_fmt(opv_wb* w, int fmt, const void* wide, size_t n_wide) { return wb_push_fmt(w, fmt, wide, n_wide, true); }
extern "C" int opv_wb_push_fmt_async(opv_wb* w, int fmt, const void* wide, size_t n_wide) { return wb_push_fmt(w, fmt, wide, n_wide, false); }

extern "C" int opv_wb_flush(opv_wb* w) {
    if (!w) return opv_int_fail(OPV_EINVAL, "opv_wb_flush: null object");
    if (!w->door.shared->ctx_alive) return opv_int_fail(OPV_ESTATE, "opv_wb_flush: the object's context has been destroyed");
    for (int s : w->streams)
        if (int r = opv_flush(w->ctx, s)) return r;
    return OPV_OK;
}

// ---- the LO schedule (include/opv_demod.h, "per-channel retune and Doppler ramps"); the rules are opv_wb_rules.h's
extern "C" uint64_t opv_wb_seg_phase(const opv_wb_seg* seg, uint64_t a) { return seg ? wb_seg_phase(*seg, a) : 0; }

extern "C" int opv_wb_seg_next(const opv_wb_seg* prev, int32_t down, int32_t up, uint64_t at, double centre_hz, double rate_hz_s, opv_wb_seg* out) {
    const char* why = nullptr;
    if (int r = wb_seg_next(prev, down, up, at, centre_hz, rate_hz_s, out, &why)) return opv_int_fail(r, why);
    return OPV_OK;
}

// host only: the lists change, nothing is enqueued and nothing waited for; pushes in flight read the tables they were launched with
extern "C" int opv_wb_retune(opv_wb* w, int count, const opv_wb_tune* tunes) {
    if (!w) return opv_int_fail(OPV_EINVAL, "opv_wb_retune: null object");
    if (!w->door.shared->ctx_alive) return opv_int_fail(OPV_ESTATE, "opv_wb_retune: the object's context has been destroyed");
    const uint64_t A = (w->kind == WbKind::Rational ? w->rcfg.first_sample : w->cfg.first_sample) + w->n_total;
    const char* why = nullptr;
    if (int r = wb_sched_retune(w->sched, A, A - w->hist_len, count, tunes, &why)) return opv_int_fail(r, why);
    return OPV_OK;
}

extern "C" int opv_wb_segments(opv_wb* w, int channel, opv_wb_seg* out, size_t cap) {
    if (!w) return opv_int_fail(OPV_EINVAL, "opv_wb_segments: null object");
    const int n = wb_sched_copy(w->sched, channel, out, cap);
    return n < 0 ? opv_int_fail(OPV_EINVAL, "opv_wb_segments: channel out of range") : n;
}
