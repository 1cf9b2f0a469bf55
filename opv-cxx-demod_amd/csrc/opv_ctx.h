// opv_ctx.h — the context behind include/opv_demod.h as the files of the C-ABI shim see it (opv_capi.hip: life, opv_process, pops,
// taps; opv_push.hip: the serving path; opv_migrate.hip; opv_link.hip; opv_tx_device.hip; opv_tx_bank.hip; opv_rccl.hip). Internal: the wideband object does
// not see it (opv_wb_internal.h is its door).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <initializer_list>
#include <vector>

#include "../../include/opv_demod.h"
#include "opv_device.h"
#include "opv_div_rules.h"
#include "opv_wb_internal.h"

extern "C" __global__ void k_offset_search(OpvStream*, OpvGlobalCfg, const double*, uint32_t*);
extern "C" __global__ void k_tie_collect(const OpvStream*, const uint32_t*, uint32_t, uint32_t, uint32_t, OpvTieStage*);
extern "C" __global__ void k_tie_apply(OpvStream*, const OpvTieStage*, uint32_t, int);
extern "C" __global__ void k_msk_frontend_rb(OpvStream*, OpvGlobalCfg, int);
extern "C" __global__ void k_msk_frontend_rb_wg4(OpvStream*, OpvGlobalCfg, int);
extern "C" __global__ void k_msk_frontend_x4_wg4(OpvStream*, OpvGlobalCfg, int);
extern "C" __global__ void k_msk_frontend_x16(OpvStream*, OpvGlobalCfg, int);
extern "C" __global__ void k_msk_frontend_x16_wg4(OpvStream*, OpvGlobalCfg, int);
extern "C" __global__ void k_msk_frontend_x16_wg8(OpvStream*, OpvGlobalCfg, int);
extern "C" __global__ void k_coherent_frontend(OpvStream*, double, double);
extern "C" __global__ void k_sync_track(OpvStream*);
extern "C" __global__ void k_frame_scale(OpvStream*, uint32_t, uint32_t);
extern "C" __global__ void k_frame_scale_wave(OpvStream*, uint32_t);
extern "C" __global__ void k_frame_decode(OpvStream*, uint32_t);
extern "C" __global__ void k_payload_scale(const double*, uint32_t, double*);
extern "C" __global__ void k_decode_payloads(const double*, uint32_t, const double*, uint8_t*, int32_t*, int8_t*, int8_t*, uint8_t*);
extern "C" __global__ void k_frame_link(OpvStream*, opv_link*, uint32_t, uint32_t);
extern "C" __global__ void k_link_payloads(const double*, uint32_t, const double*, const uint8_t*, const int32_t*, opv_link*);
extern "C" __global__ void k_div_match(OpvDivGroup*, const OpvStream*);
extern "C" __global__ void k_div_combine(const OpvDivGroup*, const OpvStream*, uint32_t);
extern "C" __global__ void k_div_scale(OpvDivGroup*, uint32_t, uint32_t);
extern "C" __global__ void k_div_decode(OpvDivGroup*, uint32_t);
extern "C" __global__ void k_div_link(OpvDivGroup*, uint32_t);
extern "C" __global__ void k_stream_pack(const OpvMove*, uint32_t);
extern "C" __global__ void k_stream_unpack(OpvStream*, int32_t*, const OpvUnpackItem*, uint32_t, const OpvMove*, uint32_t);
extern "C" __global__ void k_channel(const int4*, int4*, uint64_t, double, double, double, uint64_t);
extern "C" __global__ void k_resample_clock(const int*, uint64_t, int*, uint64_t, double);
extern "C" __global__ void k_tx_encode(const uint8_t*, uint32_t, uint8_t*, uint8_t*);
extern "C" __global__ void k_tx_scan_frames(uint8_t*, uint32_t);
extern "C" __global__ void k_tx_expand_phases(const double2*, uint32_t, uint64_t, uint64_t, double2*);
extern "C" __global__ void k_tx_modulate(const uint8_t*, const uint8_t*, const double2*, uint64_t, uint64_t, int*, uint32_t*, uint64_t*, uint32_t, uint64_t, uint64_t, const uint8_t*);
struct OpvTxbEntry;
struct OpvTxbAmb;
extern "C" __global__ void k_txb_encode(const OpvTxbEntry*, uint32_t, uint32_t, uint8_t*, uint8_t*);
extern "C" __global__ void k_txb_scan(const OpvTxbEntry*, uint32_t, uint8_t*, uint8_t*);
extern "C" __global__ void k_txb_phases(const OpvTxbEntry*, uint32_t, uint32_t, const double2*, double2*);
extern "C" __global__ void k_txb_modulate(const OpvTxbEntry*, uint32_t, const uint8_t*, const uint8_t*, const double2*, uint32_t*, OpvTxbAmb*, uint32_t, uint64_t, uint64_t, const uint8_t*);

inline int fail(int code, const char* what, hipError_t e = hipSuccess) { return opv_int_fail(code, what, e); }   // sets opv_last_error, returns code (HIPCHK: opv_wb_internal.h)

// how a failed allocation is reported: OPV_EHIP with the runtime's text, or - where the caller gives `oom` - OPV_ENOMEM with that
inline int alloc_failed(hipError_t e, const char* what, const char* oom) {
    if (!oom) return fail(OPV_EHIP, what, e);
    (void)hipGetLastError();
    return fail(OPV_ENOMEM, oom);
}

// A grow-only buffer in device (or pinned host) memory: replaced - never shrunk - when `need` bytes exceed what it holds, after the
// streams that may still read it have been waited for. The caller names those and the new capacity (each buffer's own growth policy).
template <class T, bool kPinned = false>
struct GrowBuf {
    T* p = nullptr;
    size_t cap = 0;   // bytes
    int grow(size_t need, size_t new_cap, std::initializer_list<hipStream_t> wait_for, const char* oom = nullptr) {
        if (cap >= need) return OPV_OK;
        for (hipStream_t s : wait_for) HIPCHK(hipStreamSynchronize(s));
        if (p) HIPCHK(kPinned ? hipHostFree(p) : hipFree(p));
        p = nullptr;
        cap = 0;
        const hipError_t e = kPinned ? hipHostMalloc((void**)&p, new_cap, hipHostMallocDefault) : hipMalloc((void**)&p, new_cap);
        if (e != hipSuccess) { p = nullptr; return alloc_failed(e, kPinned ? "hipHostMalloc" : "hipMalloc", oom); }
        cap = new_cap;
        return OPV_OK;
    }
    ~GrowBuf() { if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p)); }   // (opv_destroy: behind its waits, on the context's device)
};

// What a context and its diversity objects (opv_diversity.hip) share, and what outlives whichever goes first - the arrangement of
// OpvWbShared. Created by the first opv_div_create: a context without a diversity object holds a null pointer.
struct OpvDivShared {
    std::vector<uint8_t> owned;       // [n_streams]: 1 while a live diversity object has the stream as a branch
    std::vector<uint32_t> epoch;      // [n_streams]: bumped by every opv_reset_stream / opv_import_streams of the stream ...
    std::vector<uint32_t> restart;    // ... which leaves the stream's new count of released frames here: where a group's cursor restarts
    uint64_t frames_budget = 0;       // sum of the frame budgets (round_frames) of the rounds launched: what a diversity round sizes its grids by
    bool ctx_alive = true;
};
struct OpvDivTie {                    // the context's end
    std::shared_ptr<OpvDivShared> p;
    ~OpvDivTie() { if (p) p->ctx_alive = false; }
    void restarted(int s, uint32_t n_frames) { if (p) { ++p->epoch[s]; p->restart[s] = n_frames; } }
    void launched(uint64_t fr) { if (p) p->frames_budget += fr; }
};

struct StreamIn {  // host -> device per-round update
    const int16_t* iq;
    uint64_t n_avail;
    int32_t eof;
    int32_t dirty;
    uint32_t frames_popped, events_popped;  // consumer cursors of the record rings
};

struct HostStream {
    int16_t* d_iq_owned = nullptr;  // push path buffer
    int16_t* d_iq_alt = nullptr;    // second buffer of the same size: compaction copies the retained tail across and swaps
    size_t iq_cap = 0;              // samples
    const int16_t* d_iq = nullptr;  // what the kernels read
    uint64_t n_avail = 0;
    int eof = 0;
    bool dirty = false;
    bool attached = false;
    bool search_seen = false;       // a round in which k_offset_search could run for this stream has been launched
    uint64_t last_round_avail = 0;
    uint32_t popped = 0;        // frame records already handed out
    uint32_t events_popped = 0;
    uint32_t events_dropped = 0;       // overwritten in the (lossy) event ring before they were read
    int32_t decoded = 0, perfect = 0;  // over popped frames (`decoded` / `perfect` of main(), ref :1053-1054)
    uint64_t soft_floor = 0;           // an imported stream (opv_import_streams): first soft symbol / chunk-log entry that travelled with it
    uint32_t chunk_floor = 0;
    // opv_tap_push_soft (parity tap): a stream is fed EITHER IQ or staged soft symbols between two resets, never both
    bool iq_seen = false;              // IQ has arrived since the last reset (push / attach / wideband / import)
    bool soft_tapped = false;          // staged soft symbols have
    uint64_t tap_fresh = 0;            // staged symbols no round has been launched for yet
};

// the host's half of a stream as opv_reset_stream leaves it: as created, but its device buffers stay
inline HostStream reset_host_stream(const HostStream& h) {
    HostStream n;
    n.d_iq = n.d_iq_owned = h.d_iq_owned;
    n.d_iq_alt = h.d_iq_alt;
    n.iq_cap = h.iq_cap;
    return n;
}

struct opv_ctx {
    int n_streams = 0;
    opv_cfg cfg{};
    hipStream_t stream = nullptr;       // kernels, in order
    hipStream_t copy_stream = nullptr;  // host -> device IQ of opv_push_iq: overlaps the kernels of the previous round
    OpvStream* d_streams = nullptr;
    StreamIn* d_in = nullptr;
    // per-round stream updates travel through pinned host memory (no host sync in opv_process):
    // kInSlots rounds may be in flight before the host has to wait for the oldest upload
    static constexpr int kInSlots = 4;
    StreamIn* h_in = nullptr;           // kInSlots x n_streams, pinned
    hipEvent_t in_ev[kInSlots] = {};
    int* h_stall = nullptr;             // kInSlots words, pinned: round r's "a stream ended stalled" (k_collect_counts), slot r % kInSlots
    hipEvent_t done_ev = nullptr;       // behind the last round's k_collect_counts
    unsigned round_no = 0;
    std::vector<OpvStream> mirror;  // host copy, refreshed by refresh()
    std::vector<OpvStream> initial; // as created (for reset)
    std::vector<HostStream> hs;
    // pooled logs
    double* d_soft = nullptr;
    OpvFrameRec* d_frec = nullptr;
    OpvEventRec* d_events = nullptr;
    double* d_chunks = nullptr;
    uint8_t* d_frames = nullptr;
    int32_t* d_metrics = nullptr;
    double* d_fscale = nullptr;
    int32_t* d_counts = nullptr;
    // the per-frame link report (opv_link.hip): [n_streams][cap_frames] records, allocated by the first opv_enable_link_report;
    // reaches k_frame_link as a kernel argument - a stream's carry (OpvStream) does not know it, so it does not migrate
    opv_link* d_link = nullptr;
    bool link_on = false;
    double* d_offs_wtab = nullptr;      // k_offset_search's moment weights: [40 taps][cos, sin][OPV_OFFS_TERMS]
    // offset-search ties are decided with the HOST's libm (opv_offset_host.cpp), in stream order: streams whose search could not
    // decide put themselves on d_tie_list ([0] = count, then indices); behind the search opv_process enqueues, per pass of
    // tie_slots streams, k_tie_collect -> a host function -> k_tie_apply (TieWork below), and the front-end behind those
    uint32_t* d_tie_list = nullptr;
    bool host_ties = false;             // the host's libm reproduces the pinned reference energy (probed at opv_create)
    bool tx_trust_libm = false;         // the host's sin / cos behave at the transmit NCOs' flat tops as k_tx_modulate.hip assumes (probed at opv_create)
    bool push_gather = true;            // opv_push_iq_batch moves pinned blocks with one gather kernel (else: one copy per block)
    uint32_t push_gather_blocks = 32;   // workgroups of that kernel (see push_deferred)
    bool tf_guard = false;              // OPV_FRONTEND_TF_GUARD: every demodulate() call keeps the timing clamp (k_frontend.hip)
    bool rb_fp64_ring = true;           // k_msk_frontend_rb in its fp64-ring shape (128 threads) while S <= n_cu
    int n_cu = 0;                       // the device's compute units (multiProcessorCount)
    struct TieWork {                    // what the host function gets: stable for the context's life (opv_destroy drains the stream first)
        OpvTieStage* stage = nullptr;   // pinned: header + tie_slots slots
        uint32_t slots = 0;
        std::atomic<uint64_t> decided{0};   // streams the host has decided so far (opv_offset_ties_decided_on_host)
        std::atomic<uint64_t> left{0};      // streams listed beyond what a round's passes stage: the device's decision stood (opv_offset_ties_left_to_device)
    } tie;
    std::vector<int> search_now;        // streams whose offset search can run in the round being enqueued
    // opv_push_iq_batch: the table of the gather kernel / of the batched compaction, in pinned memory (the kernels read it in place)
    GrowBuf<void, true> bulk_tab;
    // typed pushes (opv_push_iq_fmt and its kin): the raw copies of blocks k_push_convert cannot read in place (pageable memory,
    // another device's pinned memory), rewritten under the rule of bulk_tab's pairs half
    GrowBuf<char> push_stage;
    // opv_push_iq_batch_async: moves enqueued on the copy stream that no host wait has covered yet; opv_process orders its kernels
    // behind push_ev on the device, every other push entry point waits on the host first
    bool push_pending = false;
    hipEvent_t push_ev = nullptr;
    OpvWbTie wb;                        // which streams live wideband objects feed (opv_wideband.hip); outlives the context for them
    OpvDivTie div;                      // which streams are branches of live diversity objects (opv_diversity.hip); null until one is created
    // stream migration (opv_export_streams / opv_import_streams): device staging buffer + pinned tables of k_stream_pack.hip, grow-only
    GrowBuf<char> mig;
    GrowBuf<char, true> mig_tab;
    uint64_t cap_soft = 0;
    uint32_t cap_frames = 0, cap_events = 0, cap_chunks = 0;
    bool mirror_valid = false;
    // Back-pressure: a stream that paused in the last round (OpvStream.stalled) must be retried by the next
    // opv_process even if the caller pushed nothing new. Unknown (= true) from a launch until the next refresh().
    bool maybe_stalled = false;
    // device transmit chain: NCO phases at symbol starts (data-independent: expanded once per context and run length from
    // the build-time checkpoint table, shared by every stream modulated afterwards) + grow-only scratch
    GrowBuf<double> tx_ckpt;             // checkpoints uploaded so far, 2 doubles each
    size_t tx_ckpt_have = 0;
    GrowBuf<double> tx_phases;           // (ph1, ph2) at every symbol start
    size_t tx_phases_have = 0;           // symbols
    GrowBuf<uint8_t> tx_scratch;         // one allocation: [frames][134], one code byte per symbol, per-frame parity / prefix (opv_tx_modulate_device)
    uint32_t* d_tx_cnt = nullptr;        // ambiguous-sample counter + list
    uint64_t* d_tx_list = nullptr;
    // flat tops (k_tx_modulate.hip): symbols [tx_flat_lo, tx_flat_hi) are decided by a bit per tone made with the host's libm;
    // d_tx_flat holds them for [tx_flat_lo, tx_flat_have)
    GrowBuf<uint8_t> tx_flat;
    uint64_t tx_flat_lo = ~0ull, tx_flat_hi = ~0ull, tx_flat_have = 0;
    const char* last_frontend = "";   // kernel the last opv_process launched for the front-end (opv_frontend_kernel)
    int frontend = 0;  // opv_set_frontend: 0 = by stream count, else 1, 4 or 16 streams per wave (opv_round_rules.h: frontend_kernel)
    bool timing = false;
    bool timing_valid = false;
    hipEvent_t ev[8] = {};

    // Host copies of the record pools (frames, metrics, frame records, events), fetched once per round
    // with four copies for ALL streams instead of three or four small copies per stream and pop: a
    // server popping 256 live streams spent 10 ms per 40 ms round in those copies. Pools above
    // kPoolMirrorMax (big offline captures) are read per stream as before.
    static constexpr size_t kPoolMirrorMax = 64u << 20;
    std::vector<uint8_t> m_frames;
    std::vector<int32_t> m_metrics;
    std::vector<OpvFrameRec> m_frec;
    std::vector<OpvEventRec> m_events;
    unsigned mirror_epoch = 0, pools_epoch = ~0u;
    std::vector<opv_link> m_link;       // the link report's ring, fetched by opv_pop_frames_link (opv_link.hip) once per mirror_epoch
    unsigned link_epoch = ~0u;

    int refresh() {
        if (mirror_valid) return OPV_OK;
        HIPCHK(hipSetDevice(cfg.device));       // (every pop / state / tap comes through here: a host with contexts on several GPUs)
        HIPCHK(hipStreamSynchronize(stream));
        HIPCHK(hipMemcpy(mirror.data(), d_streams, sizeof(OpvStream) * n_streams, hipMemcpyDeviceToHost));
        mirror_valid = true;
        ++mirror_epoch;
        maybe_stalled = false;
        for (const OpvStream& m : mirror) maybe_stalled |= m.stalled != 0;
        return OPV_OK;
    }
    size_t pool_bytes() const {
        const size_t S = (size_t)n_streams;
        return S * ((size_t)cap_frames * (OPV_FB + sizeof(int32_t) + sizeof(OpvFrameRec)) + (size_t)cap_events * sizeof(OpvEventRec));
    }
    // after refresh(): bring the pools over if they are small enough; returns whether host views exist
    int ensure_pools(bool* have) {
        *have = false;
        if (pool_bytes() > kPoolMirrorMax) return OPV_OK;
        if (pools_epoch != mirror_epoch) {
            const size_t S = (size_t)n_streams;
            m_frames.resize((size_t)OPV_FB * cap_frames * S);
            m_metrics.resize((size_t)cap_frames * S);
            m_frec.resize((size_t)cap_frames * S);
            m_events.resize((size_t)cap_events * S);
            HIPCHK(hipMemcpy(m_frames.data(), d_frames, m_frames.size(), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(m_metrics.data(), d_metrics, m_metrics.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(m_frec.data(), d_frec, m_frec.size() * sizeof(OpvFrameRec), hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(m_events.data(), d_events, m_events.size() * sizeof(OpvEventRec), hipMemcpyDeviceToHost));
            pools_epoch = mirror_epoch;
        }
        *have = true;
        return OPV_OK;
    }
    // host address of a device pointer into one of the mirrored pools (nullptr if it is not one)
    const void* host_view(const void* d) const {
        auto in = [&](const void* base, size_t bytes) { return (const char*)d >= (const char*)base && (const char*)d < (const char*)base + bytes; };
        if (in(d_frames, m_frames.size())) return m_frames.data() + ((const char*)d - (const char*)d_frames);
        if (in(d_metrics, m_metrics.size() * sizeof(int32_t))) return (const char*)m_metrics.data() + ((const char*)d - (const char*)d_metrics);
        if (in(d_frec, m_frec.size() * sizeof(OpvFrameRec))) return (const char*)m_frec.data() + ((const char*)d - (const char*)d_frec);
        if (in(d_events, m_events.size() * sizeof(OpvEventRec))) return (const char*)m_events.data() + ((const char*)d - (const char*)d_events);
        return nullptr;
    }
};

inline int check_stream(opv_ctx* c, int s) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (s < 0 || s >= c->n_streams) return fail(OPV_EINVAL, "stream index out of range");
    return OPV_OK;
}

// the context's device made current, and moves of an opv_push_iq_batch_async still under way waited for: every other push
// entry point (and reset / export / import) begins with this
inline int settle_pushes(opv_ctx* c) {
    HIPCHK(hipSetDevice(c->cfg.device));
    if (c->push_pending) {
        HIPCHK(hipStreamSynchronize(c->copy_stream));
        c->push_pending = false;
    }
    return OPV_OK;
}

// opv_link.hip: the link report's launch behind the decoder (nothing while the report is off), and its records of streams
// [lo, hi) zeroed in stream order (nothing while the ring does not exist) - what opv_reset_stream and opv_import_streams do to a slot
void link_launch(opv_ctx* c, uint64_t fr);
int link_clear(opv_ctx* c, int lo, int hi);
bool opv_tx_libm_flat_tops_as_assumed();   // opv_tx_device.hip: the probe behind opv_ctx::tx_trust_libm
// opv_tx_device.hip: the context's NCO checkpoints, flat-top zone limits and flat bits brought up to a run of nsym symbols (the
// context's device current); what opv_tx_modulate_device and a transmit bank's round (opv_tx_bank.hip) both start with
int opv_tx_prepare_run(opv_ctx* c, size_t nsym);
// a stream's staging buffer (which = 0) or its second one (1: compaction's target), allocated at first use: max_samples samples +
// slack for whole-tile reads (opv_push.hip). `oom`: the refusal is OPV_ENOMEM with that text instead of OPV_EHIP.
int ensure_iq_buffer(opv_ctx* c, HostStream& h, int which, const char* oom = nullptr);
