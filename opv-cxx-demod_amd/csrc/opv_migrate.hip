// opv_migrate.hip — stream migration behind the C ABI: a live stream out of one context and into another (no counterpart in the
// reference, whose streams are processes: SURVEY.md §5 "Checkpoint / resume: none"). The blob's format, its checks and the table
// of a stream's segments are plain C++ (opv_stream_rules.h); here: the plan of an export, the two launches, an imported slot's host half.
#include <climits>
#include <cstring>

#include "opv_ctx.h"
#include "opv_stream_rules.h"

namespace {
// grow-only: the device staging buffer and the pinned table (both idle here: every migration call ends with a wait for the stream)
int mig_buffers(opv_ctx* c, size_t dev_bytes, size_t tab_bytes) {
    if (int r = c->mig.grow(dev_bytes, dev_bytes + dev_bytes / 4 + 65536, {c->stream}, "stream migration: device staging buffer")) return r;
    return c->mig_tab.grow(tab_bytes, tab_bytes + tab_bytes / 4 + 65536, {c->stream}, "stream migration: pinned table");
}

unsigned mig_grid(size_t items) { return (unsigned)(items < 1 ? 1 : items > 4096 ? 4096 : items); }

// under opv_enable_timing a migration call brackets its device work (copy + kernel) like a round's first kernel: opv_kernel_times [0]
int mig_time(opv_ctx* c, bool end) {
    if (!c->timing) return OPV_OK;
    if (!end) { HIPCHK(hipEventRecord(c->ev[0], c->stream)); return OPV_OK; }
    for (int k = 1; k < 8; ++k) HIPCHK(hipEventRecord(c->ev[k], c->stream));
    c->timing_valid = true;
    return OPV_OK;
}

// what an export of `streams` carries, from the context as it is after opv_push_wait + opv_sync; *payload = bytes of staging needed
int plan_export(opv_ctx* c, int count, const int* streams, std::vector<BlobEntry>* ents, uint64_t* payload) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (count < 0 || (count > 0 && !streams)) return fail(OPV_EINVAL, "opv_export_streams: bad arguments");
    for (int i = 0; i < count; ++i)
        if (streams[i] < 0 || streams[i] >= c->n_streams) return fail(OPV_EINVAL, "opv_export_streams: stream index out of range");
    if (int r = settle_pushes(c)) return r;
    HIPCHK(hipStreamSynchronize(c->copy_stream));
    c->mirror_valid = false;                               // (a refresh that also waits for whatever a caller enqueued on the stream)
    if (int r = c->refresh()) return r;
    ents->assign((size_t)count, BlobEntry{});
    uint64_t total = 0;
    for (int i = 0; i < count; ++i) {
        const HostStream& h = c->hs[streams[i]];
        BlobEntry& e = (*ents)[i];
        OpvStream st = c->mirror[streams[i]];
        if (st.overflow) return fail(OPV_ESTATE, "opv_export_streams: the stream is in an error state (opv_pop_frames reports it)");
        if (h.soft_tapped) return fail(OPV_ESTATE, "opv_export_streams: the stream holds staged soft symbols (opv_tap_push_soft, a parity tap)");
        if (st.n_frames - h.popped > st.cap_frames) return fail(OPV_ESTATE, "opv_export_streams: more unpopped frames than the ring holds");
        // IQ: from the point compaction keeps up to everything pushed, processed or not; indices re-based like there
        const uint64_t keep = h.d_iq ? iq_keep(st.origin) : 0;
        uint64_t n_avail = h.d_iq ? h.n_avail : 0;
        e.last_round_avail = h.last_round_avail;
        iq_rebase(keep, &n_avail, &e.last_round_avail, &st);
        e.seg_n[SEG_IQ] = st.n_avail = n_avail;
        if (e.last_round_avail > st.n_avail) e.last_round_avail = st.n_avail;
        e.soft_first = soft_tail_first(st);
        e.seg_n[SEG_SOFT] = st.n_soft - e.soft_first;
        e.popped = h.popped;
        e.seg_n[SEG_FREC] = e.seg_n[SEG_FRAMES] = e.seg_n[SEG_METRICS] = e.seg_n[SEG_FSCALE] = st.n_frames - h.popped;
        e.events_popped = h.events_popped;
        e.events_dropped = h.events_dropped;
        if (st.n_events - e.events_popped > st.cap_events) {     // lossy ring, as opv_pop_events accounts for it
            e.events_dropped += (st.n_events - e.events_popped) - st.cap_events;
            e.events_popped = st.n_events - st.cap_events;
        }
        e.events_first = e.events_popped;
        e.seg_n[SEG_EVENTS] = st.n_events - e.events_first;
        e.seg_n[SEG_CHUNKS] = st.n_chunks < st.cap_chunks ? st.n_chunks : st.cap_chunks;
        if (st.n_chunks - (uint32_t)e.seg_n[SEG_CHUNKS] < h.chunk_floor) e.seg_n[SEG_CHUNKS] = st.n_chunks - h.chunk_floor;
        e.chunks_first = st.n_chunks - (uint32_t)e.seg_n[SEG_CHUNKS];
        e.decoded = h.decoded;
        e.perfect = h.perfect;
        e.eof = h.eof;
        e.search_seen = h.search_seen ? 1 : 0;
        st.eof = h.eof;
        st.frames_popped = e.popped;
        st.events_popped = e.events_popped;
        st.iq = nullptr; st.soft = nullptr; st.frec = nullptr; st.events = nullptr; st.chunk_log = nullptr;
        st.frames = nullptr; st.metrics = nullptr; st.fscale = nullptr;
        e.st = st;
        e.off = total;
        uint64_t o = 0;
        for (int k = 0; k < SEG_N; ++k) { e.seg_off[k] = o; o += up16(e.seg_n[k] * kSegElem[k]); }
        e.len = o;
        total += o;
    }
    *payload = total;
    return OPV_OK;
}

}  // namespace

extern "C" size_t opv_export_size(opv_ctx* c, int count, const int* streams) {
    std::vector<BlobEntry> ents;
    uint64_t payload = 0;
    if (plan_export(c, count, streams, &ents, &payload) != OPV_OK) return 0;
    return (size_t)(blob_payload_off(count) + payload);
}

extern "C" long opv_export_streams(opv_ctx* c, int count, const int* streams, void* blob, size_t cap) {
    std::vector<BlobEntry> ents;
    uint64_t payload = 0;
    if (int r = plan_export(c, count, streams, &ents, &payload)) return r;
    if (!blob) return fail(OPV_EINVAL, "opv_export_streams: null blob");
    BlobHeader h{};
    h.magic = kBlobMagic;
    h.version = kBlobVersion;
    h.sizeof_stream = sizeof(OpvStream);
    h.sizeof_header = sizeof(BlobHeader);
    h.sizeof_entry = sizeof(BlobEntry);
    h.streaming = c->cfg.streaming;
    h.coherent = c->cfg.coherent;
    h.have_init_offset = c->cfg.have_init_offset;
    h.init_offset_hz = c->cfg.have_init_offset ? c->cfg.init_offset_hz : 0.0;
    h.pll_bw_hz = c->cfg.coherent ? c->cfg.pll_bw_hz : 0.0;
    h.count = (uint32_t)count;
    h.payload_off = blob_payload_off(count);
    h.payload_bytes = payload;
    h.total_bytes = h.payload_off + payload;
    if (h.total_bytes > cap) return fail(OPV_ECAPACITY, "opv_export_streams: blob buffer too small (opv_export_size)");
    // every ring segment of every stream un-wrapped into the staging buffer by ONE launch, then ONE copy to the host
    std::vector<OpvMove> mv;
    if (int r = mig_buffers(c, (size_t)payload, 0)) return r;
    for (int i = 0; i < count; ++i) {
        const BlobEntry& e = ents[i];
        const HostStream& hs = c->hs[streams[i]];
        const OpvStream& m = c->mirror[streams[i]];
        BlobSegment seg[SEG_N];
        blob_segments(e, m, (const char*)hs.d_iq + (e.st.iq_base - m.iq_base) * 4, seg);   // (the IQ tail: behind what compaction would drop)
        for (int k = 0; k < SEG_N; ++k) segment_moves(&mv, e, k, seg[k], c->mig.p + e.off, false);
    }
    if (int r = mig_buffers(c, (size_t)payload, mv.size() * sizeof(OpvMove))) return r;
    char* out = (char*)blob;
    std::memset(out, 0, (size_t)h.payload_off);
    std::memcpy(out, &h, sizeof h);
    if (count) std::memcpy(out + sizeof h, ents.data(), (size_t)count * sizeof(BlobEntry));
    if (payload) {
        std::memcpy(c->mig_tab.p, mv.data(), mv.size() * sizeof(OpvMove));
        void* d_tab = nullptr;
        HIPCHK(hipHostGetDevicePointer(&d_tab, c->mig_tab.p, 0));
        if (int r = mig_time(c, false)) return r;
        // (the padding between segments is never written by a move: cleared, so that the same state gives the same bytes)
        HIPCHK(hipMemsetAsync(c->mig.p, 0, (size_t)payload, c->stream));
        k_stream_pack<<<mig_grid(mv.size()), 256, 0, c->stream>>>((const OpvMove*)d_tab, (uint32_t)mv.size());
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(out + h.payload_off, c->mig.p, (size_t)payload, hipMemcpyDeviceToHost, c->stream));
        if (int r = mig_time(c, true)) return r;
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    // a frame that has been released but not decoded (cannot happen after opv_process) would lose its payload's claim on the soft tail
    for (int i = 0; i < count; ++i) {
        const BlobEntry& e = ents[i];
        const char* met = out + h.payload_off + e.off + e.seg_off[SEG_METRICS];
        for (uint64_t k = 0; k < e.seg_n[SEG_METRICS]; ++k) {
            int32_t v;
            std::memcpy(&v, met + 4 * k, 4);
            if (v == INT32_MIN) return fail(OPV_ESTATE, "opv_export_streams: a released frame has not been decoded yet (call opv_process first)");
        }
    }
    return (long)h.total_bytes;
}

extern "C" int opv_blob_streams(const void* blob, size_t bytes) {
    BlobHeader h;
    if (const char* why = parse_blob(blob, bytes, &h, nullptr)) return fail(OPV_EINVAL, why);
    return (int)h.count;
}

extern "C" int opv_import_streams(opv_ctx* c, int count, const int* dst, const void* blob, size_t bytes) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (count < 0 || (count > 0 && !dst)) return fail(OPV_EINVAL, "opv_import_streams: bad arguments");
    BlobHeader h;
    std::vector<BlobEntry> ents;
    if (const char* why = parse_blob(blob, bytes, &h, &ents)) return fail(OPV_EINVAL, why);
    // ---- everything that can refuse the call is decided here, on the host, before the context is touched
    if ((uint32_t)count != h.count) return fail(OPV_EINVAL, "opv_import_streams: count differs from the streams in the blob (opv_blob_streams)");
    {
        std::vector<char> seen((size_t)c->n_streams, 0);
        for (int i = 0; i < count; ++i) {
            if (dst[i] < 0 || dst[i] >= c->n_streams) return fail(OPV_EINVAL, "opv_import_streams: destination stream index out of range");
            if (seen[dst[i]]) return fail(OPV_EINVAL, "opv_import_streams: a destination stream is named twice");
            seen[dst[i]] = 1;
        }
    }
    const opv_cfg& g = c->cfg;
    if (h.streaming != g.streaming || h.coherent != g.coherent || h.have_init_offset != g.have_init_offset ||
        (g.have_init_offset && h.init_offset_hz != g.init_offset_hz) || (g.coherent && h.pll_bw_hz != g.pll_bw_hz))
        return fail(OPV_EINVAL, "opv_import_streams: the blob was exported under another configuration (streaming / coherent / init_offset_hz / pll_bw_hz)");
    for (const BlobEntry& e : ents) {
        if (e.seg_n[SEG_IQ] > g.max_samples) return fail(OPV_ECAPACITY, "opv_import_streams: a stream's unconsumed IQ exceeds the destination's max_samples");
        if (e.seg_n[SEG_SOFT] > c->cap_soft) return fail(OPV_ECAPACITY, "opv_import_streams: a stream's soft-symbol tail exceeds the destination's ring");
        if (e.seg_n[SEG_FREC] > c->cap_frames) return fail(OPV_ECAPACITY, "opv_import_streams: more unpopped frames than the destination's frame_capacity");
    }
    if (count == 0) return OPV_OK;
    if (int r = settle_pushes(c)) return r;
    HIPCHK(hipStreamSynchronize(c->copy_stream));
    for (int i = 0; i < count; ++i) {                      // (a buffer more on a refused call is not a change of the context)
        if (ents[i].seg_n[SEG_IQ])
            if (int r = ensure_iq_buffer(c, c->hs[dst[i]], 0, "opv_import_streams: IQ buffer")) return r;
    }
    // ---- tables: one OpvUnpackItem per stream, then the moves out of the staging buffer into the destination's rings
    std::vector<OpvMove> mv;
    std::vector<OpvUnpackItem> items((size_t)count);
    if (int r = mig_buffers(c, (size_t)h.payload_bytes, 0)) return r;
    for (int i = 0; i < count; ++i) {
        const BlobEntry& e = ents[i];
        const HostStream& hs = c->hs[dst[i]];
        const OpvStream& ini = c->initial[dst[i]];
        OpvUnpackItem& it = items[i];
        std::memset(&it, 0, sizeof it);
        OpvStream& st = it.st;
        st = e.st;
        st.iq = hs.d_iq_owned;
        st.soft = ini.soft; st.cap_soft = ini.cap_soft;
        st.frec = ini.frec; st.events = ini.events; st.chunk_log = ini.chunk_log;
        st.frames = ini.frames; st.metrics = ini.metrics; st.fscale = ini.fscale;
        st.cap_frames = ini.cap_frames; st.cap_events = ini.cap_events; st.cap_chunks = ini.cap_chunks;
        st.fe_calls_free = st.fe_calls_guarded = 0;        // (a count of this context's launches, not part of a stream's carry)
        it.stream = (uint32_t)dst[i];
        it.live_first = e.popped % ini.cap_frames;
        it.live_n = (uint32_t)e.seg_n[SEG_FREC];
        BlobSegment seg[SEG_N];
        blob_segments(e, st, hs.d_iq_owned, seg);
        for (int k = 0; k < SEG_N; ++k) segment_moves(&mv, e, k, seg[k], c->mig.p + e.off, true);
    }
    const size_t items_bytes = (items.size() * sizeof(OpvUnpackItem) + 15u) & ~(size_t)15u;
    if (int r = mig_buffers(c, (size_t)h.payload_bytes, items_bytes + mv.size() * sizeof(OpvMove))) return r;
    std::memcpy(c->mig_tab.p, items.data(), items.size() * sizeof(OpvUnpackItem));
    if (!mv.empty()) std::memcpy((char*)c->mig_tab.p + items_bytes, mv.data(), mv.size() * sizeof(OpvMove));
    void* d_tab = nullptr;
    HIPCHK(hipHostGetDevicePointer(&d_tab, c->mig_tab.p, 0));
    // ---- ONE copy and ONE launch on the context's stream: behind the rounds in flight, in front of the next one
    if (int r = mig_time(c, false)) return r;
    if (h.payload_bytes) HIPCHK(hipMemcpyAsync(c->mig.p, (const char*)blob + h.payload_off, (size_t)h.payload_bytes, hipMemcpyHostToDevice, c->stream));
    k_stream_unpack<<<mig_grid(items.size() + mv.size()), 256, 0, c->stream>>>(c->d_streams, c->d_counts, (const OpvUnpackItem*)d_tab, (uint32_t)items.size(),
                                                                             (const OpvMove*)((char*)d_tab + items_bytes), (uint32_t)mv.size());
    HIPCHK(hipGetLastError());
    if (int r = mig_time(c, true)) return r;
    for (int i = 0; i < count; ++i) {                      // the host's half of the slot: opv_reset_stream, then the load
        const BlobEntry& e = ents[i];
        HostStream n = reset_host_stream(c->hs[dst[i]]);
        n.n_avail = e.seg_n[SEG_IQ];
        n.eof = e.eof;
        n.dirty = true;                                    // (iq / n_avail / eof and the cursors reach the kernels with the next round's inputs too)
        n.search_seen = e.search_seen != 0;
        n.last_round_avail = e.last_round_avail;
        n.popped = e.popped;
        n.events_popped = e.events_popped;
        n.events_dropped = e.events_dropped;
        n.decoded = e.decoded;
        n.perfect = e.perfect;
        n.soft_floor = e.soft_first;
        n.iq_seen = true;                                  // (its soft symbols came out of a front-end)
        n.chunk_floor = e.chunks_first + (uint32_t)(e.seg_n[SEG_CHUNKS] - (e.seg_n[SEG_CHUNKS] < c->cap_chunks ? e.seg_n[SEG_CHUNKS] : c->cap_chunks));
        c->hs[dst[i]] = n;
        c->div.restarted(dst[i], e.st.n_frames);           // (a diversity group combines only what the stream releases from here on)
    }
    c->mirror_valid = false;
    c->maybe_stalled = true;
    for (int i = 0; i < count; ++i)                        // link records do not travel: the slot's read valid = 0, as after a reset
        if (int r = link_clear(c, dst[i], dst[i] + 1)) return r;
    HIPCHK(hipStreamSynchronize(c->stream));               // the blob is the caller's again
    return OPV_OK;
}
