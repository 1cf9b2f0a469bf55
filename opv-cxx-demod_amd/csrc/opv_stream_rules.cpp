// opv_stream_rules.cpp — the parts of opv_stream_rules.h that read a caller's bytes or fill tables: the migration blob's checks
// and the moves of a migrated stream's segments. Plain C++, compiled with the host compiler (Makefile: CXXFLAGS).
#include "opv_stream_rules.h"

#include <cstring>

uint64_t soft_tail_first(const OpvStream& st) {
    uint64_t lo = st.trk_next;
    if (st.trk_state != OPV_HUNTING && st.trk_anchor + 1 < lo) lo = st.trk_anchor + 1;
    lo = lo >= 24 ? lo - 24 : 0;
    if (lo > st.n_soft) lo = st.n_soft;
    lo &= ~1ull;
    if (st.n_soft > st.cap_soft && lo < st.n_soft - st.cap_soft) lo = (st.n_soft - st.cap_soft + 1) & ~1ull;   // (what the ring still holds)
    return lo;
}

const char* parse_blob(const void* blob, size_t bytes, BlobHeader* h, std::vector<BlobEntry>* ents) {
    if (!blob || bytes < sizeof(BlobHeader)) return "stream blob: missing or shorter than its header";
    std::memcpy(h, blob, sizeof *h);    // (the caller's bytes may sit at any alignment)
    if (h->magic != kBlobMagic) return "stream blob: wrong magic";
    if (h->version != kBlobVersion || h->sizeof_stream != sizeof(OpvStream) || h->sizeof_header != sizeof(BlobHeader) || h->sizeof_entry != sizeof(BlobEntry))
        return "stream blob: written by another build of the library (format version / struct sizes differ)";
    if (h->total_bytes > bytes || h->total_bytes < sizeof(BlobHeader)) return "stream blob: truncated";
    if (h->count > 0x7FFFFFFFu || (uint64_t)h->count > (h->total_bytes - sizeof(BlobHeader)) / sizeof(BlobEntry)) return "stream blob: stream count does not fit the blob";
    const uint64_t dir_end = sizeof(BlobHeader) + (uint64_t)h->count * sizeof(BlobEntry);
    if ((h->payload_off & 15u) || h->payload_off < dir_end || h->payload_off > h->total_bytes || h->payload_bytes != h->total_bytes - h->payload_off)
        return "stream blob: payload offset / length out of range";
    if (!ents) return nullptr;
    ents->resize(h->count);
    if (h->count) std::memcpy(ents->data(), (const char*)blob + sizeof(BlobHeader), (size_t)h->count * sizeof(BlobEntry));
    for (const BlobEntry& e : *ents) {
        if ((e.off & 15u) || e.off > h->payload_bytes || e.len > h->payload_bytes - e.off) return "stream blob: a stream's payload lies outside the blob";
        for (int k = 0; k < SEG_N; ++k) {
            if (e.seg_n[k] >= (1ull << 31)) return "stream blob: segment length out of range";
            const uint64_t b = e.seg_n[k] * kSegElem[k];
            if ((e.seg_off[k] & 15u) || e.seg_off[k] > e.len || b > e.len - e.seg_off[k]) return "stream blob: a segment lies outside its stream's payload";
        }
        const OpvStream& st = e.st;
        const uint32_t nf = (uint32_t)e.seg_n[SEG_FREC];
        bool ok = e.seg_n[SEG_IQ] == st.n_avail && st.origin <= st.n_avail && st.overflow == 0;
        ok = ok && e.soft_first + e.seg_n[SEG_SOFT] == st.n_soft && (e.soft_first & 1u) == 0 && e.soft_first <= soft_tail_first(st) && st.trk_next <= st.n_soft;
        ok = ok && e.seg_n[SEG_FRAMES] == nf && e.seg_n[SEG_METRICS] == nf && e.seg_n[SEG_FSCALE] == nf && e.popped + nf == st.n_frames;
        ok = ok && e.events_first + (uint32_t)e.seg_n[SEG_EVENTS] == st.n_events && e.events_first == e.events_popped;
        ok = ok && e.chunks_first + (uint32_t)e.seg_n[SEG_CHUNKS] == st.n_chunks && e.last_round_avail <= st.n_avail;
        if (!ok) return "stream blob: a stream's indices contradict its segments";
    }
    return nullptr;
}

void blob_segments(const BlobEntry& e, const OpvStream& r, const void* iq, BlobSegment seg[SEG_N]) {
    seg[SEG_IQ] = {(char*)iq, e.seg_n[SEG_IQ], 0, e.seg_n[SEG_IQ], false};          // (linear: a ring of exactly its length)
    seg[SEG_SOFT] = {(char*)r.soft, r.cap_soft, e.soft_first, e.seg_n[SEG_SOFT], false};
    seg[SEG_FREC] = {(char*)r.frec, r.cap_frames, e.popped, e.seg_n[SEG_FREC], false};
    seg[SEG_FRAMES] = {(char*)r.frames, r.cap_frames, e.popped, e.seg_n[SEG_FRAMES], false};
    seg[SEG_METRICS] = {(char*)r.metrics, r.cap_frames, e.popped, e.seg_n[SEG_METRICS], false};
    seg[SEG_FSCALE] = {(char*)r.fscale, r.cap_frames, e.popped, e.seg_n[SEG_FSCALE], false};
    seg[SEG_EVENTS] = {(char*)r.events, r.cap_events, e.events_first, e.seg_n[SEG_EVENTS], true};
    seg[SEG_CHUNKS] = {(char*)r.chunk_log, r.cap_chunks, e.chunks_first, e.seg_n[SEG_CHUNKS], true};
}

void segment_moves(std::vector<OpvMove>* mv, const BlobEntry& e, int k, const BlobSegment& g, char* base, bool to_ring) {
    const uint64_t elem = kSegElem[k], n = g.lossy && g.n > g.cap ? g.cap : g.n, skip = g.n - n;   // a lossy ring: the newest entries it holds
    if (n == 0) return;
    const RingRuns r = ring_runs(g.first + skip, n, g.cap);
    char* linear = base + e.seg_off[k] + skip * elem;
    const struct { uint64_t slot, bytes; } runs[2] = {{r.p0, r.run0 * elem}, {0, r.run1 * elem}};
    for (const auto& run : runs) {
        for (uint64_t o = 0; o < run.bytes; o += OPV_MOVE_PIECE) {
            const uint64_t b = run.bytes - o < OPV_MOVE_PIECE ? run.bytes - o : OPV_MOVE_PIECE;
            char* in_ring = g.ring + run.slot * elem + o;
            mv->push_back(to_ring ? OpvMove{linear + o, in_ring, (uint32_t)b, 0} : OpvMove{in_ring, linear + o, (uint32_t)b, 0});
        }
        linear += run.bytes;
    }
}
