// opv_stream_rules.h — the rules that keep a stream's buffers consistent, once each, in plain C++ (no HIP header: with
// opv_stream_rules.cpp it compiles with the host compiler like opv_offset_host.cpp, and runs under sanitizers without a GPU).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/opv_demod.h"
#include "opv_device.h"

// ---- compaction: IQ in front of the current chunk origin, minus the 16-sample reach of the early gate / tile alignment, is
// dropped; `keep` (samples dropped) is a multiple of 4 so that the retained tail stays 16-byte aligned
inline uint64_t iq_keep(uint64_t origin) { return origin >= 16 ? ((origin - 16) & ~3ull) : 0; }

// the re-base that goes with it: the host's view of the stream and an OpvStream (origin + iq_base stays what it was)
inline void iq_rebase(uint64_t keep, uint64_t* n_avail, uint64_t* last_round_avail, OpvStream* st) {
    *n_avail -= keep;
    *last_round_avail = *last_round_avail > keep ? *last_round_avail - keep : 0;
    st->origin -= keep;
    st->n_avail -= keep;
    st->iq_base += keep;
}

// ---- rings: elements [first, first + n) of a ring of `cap` slots (n <= cap) are run0 slots from p0 on, then run1 from slot 0
struct RingRuns { uint64_t p0, run0, run1; };
inline RingRuns ring_runs(uint64_t first, uint64_t n, uint64_t cap) {
    const uint64_t p0 = first % cap, run0 = n < cap - p0 ? n : cap - p0;
    return {p0, run0, n - run0};
}

// first soft symbol a push of staged symbols must leave alone (k_frontend.hip: soft_keep - the front-end's own rule for room)
inline uint64_t soft_keep(const OpvStream& st) {
    uint64_t keep = st.trk_next >= 24 ? st.trk_next - 24 : 0;
    if (st.trk_state != OPV_HUNTING && st.trk_anchor < keep) keep = st.trk_anchor;
    return keep;
}

// ---- the table-driven kernels (k_push_gather, k_compact): an item is split into `slices` work items so that few items still keep
// enough moves in flight - about 1024, never thinner than one move per lane of a block. `most`: the largest item, `unit`: one move (same units); items >= 1
struct LaunchShape { uint32_t slices, grid; };
inline LaunchShape table_launch(uint32_t items, uint32_t most, uint32_t unit, uint32_t grid_cap) {
    uint32_t slices = items >= 1024 ? 1 : (1024 + items - 1) / items;
    const uint32_t by_size = most / (256u * unit);
    if (slices > by_size) slices = by_size ? by_size : 1;
    const uint32_t grid = items * slices;
    return {slices, grid > grid_cap ? grid_cap : grid};
}

// ---- stream migration: the blob is [BlobHeader][BlobEntry x count][payload]. An entry is the stream's OpvStream (pointers
// cleared, IQ indices re-based to the exported tail as compaction re-bases them), the host's fields, and where its eight payload
// segments lie; the payload is what k_stream_pack put into the staging buffer, byte for byte. The format is private to one build
// of the library: every header field must match, and parse_blob checks every offset, length and index before anything is launched.
constexpr uint64_t kBlobMagic = 0x31424f4c4256504full;   // "OPVBLOB1"
constexpr uint32_t kBlobVersion = 1;
enum { SEG_IQ, SEG_SOFT, SEG_FREC, SEG_FRAMES, SEG_METRICS, SEG_FSCALE, SEG_EVENTS, SEG_CHUNKS, SEG_N };
constexpr uint64_t kSegElem[SEG_N] = {4, sizeof(double), sizeof(OpvFrameRec), OPV_FB, sizeof(int32_t), sizeof(double), sizeof(OpvEventRec), 5 * sizeof(double)};

struct BlobHeader {
    uint64_t magic;
    uint32_t version, sizeof_stream, sizeof_header, sizeof_entry;
    int32_t streaming, coherent, have_init_offset;   // the cfg fields that fix behaviour (afc_alpha travels in the OpvStream)
    uint32_t count;
    double init_offset_hz, pll_bw_hz;
    uint64_t total_bytes, payload_off, payload_bytes;
};
struct BlobEntry {
    uint64_t off, len;                  // the stream's payload: offset from payload_off (multiple of 16) and bytes
    uint64_t seg_off[SEG_N];            // from `off`, multiples of 16
    uint64_t seg_n[SEG_N];              // ELEMENTS (samples, symbols, records, frames, ..., chunk-log entries)
    uint64_t soft_first;                // absolute index of the first carried soft symbol (even)
    uint32_t events_first, chunks_first;   // absolute indices; frames start at `popped`
    uint32_t popped, events_popped, events_dropped;
    int32_t decoded, perfect, eof, search_seen, pad;
    uint64_t last_round_avail;
    OpvStream st;
};

inline uint64_t up16(uint64_t v) { return (v + 15u) & ~15ull; }
inline uint64_t blob_payload_off(int count) { return (sizeof(BlobHeader) + (uint64_t)count * sizeof(BlobEntry) + 255u) & ~255ull; }

// first soft symbol the tracker or the decoder can still read (k_frontend.hip: soft_keep, k_sync_track.hip), even
uint64_t soft_tail_first(const OpvStream& st);

// nullptr if the blob holds together (*h filled, and *ents unless ents is null), else why not; every refusal is OPV_EINVAL
const char* parse_blob(const void* blob, size_t bytes, BlobHeader* h, std::vector<BlobEntry>* ents);

// One segment of a migrated stream against the rings of a context: `n` elements from absolute index `first` of a ring of `cap`
// slots. A lossy ring (events, chunk log) takes only the newest entries it holds; the others refuse an import that does not fit.
// `rings`: an OpvStream of the context the segments live in (its log pointers and capacities); `iq`: the linear IQ tail
struct BlobSegment { char* ring; uint64_t cap, first, n; bool lossy; };
void blob_segments(const BlobEntry& e, const OpvStream& rings, const void* iq, BlobSegment seg[SEG_N]);

// the moves of segment k of `e` between its ring and the entry's payload at `base`: un-wrapped (ring_runs) and cut into pieces of
// at most OPV_MOVE_PIECE bytes (to_ring: payload -> ring, else ring -> payload)
void segment_moves(std::vector<OpvMove>* mv, const BlobEntry& e, int k, const BlobSegment& g, char* base, bool to_ring);
