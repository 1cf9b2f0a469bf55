// stream_rules_probe.cpp — test support for csrc/opv_stream_rules.{h,cpp} (plain C++, no GPU): a C face for ctypes
// (tests/test_stream_rules_host.py) and, with -DPROBE_MAIN, a stand-alone program that runs the same blobs and grids through
// parse_blob, ring_runs, the segment table and the launch shape and prints one line (tests/test_sanitizers.py builds it with and
// without sanitizers and compares the lines). probe_blob_shift moves a blob's absolute indices forward: how
// tests/test_gpu_far_positions.py takes a live stream across symbol and sample 2^32.
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "opv_stream_rules.h"

extern "C" {
uint64_t probe_iq_keep(uint64_t origin) { return iq_keep(origin); }
// v = {n_avail, last_round_avail, origin, st.n_avail, iq_base}, re-based in place
void probe_iq_rebase(uint64_t keep, uint64_t v[5]) {
    OpvStream st;
    std::memset(&st, 0, sizeof st);
    st.origin = v[2]; st.n_avail = v[3]; st.iq_base = v[4];
    iq_rebase(keep, &v[0], &v[1], &st);
    v[2] = st.origin; v[3] = st.n_avail; v[4] = st.iq_base;
}
void probe_ring_runs(uint64_t first, uint64_t n, uint64_t cap, uint64_t out[3]) {
    const RingRuns r = ring_runs(first, n, cap);
    out[0] = r.p0; out[1] = r.run0; out[2] = r.run1;
}
void probe_table_launch(uint32_t items, uint32_t most, uint32_t unit, uint32_t grid_cap, uint32_t out[2]) {
    const LaunchShape l = table_launch(items, most, unit, grid_cap);
    out[0] = l.slices; out[1] = l.grid;
}
// the refusal's text ("" if the blob holds together); *count = streams in the blob
const char* probe_parse_blob(const void* blob, size_t bytes, int with_entries, uint32_t* count) {
    BlobHeader h;
    std::vector<BlobEntry> ents;
    const char* why = parse_blob(blob, bytes, &h, with_entries ? &ents : nullptr);
    if (!why && count) *count = h.count;
    return why ? why : "";
}
// where the fields a test pokes live
long probe_offset(const char* name) {
    const std::string n = name;
#define H(f) if (n == "h." #f) return (long)offsetof(BlobHeader, f);
#define E(f) if (n == "e." #f) return (long)offsetof(BlobEntry, f);
#define S(f) if (n == "st." #f) return (long)(offsetof(BlobEntry, st) + offsetof(OpvStream, f));
    H(magic) H(version) H(sizeof_stream) H(sizeof_header) H(sizeof_entry) H(count) H(total_bytes) H(payload_off) H(payload_bytes)
    E(off) E(len) E(seg_off) E(seg_n) E(soft_first) E(events_first) E(chunks_first) E(popped) E(events_popped) E(last_round_avail)
    S(n_avail) S(origin) S(overflow) S(n_soft) S(cap_soft) S(trk_next) S(trk_anchor) S(trk_state) S(n_frames) S(n_events) S(n_chunks) S(iq_base)
    S(total_samples) S(fo_sum)
#undef H
#undef E
#undef S
    if (n == "frec.payload_sym") return (long)offsetof(OpvFrameRec, payload_sym);
    if (n == "frec.release_sym") return (long)offsetof(OpvFrameRec, release_sym);
    if (n == "event.sym_idx") return (long)offsetof(OpvEventRec, sym_idx);
    if (n.size() == 9 && n.compare(0, 8, "segelem.") == 0 && n[8] >= '0' && n[8] < '0' + SEG_N) return (long)kSegElem[n[8] - '0'];   // bytes per element of segment k
    if (n == "sizeof.frec") return (long)sizeof(OpvFrameRec);
    if (n == "sizeof.event") return (long)sizeof(OpvEventRec);
    if (n == "sizeof.header") return (long)sizeof(BlobHeader);
    if (n == "sizeof.entry") return (long)sizeof(BlobEntry);
    if (n == "sizeof.stream") return (long)sizeof(OpvStream);
    return -1;
}
// A stream moved to a far position: every absolute SYMBOL index of every entry of the blob (n_soft, the tracker's anchor and next,
// soft_first, payload_sym / release_sym of the carried frame records, sym_idx of the carried events) forward by d_sym, every absolute
// SAMPLE index (total_samples, iq_base) by d_samp, in place. origin, n_avail and last_round_avail are relative to the IQ tail, fo_sum
// is the LO's phase and the 32-bit frame / event / chunk counters wrap years away: all left alone. Returns 0 if the blob passed
// parse_blob before and after; non-zero, with the bytes as they were, if it did not, if a shift is no multiple of 4 (silence_pd
// reads ksym & 3, soft_first stays even, the IQ tail stays 16-byte aligned) or if an entry has n_soft < 24 or trk_next < 23 (its
// hunt has not reached symbol 23 yet and would start at another symbol after the shift: not the same run).
int probe_blob_shift(void* blob, size_t bytes, uint64_t d_sym, uint64_t d_samp) {
    BlobHeader h;
    std::vector<BlobEntry> ents;
    if (parse_blob(blob, bytes, &h, &ents)) return 1;
    if ((d_sym & 3u) || (d_samp & 3u)) return 2;
    for (const BlobEntry& e : ents)
        if (e.st.n_soft < 24 || e.st.trk_next < 23) return 3;
    std::vector<char> b((const char*)blob, (const char*)blob + h.total_bytes);
    auto add = [&](uint64_t at, uint64_t d) {               // (the caller's bytes may sit at any alignment)
        uint64_t v;
        std::memcpy(&v, b.data() + at, 8);
        v += d;
        std::memcpy(b.data() + at, &v, 8);
    };
    for (size_t i = 0; i < ents.size(); ++i) {
        BlobEntry& e = ents[i];
        e.st.n_soft += d_sym; e.st.trk_anchor += d_sym; e.st.trk_next += d_sym; e.soft_first += d_sym;
        e.st.total_samples += d_samp; e.st.iq_base += d_samp;
        std::memcpy(b.data() + sizeof(BlobHeader) + i * sizeof(BlobEntry), &e, sizeof e);
        const uint64_t at = h.payload_off + e.off;
        for (uint64_t k = 0; k < e.seg_n[SEG_FREC]; ++k) {
            add(at + e.seg_off[SEG_FREC] + k * sizeof(OpvFrameRec) + offsetof(OpvFrameRec, payload_sym), d_sym);
            add(at + e.seg_off[SEG_FREC] + k * sizeof(OpvFrameRec) + offsetof(OpvFrameRec, release_sym), d_sym);
        }
        for (uint64_t k = 0; k < e.seg_n[SEG_EVENTS]; ++k) add(at + e.seg_off[SEG_EVENTS] + k * sizeof(OpvEventRec) + offsetof(OpvEventRec, sym_idx), d_sym);
    }
    if (parse_blob(b.data(), b.size(), &h, &ents)) return 4;
    std::memcpy(blob, b.data(), b.size());
    return 0;
}
uint64_t probe_blob_payload_off(int count) { return blob_payload_off(count); }
uint64_t probe_blob_magic(void) { return kBlobMagic; }
// the moves of all eight segments of an entry against rings at made-up addresses: returns their number, and in sum[2] the bytes
// moved and a checksum of (ring offset, payload offset, bytes) of every move; every move is checked to lie inside its ring
long probe_segment_moves(const BlobEntry* e, const uint64_t cap[4], int to_ring, uint64_t sum[2]) {
    OpvStream r;
    std::memset(&r, 0, sizeof r);
    char* const ring0 = (char*)0x100000000ull;             // (addresses only: nothing is dereferenced)
    const uint64_t stride = 1ull << 32;
    r.soft = (double*)(ring0 + 1 * stride); r.frec = (OpvFrameRec*)(ring0 + 2 * stride); r.frames = (uint8_t*)(ring0 + 3 * stride);
    r.metrics = (int32_t*)(ring0 + 4 * stride); r.fscale = (double*)(ring0 + 5 * stride); r.events = (OpvEventRec*)(ring0 + 6 * stride);
    r.chunk_log = (double*)(ring0 + 7 * stride);
    r.cap_soft = cap[0]; r.cap_frames = (uint32_t)cap[1]; r.cap_events = (uint32_t)cap[2]; r.cap_chunks = (uint32_t)cap[3];
    BlobSegment seg[SEG_N];
    blob_segments(*e, r, ring0, seg);
    std::vector<OpvMove> mv;
    char* const base = (char*)(20 * stride);
    sum[0] = sum[1] = 0;
    for (int k = 0; k < SEG_N; ++k) {
        const size_t before = mv.size();
        segment_moves(&mv, *e, k, seg[k], base, to_ring != 0);
        for (size_t i = before; i < mv.size(); ++i) {
            const char* in_ring = (const char*)(to_ring ? mv[i].dst : mv[i].src);
            const char* in_blob = (const char*)(to_ring ? mv[i].src : mv[i].dst);
            const uint64_t ro = (uint64_t)(in_ring - seg[k].ring), bo = (uint64_t)(in_blob - base);
            if (mv[i].bytes == 0 || mv[i].bytes > OPV_MOVE_PIECE || ro + mv[i].bytes > seg[k].cap * kSegElem[k]) return -1;
            if (bo < e->seg_off[k] || bo + mv[i].bytes > e->seg_off[k] + e->seg_n[k] * kSegElem[k]) return -2;
            sum[0] += mv[i].bytes;
            sum[1] = sum[1] * 1000003u + ro * 31u + bo * 7u + mv[i].bytes;
        }
    }
    return (long)mv.size();
}
}

#ifdef PROBE_MAIN
// a valid blob of two streams with empty segments (stream 1: non-zero cursors), then a set of mutations of it
static std::vector<char> base_blob() {
    BlobHeader h;
    std::memset(&h, 0, sizeof h);
    h.magic = kBlobMagic; h.version = kBlobVersion; h.sizeof_stream = sizeof(OpvStream); h.sizeof_header = sizeof(BlobHeader); h.sizeof_entry = sizeof(BlobEntry);
    h.streaming = 1; h.count = 2; h.payload_off = blob_payload_off(2); h.payload_bytes = 1024; h.total_bytes = h.payload_off + h.payload_bytes;
    std::vector<char> b((size_t)h.total_bytes, 0);
    std::memcpy(b.data(), &h, sizeof h);
    for (int i = 0; i < 2; ++i) {
        BlobEntry e;
        std::memset(&e, 0, sizeof e);
        e.off = 512u * i; e.len = 512;
        for (int k = 0; k < SEG_N; ++k) e.seg_off[k] = 16u * k;
        if (i) { e.popped = 3; e.st.n_frames = 3; e.events_first = e.events_popped = 5; e.st.n_events = 5; e.chunks_first = 2; e.st.n_chunks = 2; e.st.iq_base = 1000; }
        std::memcpy(b.data() + sizeof h + sizeof e * i, &e, sizeof e);
    }
    return b;
}

// a valid blob of two streams past symbol 24, each with a soft tail of 40 symbols, two unpopped frame records and three events
static std::vector<char> live_blob() {
    const uint64_t n[SEG_N] = {0, 40, 2, 2, 2, 2, 3, 0};
    uint64_t off[SEG_N], len = 0;
    for (int k = 0; k < SEG_N; ++k) { off[k] = len; len += up16(n[k] * kSegElem[k]); }
    BlobHeader h;
    std::memset(&h, 0, sizeof h);
    h.magic = kBlobMagic; h.version = kBlobVersion; h.sizeof_stream = sizeof(OpvStream); h.sizeof_header = sizeof(BlobHeader); h.sizeof_entry = sizeof(BlobEntry);
    h.streaming = 1; h.count = 2; h.payload_off = blob_payload_off(2); h.payload_bytes = 2 * len; h.total_bytes = h.payload_off + h.payload_bytes;
    std::vector<char> b((size_t)h.total_bytes, 0);
    std::memcpy(b.data(), &h, sizeof h);
    for (int i = 0; i < 2; ++i) {
        BlobEntry e;
        std::memset(&e, 0, sizeof e);
        e.off = len * i; e.len = len;
        for (int k = 0; k < SEG_N; ++k) { e.seg_off[k] = off[k]; e.seg_n[k] = n[k]; }
        e.st.n_soft = 5000 + 2 * i; e.st.trk_next = e.st.n_soft; e.st.trk_anchor = 4990; e.st.trk_state = i ? OPV_LOCKED : OPV_HUNTING; e.st.cap_soft = 4096;
        e.soft_first = e.st.n_soft - 40;
        e.popped = 3u * i; e.st.n_frames = e.popped + 2; e.events_first = e.events_popped = 5u * i; e.st.n_events = e.events_first + 3;
        e.st.total_samples = 200000; e.st.iq_base = 1000u * i;
        std::memcpy(b.data() + sizeof h + sizeof e * i, &e, sizeof e);
        for (uint64_t k = 0; k < 2; ++k) {
            const OpvFrameRec r = {2800 + 2168 * k, 4944 + 2168 * k, 0.9, 1, 0};
            std::memcpy(b.data() + h.payload_off + e.off + off[SEG_FREC] + k * sizeof r, &r, sizeof r);
        }
        for (uint64_t k = 0; k < 3; ++k) {
            const OpvEventRec r = {(int32_t)(1 + k), 0, 23 + 2168 * k, 0.8, 1.0};
            std::memcpy(b.data() + h.payload_off + e.off + off[SEG_EVENTS] + k * sizeof r, &r, sizeof r);
        }
    }
    return b;
}

int main() {
    unsigned long long acc = 0;
    auto mix = [&](unsigned long long v) { acc = acc * 1000003ull + v; };
    // the far-position shift (probe_blob_shift): taken with its multiples of 4, each in an allocation of exactly the blob's length;
    // refused - the bytes untouched - for the other shifts, for a truncated blob and for the base blob's streams below symbol 24
    {
        const std::vector<char> live = live_blob();
        for (uint64_t d : {(uint64_t)0, (uint64_t)4, (uint64_t)1 << 31, ((uint64_t)1 << 32) - 4, ((uint64_t)1 << 40) + 8}) {
            std::vector<char> b = live;
            if (probe_blob_shift(b.data(), b.size(), d, d + 4) != 0) return 5;
            BlobHeader h;
            std::vector<BlobEntry> ents;
            if (parse_blob(b.data(), b.size(), &h, &ents) || ents[1].st.n_soft != 5002 + d || ents[1].st.iq_base != 1000 + d + 4) return 6;
            uint64_t v;
            std::memcpy(&v, b.data() + h.payload_off + ents[1].off + ents[1].seg_off[SEG_EVENTS] + 2 * sizeof(OpvEventRec) + offsetof(OpvEventRec, sym_idx), 8);
            if (v != 23 + 2 * 2168 + d) return 7;
            mix(ents[0].soft_first); mix(ents[1].st.trk_anchor); mix(ents[0].st.total_samples);
        }
        for (uint64_t d : {(uint64_t)1, (uint64_t)2, (uint64_t)6}) {
            std::vector<char> b = live;
            if (probe_blob_shift(b.data(), b.size(), d, 0) == 0 || probe_blob_shift(b.data(), b.size(), 0, d) == 0 || b != live) return 8;
        }
        std::vector<char> cut(live.begin(), live.end() - 8), low = base_blob(), low0 = low;
        if (probe_blob_shift(cut.data(), cut.size(), 4, 4) == 0 || probe_blob_shift(low.data(), low.size(), 4, 4) == 0 || low != low0) return 9;
    }
    // blobs: the base, every prefix length that matters, every byte of the header and of the first entry's index fields poked
    const std::vector<char> good = base_blob();
    uint32_t count = 0;
    int accepted = 0, refused = 0;
    auto run = [&](const std::vector<char>& b, size_t bytes) {
        std::vector<char> exact(b.begin(), b.begin() + bytes);             // (an allocation of exactly `bytes`: a read past it is a report)
        const char* why = probe_parse_blob(exact.data(), bytes, 1, &count);
        if (*why) { ++refused; mix(std::strlen(why)); } else { ++accepted; mix(count); }
        (void)probe_parse_blob(exact.data(), bytes, 0, &count);
    };
    run(good, good.size());
    for (size_t n = 0; n <= good.size(); n += (n < 1200 ? 1 : 37)) run(good, n);
    const size_t poke_end = sizeof(BlobHeader) + offsetof(BlobEntry, st);
    for (size_t at = 0; at < poke_end; ++at)
        for (unsigned char v : {(unsigned char)0x5A, (unsigned char)0xFF, (unsigned char)0x01}) {
            std::vector<char> b = good;
            b[at] = (char)(b[at] ^ v);
            run(b, b.size());
        }
    for (size_t at = 0; at < sizeof(OpvStream); at += 4) {                 // ... and the OpvStream's words
        std::vector<char> b = good;
        b[sizeof(BlobHeader) + offsetof(BlobEntry, st) + at] ^= 0x5A;
        run(b, b.size());
    }
    // rings, launch shapes, what compaction keeps
    for (uint64_t cap : {(uint64_t)1, (uint64_t)2, (uint64_t)5, (uint64_t)4096})
        for (uint64_t first : {(uint64_t)0, (uint64_t)1, cap - 1, cap, cap + 1, 3 * cap - 1, ((uint64_t)1 << 40) + 3})
            for (uint64_t n = 0; n <= cap; n += (cap > 8 ? 511 : 1)) {
                uint64_t r[3];
                probe_ring_runs(first, n, cap, r);
                if (r[0] >= cap || r[1] + r[2] != n || r[0] + r[1] > cap || r[2] > r[0]) return 2;
                mix(r[0]); mix(r[1]);
            }
    for (uint32_t m : {1u, 2u, 14u, 1023u, 1024u, 5000u})
        for (uint32_t most : {0u, 1u, 4u, 16u, 4092u, 16368u, 347000u})
            for (uint32_t unit : {4u, 16u})
                for (uint32_t cap : {32u, 2048u}) {
                    uint32_t l[2];
                    probe_table_launch(m, most, unit, cap, l);
                    if (l[0] < 1 || l[1] < 1 || l[1] > cap) return 3;
                    mix(l[0]); mix(l[1]);
                }
    for (uint64_t o = 0; o <= 40; ++o) mix(probe_iq_keep(o));
    mix(probe_iq_keep((1ull << 31) - 1));
    // the segment table: an entry with every segment filled, against rings smaller and larger than the lossy logs
    BlobEntry e;
    std::memset(&e, 0, sizeof e);
    const uint64_t n[SEG_N] = {100000, 3000, 7, 7, 7, 7, 300, 9};
    uint64_t o = 0;
    for (int k = 0; k < SEG_N; ++k) { e.seg_n[k] = n[k]; e.seg_off[k] = o; o += up16(n[k] * kSegElem[k]); }
    e.len = o; e.soft_first = 5000; e.popped = 6; e.events_first = 250; e.chunks_first = 14;
    for (int to_ring = 0; to_ring < 2; ++to_ring)
        for (uint64_t cev : {(uint64_t)64, (uint64_t)300, (uint64_t)1000}) {
            const uint64_t cap[4] = {4096, 8, to_ring ? cev : (uint64_t)1000, (uint64_t)(to_ring ? 4 : 16)};
            uint64_t sum[2];
            const long moves = probe_segment_moves(&e, cap, to_ring, sum);
            if (moves < 0) return 4;
            mix((unsigned long long)moves); mix(sum[0]); mix(sum[1]);
        }
    std::printf("%d %d %llx\n", accepted, refused, acc);
    return 0;
}
#endif
