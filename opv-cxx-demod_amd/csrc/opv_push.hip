// opv_push.hip — the serving path of the C-ABI shim: pushes (single, batched, asynchronous), the compaction that keeps a
// long-running stream inside its bounded device buffers, flush / attach, and the wideband front door's way in. What the pushes
// share is written once: opv_stream_rules.h, and push_admit / ensure_iq_buffer / push_finish below. Typed pushes (cs8, cu8, cf32)
// are the same pushes with a format: k_push_convert beside k_push_gather, push_convert_deferred beside push_deferred; the rule that
// widens a sample is opv_iq_format.h's. A typed pair is cut into a head (the samples in front of the SOURCE's first 16-byte boundary,
// one per lane), a body (16 bytes per lane and move, aligned to the source - the side that crosses the link - and stored to a
// destination that is only 4-byte aligned) and a tail (what is left behind the last whole 16 bytes): the comment on k_push_convert.
#include <utility>

#include "opv_ctx.h"
#include "opv_iq_format.h"
#include "opv_stream_rules.h"

namespace {

// ---- the serving path's two bulk moves (a live server pushes one 40 ms chunk per stream and round: N separate 347 KB blocks) ----
// k_push_gather: host -> device for MANY streams in one launch. The sources are the caller's buffers in pinned host memory, read
// through their device-visible addresses (16 B per lane over PCIe); the table itself lives in pinned memory too. One
// hipMemcpyAsync per stream moves 1536 such blocks at 21 GB/s (per-copy overhead), this kernel at 57 - the link's rate for one
// large copy (scripts/microbench/h2d_many.hip). A pair is split into `slices` work items so that few streams still keep
// enough loads in flight.
struct PushPair {
    const void* src;     // device-visible address of the caller's samples
    void* dst;           // where they go in the stream's device buffer
    uint32_t bytes;      // multiple of 4 (one sample)
    uint32_t wide;       // 1: src and dst are 16-byte aligned (int4 moves + a tail of ints), 0: 4-byte moves
};
__global__ __launch_bounds__(256) void k_push_gather(const PushPair* tab, uint32_t n_pairs, uint32_t slices) {
    for (uint32_t w = blockIdx.x; w < n_pairs * slices; w += gridDim.x) {
        const PushPair p = tab[w / slices];
        const uint32_t sl = w % slices;
        if (p.wide) {
            const uint32_t quads = p.bytes >> 4, per = (quads + slices - 1) / slices;
            const uint32_t lo = sl * per, hi = lo + per < quads ? lo + per : quads;
            const int4* s4 = (const int4*)p.src;
            int4* d4 = (int4*)p.dst;
            for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) d4[i] = s4[i];
            if (sl == 0) {                                  // at most three samples behind the last full quad
                const uint32_t rem = (p.bytes & 15u) >> 2;
                if (threadIdx.x < rem) ((int*)p.dst)[quads * 4 + threadIdx.x] = ((const int*)p.src)[quads * 4 + threadIdx.x];
            }
        } else {
            const uint32_t words = p.bytes >> 2, per = (words + slices - 1) / slices;
            const uint32_t lo = sl * per, hi = lo + per < words ? lo + per : words;
            for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) ((int*)p.dst)[i] = ((const int*)p.src)[i];
        }
    }
}
// k_push_convert<fmt>: k_push_gather for blocks that are NOT int16 (include/opv_demod.h, "typed IQ pushes"): the block crosses PCIe in
// the radio's own format - CS8 / CU8 at half the bytes of int16, CF32 at twice - and is widened to int16 here, behind the link, by
// the one rule of opv_iq_format.h. Same shape as k_push_gather: a pinned table of pairs, each cut into `slices` work items by
// table_launch, the same deliberately small grid (push_deferred). A source is the caller's pinned block read in place, or the raw
// copy of a pageable one in a device stage; a launch for ONE block (the wideband door, the scan, opv_convert_iq_device) hands its
// pair over by value instead (tab == nullptr), so that nothing pinned has to outlive the call.
//   How a pair is cut. The source may start at any multiple of its format's alignment (2 bytes for CS8 / CU8, 4 for CF32), the
//   destination d_iq + 2 n_avail at any multiple of 4. The WIDE MOVES ARE ALIGNED TO THE SOURCE, the side that crosses the link:
//     head  the samples in front of the source's first 16-byte boundary: 0 .. 7 of CS8 / CU8, 0 .. 1 of CF32; one sample per lane
//           (a 2-byte load of CS8 / CU8, an 8-byte one of CF32 as two floats; a 4-byte store), lanes 0 .. 7 of slice 0;
//     body  16 bytes per lane and move, each on a 16-byte boundary of the source: 8 samples of CS8 / CU8 in and 32 bytes out (two
//           16-byte stores), 2 samples of CF32 in and 8 bytes out (one store). The stores are only 4-byte aligned, which global
//           memory allows (the vector types below say so to the compiler). The body's 16-byte groups are what the slices share;
//     tail  what is left behind the last whole group, 0 .. 7 (0 .. 1) samples, moved like the head by lanes 8 .. 15 of slice 0.
//   A CF32 source 4 bytes off an 8-byte boundary never reaches a 16-byte boundary at a sample: it has no head, and its body's
//   16-byte loads are 4-byte aligned (the hardware splits them; the link carries the same bytes in more requests).
// No LDS, no atomics, no scratch. hipcc 7.0, gfx950, -Rpass-analysis=kernel-resource-usage:
//   k_push_convert<CS8>   33 VGPRs, 0 AGPRs, 36 SGPRs, no scratch, no LDS, occupancy 8 waves / SIMD
//   k_push_convert<CU8>   33 VGPRs, 0 AGPRs, 36 SGPRs, no scratch, no LDS, occupancy 8 waves / SIMD
//   k_push_convert<CF32>  24 VGPRs, 0 AGPRs, 36 SGPRs, no scratch, no LDS, occupancy 8 waves / SIMD
struct ConvPair {
    const void* src;     // device-visible address of the caller's samples (or of their raw copy in a device stage)
    void* dst;           // where they go in the stream's device buffer, as int16
    uint32_t n;          // samples
    uint32_t pad;
};
static_assert(sizeof(ConvPair) == sizeof(PushPair), "the pairs half of bulk_table serves either kernel");
typedef uint32_t u32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));   // 16 / 8 bytes at an address that is only 4-byte aligned
typedef uint32_t u32x2_a4 __attribute__((ext_vector_type(2), aligned(4)));
typedef float f32x4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ inline uint32_t iq_word(int16_t i, int16_t q) { return (uint32_t)(uint16_t)i | (uint32_t)(uint16_t)q << 16; }
template <int kFmt>
__device__ inline uint32_t convert_sample(const void* src, uint32_t k) {    // sample k of the block, by narrow loads
    return iq_word(opv_iq_component<kFmt>(src, 2 * (size_t)k), opv_iq_component<kFmt>(src, 2 * (size_t)k + 1));
}
__device__ inline uint32_t convert_word8(int fmt, uint32_t w, int k) {      // sample k (0 / 1) of the four bytes I0 Q0 I1 Q1
    const uint32_t i = w >> (16 * k) & 255u, q = w >> (16 * k + 8) & 255u;
    return fmt == OPV_IQ_CS8 ? iq_word(opv_iq_from_cs8((int8_t)i), opv_iq_from_cs8((int8_t)q))
                             : iq_word(opv_iq_from_cu8((uint8_t)i), opv_iq_from_cu8((uint8_t)q));
}

template <int kFmt>
__global__ __launch_bounds__(256) void k_push_convert(const ConvPair* tab, uint32_t n_pairs, uint32_t slices, ConvPair one) {
    constexpr uint32_t kBytes = kFmt == OPV_IQ_CF32 ? 8u : 2u;              // per sample
    constexpr uint32_t kGroup = 16u / kBytes;                               // samples per 16-byte move
    for (uint32_t w = blockIdx.x; w < n_pairs * slices; w += gridDim.x) {
        const ConvPair p = tab ? tab[w / slices] : one;
        const uint32_t sl = w % slices;
        const uintptr_t a = (uintptr_t)p.src;
        uint32_t head = (a & (kBytes - 1)) ? 0u : (uint32_t)((16u - (a & 15u)) & 15u) / kBytes;
        if (head > p.n) head = p.n;
        const uint32_t groups = (p.n - head) / kGroup, per = (groups + slices - 1) / slices;
        const uint32_t lo = sl * per, hi = lo + per < groups ? lo + per : groups;
        const char* body = (const char*)p.src + (size_t)head * kBytes;
        uint32_t* d = (uint32_t*)p.dst;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) {
            uint32_t* o = d + head + (size_t)i * kGroup;
            if (kFmt == OPV_IQ_CF32) {
                const f32x4_a4 v = *(const f32x4_a4*)(body + (size_t)i * 16);
                u32x2_a4 r;
                r.x = iq_word(opv_iq_from_cf32(v.x), opv_iq_from_cf32(v.y));
                r.y = iq_word(opv_iq_from_cf32(v.z), opv_iq_from_cf32(v.w));
                *(u32x2_a4*)o = r;
            } else {
                const uint4 v = *(const uint4*)(body + (size_t)i * 16);     // (16-byte aligned: the head saw to that)
                u32x4_a4 r0, r1;
                r0.x = convert_word8(kFmt, v.x, 0); r0.y = convert_word8(kFmt, v.x, 1);
                r0.z = convert_word8(kFmt, v.y, 0); r0.w = convert_word8(kFmt, v.y, 1);
                r1.x = convert_word8(kFmt, v.z, 0); r1.y = convert_word8(kFmt, v.z, 1);
                r1.z = convert_word8(kFmt, v.w, 0); r1.w = convert_word8(kFmt, v.w, 1);
                *(u32x4_a4*)o = r0;
                *(u32x4_a4*)(o + 4) = r1;
            }
        }
        if (sl == 0 && threadIdx.x < 16) {                                  // head: lanes 0 .. 7, tail: lanes 8 .. 15
            const uint32_t t = threadIdx.x & 7u, done = head + groups * kGroup;
            if (threadIdx.x < 8) {
                if (t < head) d[t] = convert_sample<kFmt>(p.src, t);
            } else if (done + t < p.n) {
                d[done + t] = convert_sample<kFmt>(p.src, done + t);
            }
        }
    }
}

// k_compact: the retained tails of MANY streams' staging buffers across to their second buffers in one launch, and the streams'
// device contexts re-based (opv_stream_rules.h: iq_rebase, here on the device). Exactly `samples` samples move: what lies
// behind them belongs to the pushes that follow on the copy stream.
struct CompactItem {
    const int* src;      // retained tail in the full buffer (16-byte aligned: `keep` is a multiple of 4 samples)
    int* dst;            // head of the other buffer
    uint32_t samples;
    uint32_t stream;
    uint64_t keep;       // samples dropped in front
};
__global__ __launch_bounds__(256) void k_compact(OpvStream* streams, const CompactItem* items, uint32_t n_items, uint32_t slices) {
    for (uint32_t w = blockIdx.x; w < n_items * slices; w += gridDim.x) {
        const CompactItem it = items[w / slices];
        const uint32_t sl = w % slices;
        const uint32_t quads = it.samples >> 2, per = (quads + slices - 1) / slices;
        const uint32_t lo = sl * per, hi = lo + per < quads ? lo + per : quads;
        const int4* s4 = (const int4*)it.src;
        int4* d4 = (int4*)it.dst;
        for (uint32_t i = lo + threadIdx.x; i < hi; i += 256) d4[i] = s4[i];
        if (sl == 0) {
            if (threadIdx.x < (it.samples & 3u)) it.dst[quads * 4 + threadIdx.x] = it.src[quads * 4 + threadIdx.x];
            if (threadIdx.x == 0) {
                OpvStream& st = streams[it.stream];
                st.iq = (const int16_t*)it.dst;
                st.origin -= it.keep;
                st.n_avail -= it.keep;
                st.iq_base += it.keep;
            }
        }
    }
}

}  // namespace

// grow-only pinned table for the two bulk kernels: [CompactItem x n][PushPair x n], each half read in place by its kernel.
// The items half is rewritten only behind a wait for `stream` (k_compact runs there: compact_streams waits before it fills the
// table), the pairs half only behind a wait for the copy stream (k_push_gather runs there: every batch ends with that wait or is
// settled by the next push, and compact_streams begins with it). A batch that compacts half-way (push_enqueue) runs push_deferred
// -> compact_streams -> the rest: the first gather is waited for before its pairs are rewritten - inside both rules.
static int bulk_table(opv_ctx* c, size_t n, CompactItem** items, PushPair** pairs) {
    const size_t need = n * (sizeof(CompactItem) + sizeof(PushPair));
    if (int r = c->bulk_tab.grow(need, need < 65536 ? 65536 : 2 * need, {c->copy_stream, c->stream})) return r;
    const size_t per = c->bulk_tab.cap / (sizeof(CompactItem) + sizeof(PushPair));
    *items = (CompactItem*)c->bulk_tab.p;
    *pairs = (PushPair*)((char*)c->bulk_tab.p + per * sizeof(CompactItem));
    return OPV_OK;
}

int ensure_iq_buffer(opv_ctx* c, HostStream& h, int which, const char* oom) {
    int16_t*& p = which ? h.d_iq_alt : h.d_iq_owned;
    if (p) return OPV_OK;
    const hipError_t e = hipMalloc((void**)&p, (size_t)c->cfg.max_samples * 4 + 16384);   // + slack for whole-tile reads
    if (e != hipSuccess) { p = nullptr; return alloc_failed(e, "hipMalloc of a stream's IQ buffer", oom); }
    h.iq_cap = c->cfg.max_samples;                         // (a buffer more on a refused call is not a change of the context)
    if (!which && !h.attached) h.d_iq = p;
    return OPV_OK;
}

// Long-running streams: the per-stream device buffers are bounded (opv_cfg.max_samples). When a push would overflow the IQ
// buffer, everything the kernels can no longer touch is dropped (opv_stream_rules.h: iq_keep): the retained tail goes across
// to the stream's second buffer and the two swap. The soft-symbol log and the records are rings on the device and need no host
// action; indices handed to the caller stay absolute. For MANY streams (a live server's staging buffers fill in the same round) as
// for one: one wait, one launch; an item of no samples still re-bases its stream. Streams that cannot be compacted (nothing
// consumed yet) are left to the caller's own check.
static int compact_streams(opv_ctx* c, const std::vector<int>& which) {
    HIPCHK(hipStreamSynchronize(c->copy_stream));         // copies enqueued earlier land first
    if (int r = c->refresh()) return r;                    // (once per round: the mirror stays valid, re-based below, for the next call)
    HIPCHK(hipStreamSynchronize(c->stream));               // a k_compact launched since that refresh has read its items
    CompactItem* items = nullptr;
    PushPair* pairs = nullptr;
    if (int r = bulk_table(c, (size_t)c->n_streams, &items, &pairs)) return r;
    uint32_t m = 0, most = 0;
    for (int s : which) {
        HostStream& h = c->hs[s];
        OpvStream& st = c->mirror[s];
        const uint64_t keep = iq_keep(st.origin);
        if (keep == 0 || !h.d_iq_owned) continue;
        const uint64_t len = h.n_avail - keep;             // samples to retain (less than two chunks in steady state)
        if (int r = ensure_iq_buffer(c, h, 1)) return r;
        items[m++] = {(const int*)(h.d_iq_owned + 2 * keep), (int*)h.d_iq_alt, (uint32_t)len, (uint32_t)s, keep};
        if ((uint32_t)len > most) most = (uint32_t)len;
        std::swap(h.d_iq_owned, h.d_iq_alt);
        h.d_iq = h.d_iq_owned;
        iq_rebase(keep, &h.n_avail, &h.last_round_avail, &st);
        h.dirty = true;                                    // (iq and n_avail reach the device with the next round's inputs)
        st.iq = h.d_iq;
    }
    if (m) {
        void* d_items = nullptr;
        HIPCHK(hipHostGetDevicePointer(&d_items, items, 0));
        const LaunchShape l = table_launch(m, most, 4, 2048);          // (samples: one 16-byte move is 4 of them)
        k_compact<<<l.grid, 256, 0, c->stream>>>(c->d_streams, (const CompactItem*)d_items, m, l.slices);   // in stream order before the next kernels
        HIPCHK(hipGetLastError());
    }
    return OPV_OK;
}

// who may be pushed to: the checks of `which` in this order (opv_flush and opv_attach_device_iq make the ones that apply to them)
enum { ADMIT_UNATTACHED = 1, ADMIT_UNFLUSHED = 2, ADMIT_NO_SOFT = 4, ADMIT_PUSH = 7 };
static int push_admit(const HostStream& h, int which = ADMIT_PUSH) {
    if ((which & ADMIT_UNATTACHED) && h.attached) return fail(OPV_ESTATE, "stream has an attached device capture");
    if ((which & ADMIT_UNFLUSHED) && h.eof) return fail(OPV_ESTATE, "push after flush");
    if ((which & ADMIT_NO_SOFT) && h.soft_tapped) return fail(OPV_ESTATE, "stream holds staged soft symbols (opv_tap_push_soft; reset it first)");
    return OPV_OK;
}
static const char kNoRoom[] = "opv_cfg.max_samples exceeded (unprocessed samples + this push do not fit; "
                              "call opv_process between pushes or raise max_samples)";

// a block on its way into a stream: `bytes` of the SOURCE, in format `fmt` (one format per call: the blocks of a batch share it)
struct DeferredCopy { void* dst; const void* src; size_t bytes; int fmt; };
static int push_deferred(opv_ctx* c, const std::vector<DeferredCopy>& copies);

// A typed block (fmt != OPV_IQ_CS16) always comes with `defer`: it moves with its batch, through k_push_convert. Capacity,
// compaction, n_avail and admission count samples and do not know the format.
static int push_enqueue(opv_ctx* c, int s, const void* iq, size_t n, std::vector<DeferredCopy>* defer = nullptr, int fmt = OPV_IQ_CS16) {
    if (int r = check_stream(c, s)) return r;
    HostStream& h = c->hs[s];
    if (int r = push_admit(h)) return r;
    if (n == 0) return OPV_OK;
    if (!iq) return fail(OPV_EINVAL, "null IQ pointer");
    if (fmt != OPV_IQ_CS16 && ((uintptr_t)iq & (opv_iq_align_of(fmt) - 1)) != 0)
        return fail(OPV_EINVAL, "typed push: the source is not aligned for its format (2 bytes for cs8 / cu8, 4 for cf32)");
    if (h.n_avail + n > c->cfg.max_samples) {
        if (defer && !defer->empty()) {                // blocks of this batch not yet under way (one of them may be this stream's) go first
            if (int r = push_deferred(c, *defer)) return r;
            defer->clear();
        }
        if (int r = compact_streams(c, {s})) return r;
        if (h.n_avail + n > c->cfg.max_samples) return fail(OPV_ECAPACITY, kNoRoom);
    }
    if (int r = ensure_iq_buffer(c, h, 0)) return r;
    // On the copy stream: the kernels of an opv_process still in flight only read samples below the
    // n_avail they were launched with, so new samples land behind them while they run (H2D over
    // PCIe overlaps compute).
    if (defer) defer->push_back({h.d_iq_owned + 2 * h.n_avail, iq, n * opv_iq_bytes_of(fmt), fmt});   // (opv_push_iq_batch moves its blocks together)
    else HIPCHK(hipMemcpyAsync(h.d_iq_owned + 2 * h.n_avail, iq, n * 4, hipMemcpyHostToDevice, c->copy_stream));
    h.n_avail += n;
    h.dirty = true;
    h.iq_seen = true;
    return OPV_OK;
}

static int convert_launch(int fmt, const ConvPair* d_tab, uint32_t m, LaunchShape l, ConvPair one, hipStream_t on) {
    switch (fmt) {
    case OPV_IQ_CS8: k_push_convert<OPV_IQ_CS8><<<l.grid, 256, 0, on>>>(d_tab, m, l.slices, one); break;
    case OPV_IQ_CU8: k_push_convert<OPV_IQ_CU8><<<l.grid, 256, 0, on>>>(d_tab, m, l.slices, one); break;
    case OPV_IQ_CF32: k_push_convert<OPV_IQ_CF32><<<l.grid, 256, 0, on>>>(d_tab, m, l.slices, one); break;
    default: return fail(OPV_EINVAL, "no convert kernel for this format");   // (a missing kernel is an error, never a quiet copy)
    }
    HIPCHK(hipGetLastError());
    return OPV_OK;
}

// One block through k_push_convert on `on`, its pair handed over by value (opv_wb_internal.h: the wideband door's and the scan's
// typed pushes, opv_convert_iq_device). In pieces of at most 2^31 source bytes: a pair counts in 32 bits.
int opv_int_convert_launch(int fmt, const void* d_src, int16_t* d_dst, size_t n, hipStream_t on, uint32_t grid_cap) {
    const size_t bytes = opv_iq_bytes_of(fmt), piece = ((size_t)1 << 31) / (bytes ? bytes : 1);
    for (size_t at = 0; at < n; at += piece) {
        const uint32_t k = (uint32_t)(n - at < piece ? n - at : piece);
        const ConvPair one = {(const char*)d_src + at * bytes, d_dst + 2 * at, k, 0};
        if (int r = convert_launch(fmt, nullptr, 1, table_launch(1, (uint32_t)(k * bytes), 16, grid_cap), one, on)) return r;
    }
    return OPV_OK;
}

// The deferred blocks of one TYPED batch (cs8, cu8 or cf32: one format per call): ONE k_push_convert launch on the copy stream
// serves them all. A block in pinned memory of this device is read in place, through the table; anything else - pageable memory,
// pinned memory of another device, 2^32 bytes or more, every block under OPV_PUSH_NO_GATHER - is first copied RAW into the
// context's grow-only device stage and converted from there by the same launch. The stage is rewritten under the rule of the
// table's pairs half (bulk_table): only behind a wait for the copy stream.
static int push_convert_deferred(opv_ctx* c, const std::vector<DeferredCopy>& copies) {
    const int fmt = copies[0].fmt;
    const size_t per = opv_iq_bytes_of(fmt);
    CompactItem* items = nullptr;
    PushPair* table = nullptr;
    if (int r = bulk_table(c, copies.size() > (size_t)c->n_streams ? copies.size() : (size_t)c->n_streams, &items, &table)) return r;
    ConvPair* pairs = (ConvPair*)table;
    std::vector<const void*> view(copies.size(), nullptr);
    size_t stage_bytes = 0;
    bool in_place = false;
    for (size_t i = 0; i < copies.size(); ++i) {
        const DeferredCopy& k = copies[i];
        if (c->push_gather && k.bytes < (1ull << 32)) view[i] = opv_int_pinned_view(k.src, c->cfg.device);
        if (view[i]) in_place = true;
        else stage_bytes += (k.bytes + 15) & ~(size_t)15;
    }
    if (int r = c->push_stage.grow(stage_bytes, stage_bytes < (1u << 20) ? (1u << 20) : stage_bytes + stage_bytes / 4, {c->copy_stream})) return r;
    uint32_t m = 0, most = 0;
    size_t off = 0;
    for (size_t i = 0; i < copies.size(); ++i) {
        const DeferredCopy& k = copies[i];
        const void* src = view[i];
        const size_t n = k.bytes / per;
        if (!src) {
            HIPCHK(hipMemcpyAsync(c->push_stage.p + off, k.src, k.bytes, hipMemcpyHostToDevice, c->copy_stream));
            src = c->push_stage.p + off;
            off += (k.bytes + 15) & ~(size_t)15;
        }
        const size_t b = k.bytes < 0xffffffffull ? k.bytes : 0xffffffffull;
        pairs[m++] = {src, k.dst, (uint32_t)n, 0};         // (n < 2^31: push_enqueue admitted it under opv_cfg.max_samples)
        if ((uint32_t)b > most) most = (uint32_t)b;
    }
    if (m) {
        void* d_pairs = nullptr;
        HIPCHK(hipHostGetDevicePointer(&d_pairs, pairs, 0));
        // the small grid of push_deferred, for its reason, while a block is read across the link; a launch that only reads the stage
        // has the device's memory on both sides
        const LaunchShape l = table_launch(m, most, 16, in_place ? c->push_gather_blocks : 2048);
        if (int r = convert_launch(fmt, (const ConvPair*)d_pairs, m, l, ConvPair{}, c->copy_stream)) return r;
    }
    return OPV_OK;
}

// The deferred copies of one batch. Blocks in pinned (device-visible) host memory go through ONE gather kernel on the copy
// stream; anything else - pageable memory, a source that is not 4-byte aligned - takes hipMemcpyAsync as before.
static int push_deferred(opv_ctx* c, const std::vector<DeferredCopy>& copies) {
    if (copies.empty()) return OPV_OK;
    if (copies[0].fmt != OPV_IQ_CS16) return push_convert_deferred(c, copies);
    CompactItem* items = nullptr;
    PushPair* pairs = nullptr;
    uint32_t m = 0, most = 0;
    const bool try_gather = copies.size() >= 2 && c->push_gather;
    if (try_gather)
        if (int r = bulk_table(c, copies.size() > (size_t)c->n_streams ? copies.size() : (size_t)c->n_streams, &items, &pairs)) return r;
    for (const DeferredCopy& k : copies) {
        bool gathered = false;
        if (try_gather && ((uintptr_t)k.src & 3u) == 0 && k.bytes < (1ull << 32)) {
            hipPointerAttribute_t at;
            // (pinned memory that belongs to ANOTHER device's context is left to hipMemcpyAsync: whether this device may read it in a
            // kernel depends on how it was allocated, and a wrong guess is a page fault, not an error code)
            if (hipPointerGetAttributes(&at, k.src) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer && at.device == c->cfg.device) {
                const uint32_t wide = (((uintptr_t)at.devicePointer | (uintptr_t)k.dst) & 15u) == 0 ? 1u : 0u;
                pairs[m++] = {at.devicePointer, k.dst, (uint32_t)k.bytes, wide};
                if ((uint32_t)k.bytes > most) most = (uint32_t)k.bytes;
                gathered = true;
            } else {
                (void)hipGetLastError();                   // (pageable memory: "invalid value" - not an error of ours)
            }
        }
        if (!gathered) HIPCHK(hipMemcpyAsync(k.dst, k.src, k.bytes, hipMemcpyHostToDevice, c->copy_stream));
    }
    if (m) {
        void* d_pairs = nullptr;
        HIPCHK(hipHostGetDevicePointer(&d_pairs, pairs, 0));
        // A SMALL grid on purpose: PCIe's latency x bandwidth product is ~120 KB, and 32 blocks x 256 lanes x 16 B = 128 KB of
        // reads in flight already run the link at its rate (56 GB/s; 16 blocks: 45). More does not move more - but it fills the
        // memory system's request queues with reads that take microseconds, and the kernels of an opv_process running beside an
        // asynchronous batch then crawl (5120 streams: round kernels 3.5 ms beside 32 blocks, 18 ms beside 128, 27 ms beside 256).
        const LaunchShape l = table_launch(m, most, 16, c->push_gather_blocks);   // work items of <= 347 KB / slices: an even load over the blocks
        k_push_gather<<<l.grid, 256, 0, c->copy_stream>>>((const PushPair*)d_pairs, m, l.slices);
        HIPCHK(hipGetLastError());
    }
    return OPV_OK;
}

// the end of a push: the buffers are the caller's again after a host wait for the copy stream, or the moves stay under way
// behind an event (opv_process orders its kernels behind it; opv_push_wait and every other push entry point wait on the host)
static int push_finish(opv_ctx* c, bool wait) {
    if (wait) {
        HIPCHK(hipStreamSynchronize(c->copy_stream));
    } else {
        if (!c->push_ev) HIPCHK(hipEventCreateWithFlags(&c->push_ev, hipEventDisableTiming));
        HIPCHK(hipEventRecord(c->push_ev, c->copy_stream));
        c->push_pending = true;
    }
    return OPV_OK;
}

extern "C" int opv_push_wait(opv_ctx* c) {
    if (!c) return fail(OPV_EINVAL, "null context");
    return settle_pushes(c);
}

extern "C" int opv_push_iq(opv_ctx* c, int s, const int16_t* iq, size_t n) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (int r = settle_pushes(c)) return r;
    if (int r = push_enqueue(c, s, iq, n)) return r;
    // The caller keeps ownership of `iq`: the copy must have left the host buffer before we return,
    // which is a wait for THIS copy only, not for the kernels.
    return push_finish(c, true);
}

static int push_batch(opv_ctx* c, int count, const int* streams, const void* const* iq, const size_t* n_samples, bool wait, int fmt = OPV_IQ_CS16) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (count < 0 || (count > 0 && (!streams || !iq || !n_samples))) return fail(OPV_EINVAL, "opv_push_iq_batch: bad arguments");
    if (int r = settle_pushes(c)) return r;                // (the table of an earlier asynchronous batch may still be read)
    // staging buffers that would overflow are compacted together first (a live server's streams fill in the same round)
    std::vector<int> full;
    for (int i = 0; i < count; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= c->n_streams) continue;          // (reported by push_enqueue below, at its place in the order)
        const HostStream& h = c->hs[s];
        if (!h.attached && !h.eof && n_samples[i] && h.n_avail + n_samples[i] > c->cfg.max_samples) full.push_back(s);
    }
    if (!full.empty())
        if (int r = compact_streams(c, full)) return r;
    std::vector<DeferredCopy> copies;
    copies.reserve((size_t)count);
    int rc = OPV_OK;
    for (int i = 0; i < count && rc == OPV_OK; ++i) rc = push_enqueue(c, streams[i], iq[i], n_samples[i], &copies, fmt);
    const int rc2 = push_deferred(c, copies);              // (streams before an error have been pushed)
    if (int r = push_finish(c, wait || rc != OPV_OK || rc2 != OPV_OK)) return r;   // one wait (or one event) for all copies
    return rc != OPV_OK ? rc : rc2;
}

extern "C" int opv_push_iq_batch(opv_ctx* c, int count, const int* streams, const int16_t* const* iq, const size_t* n) { return push_batch(c, count, streams, (const void* const*)iq, n, true); }
extern "C" int opv_push_iq_batch_async(opv_ctx* c, int count, const int* streams, const int16_t* const* iq, const size_t* n) { return push_batch(c, count, streams, (const void* const*)iq, n, false); }

// ---- typed pushes (include/opv_demod.h): one format per call. CS16 IS the int16 path - the old entry point, the old kernel, the old
// arguments; the other formats take push_batch with their format, a single block as a batch of one.
static int fmt_refusal(int fmt) {
    return opv_iq_align_of(fmt) ? OPV_OK : fail(OPV_EINVAL, "unknown sample format (OPV_IQ_CS16, OPV_IQ_CS8, OPV_IQ_CU8 or OPV_IQ_CF32)");
}

extern "C" int opv_push_iq_fmt(opv_ctx* c, int s, int fmt, const void* samples, size_t n) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (int r = fmt_refusal(fmt)) return r;
    if (fmt == OPV_IQ_CS16) return opv_push_iq(c, s, (const int16_t*)samples, n);
    return push_batch(c, 1, &s, &samples, &n, true, fmt);
}

static int push_batch_fmt(opv_ctx* c, int fmt, int count, const int* streams, const void* const* samples, const size_t* n, bool wait) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (int r = fmt_refusal(fmt)) return r;
    return push_batch(c, count, streams, samples, n, wait, fmt);   // (CS16: fmt's default, every block through push_deferred's int16 half)
}
extern "C" int opv_push_iq_batch_fmt(opv_ctx* c, int fmt, int count, const int* streams, const void* const* samples, const size_t* n) { return push_batch_fmt(c, fmt, count, streams, samples, n, true); }
extern "C" int opv_push_iq_batch_fmt_async(opv_ctx* c, int fmt, int count, const int* streams, const void* const* samples, const size_t* n) { return push_batch_fmt(c, fmt, count, streams, samples, n, false); }

// on the context's stream (kernels, in order), asynchronously like opv_channel_device; CS16 is a copy
extern "C" int opv_convert_iq_device(opv_ctx* c, int fmt, const void* d_in, int16_t* d_out, size_t n) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (int r = fmt_refusal(fmt)) return r;
    if (n == 0) return OPV_OK;
    if (!d_in || !d_out) return fail(OPV_EINVAL, "opv_convert_iq_device: null device pointer");
    if (((uintptr_t)d_in & (opv_iq_align_of(fmt) - 1)) != 0 || ((uintptr_t)d_out & 3u) != 0)
        return fail(OPV_EINVAL, "opv_convert_iq_device: the input must be aligned for its format, the output to 4 bytes");
    HIPCHK(hipSetDevice(c->cfg.device));
    if (fmt == OPV_IQ_CS16) {
        HIPCHK(hipMemcpyAsync(d_out, d_in, n * 4, hipMemcpyDeviceToDevice, c->stream));
        return OPV_OK;
    }
    return opv_int_convert_launch(fmt, d_in, d_out, n, c->stream, 2048);
}

extern "C" int opv_flush(opv_ctx* c, int s) {
    if (int r = check_stream(c, s)) return r;
    if (int r = push_admit(c->hs[s], ADMIT_NO_SOFT)) return r;
    c->hs[s].eof = 1;
    c->hs[s].dirty = true;
    return OPV_OK;
}

extern "C" int opv_attach_device_iq(opv_ctx* c, int s, const int16_t* d_iq, size_t n, int eof) {
    if (int r = check_stream(c, s)) return r;
    HostStream& h = c->hs[s];
    if (h.d_iq_owned && h.n_avail && !h.attached) return fail(OPV_ESTATE, "stream already has pushed samples (reset it first)");
    if (int r = push_admit(h, ADMIT_NO_SOFT)) return r;
    if (!d_iq && n) return fail(OPV_EINVAL, "null device pointer");
    if (((uintptr_t)d_iq & 15u) != 0) return fail(OPV_EINVAL, "device IQ pointer must be 16-byte aligned");
    if (n > c->cfg.max_samples) return fail(OPV_ECAPACITY, "opv_cfg.max_samples exceeded");
    if (h.attached && (d_iq != h.d_iq || n < h.n_avail)) return fail(OPV_ESTATE, "attached capture may only grow");
    h.attached = true;
    h.iq_seen = true;
    h.d_iq = d_iq;
    h.n_avail = n;
    h.eof = eof ? 1 : 0;
    h.dirty = true;
    return OPV_OK;
}

// ---- the wideband front door's way in (opv_wb_internal.h; opv_wideband.hip holds the object, k_wideband.hip the kernel) ----------
int opv_int_door(opv_ctx* c, OpvCtxDoor* out) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (!c->wb.p) {
        c->wb.p = std::make_shared<OpvWbShared>();
        c->wb.p->owned.assign((size_t)c->n_streams, 0);
    }
    out->n_streams = c->n_streams;
    out->device = c->cfg.device;
    out->copy_stream = c->copy_stream;
    out->shared = c->wb.p;
    return OPV_OK;
}

// (no wait for an asynchronous push still under way: a wideband object's table, carry and staging buffer are its own and are
// handed on in copy-stream order, and opv_int_push_reserve waits by itself before a tail is moved. So the K-channel pushes of
// many objects queue up behind each other on the device while the host goes on.)
int opv_int_push_begin(opv_ctx* c) { HIPCHK(hipSetDevice(c->cfg.device)); return OPV_OK; }

int opv_int_push_reserve(opv_ctx* c, int count, const int* streams, const uint32_t* n, int** dst) {
    // push_enqueue's rules, for all streams before anything moves: first what refuses the call ...
    std::vector<int> full;
    for (int i = 0; i < count; ++i) {
        if (int r = check_stream(c, streams[i])) return r;
        const HostStream& h = c->hs[streams[i]];
        if (int r = push_admit(h)) return r;
        if (n[i] && h.n_avail + n[i] > c->cfg.max_samples) full.push_back(streams[i]);
    }
    if (!full.empty()) {
        HIPCHK(hipStreamSynchronize(c->copy_stream));      // samples enqueued earlier land before a tail is moved
        if (int r = c->refresh()) return r;
        for (int i = 0; i < count; ++i) {                  // would compaction make the room?
            const HostStream& h = c->hs[streams[i]];
            const uint64_t keep = h.d_iq_owned ? iq_keep(c->mirror[streams[i]].origin) : 0;
            if (n[i] && h.n_avail - keep + n[i] > c->cfg.max_samples) return fail(OPV_ECAPACITY, kNoRoom);
        }
        // ... then the changes: compaction, lazy allocation, the reservation itself
        if (int r = compact_streams(c, full)) return r;
    }
    for (int i = 0; i < count; ++i)
        if (int r = ensure_iq_buffer(c, c->hs[streams[i]], 0, "wideband push: IQ buffer")) return r;
    for (int i = 0; i < count; ++i) {
        HostStream& h = c->hs[streams[i]];
        dst[i] = (int*)(h.d_iq_owned + 2 * h.n_avail);
        if (n[i]) {
            h.n_avail += n[i];
            h.dirty = true;
            h.iq_seen = true;
        }
    }
    return OPV_OK;
}

int opv_int_push_end(opv_ctx* c, bool wait) { return push_finish(c, wait); }

extern "C" long opv_tap_iq(opv_ctx* c, int s, uint64_t first, int16_t* out, size_t cap) {
    if (int r = check_stream(c, s)) return r;
    if (!out && cap) return fail(OPV_EINVAL, "null out");
    if (int r = settle_pushes(c)) return r;
    HIPCHK(hipStreamSynchronize(c->copy_stream));
    if (int r = c->refresh()) return r;
    const HostStream& h = c->hs[s];
    const uint64_t base = c->mirror[s].iq_base;
    if (first < base || first >= base + h.n_avail || !h.d_iq) return 0;
    uint64_t n = base + h.n_avail - first;
    if (n > cap) n = cap;
    HIPCHK(hipMemcpy(out, h.d_iq + 2 * (first - base), n * 4, hipMemcpyDeviceToHost));
    return (long)n;
}
