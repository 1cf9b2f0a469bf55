// k_stream_pack.hip — the two bulk moves of stream migration (opv_export_streams / opv_import_streams, opv_capi.hip).
//
// No counterpart in the reference, whose streams are processes and cannot leave them ("Checkpoint / resume: none").
//
// k_stream_pack:   the carried tails of MANY streams - unconsumed IQ, the soft symbols the tracker can still read, unpopped frame
//                  records with their bytes, metrics and scales, unread events, the chunk log - out of their rings into ONE contiguous
//                  staging buffer, which one device-to-host copy then takes across.
// k_stream_unpack: the reverse behind one host-to-device copy, into the rings of the destination slots (whose capacities may differ:
//                  the host recomputed every ring position from the absolute indices), plus what opv_reset_stream does for a slot -
//                  the INT32_MIN fill of its metrics ring - and the re-based OpvStream itself.
//
// Both are table-driven like k_push_gather / k_compact (opv_capi.hip): the tables live in pinned host memory and are read in place.
// One work item is one OpvMove, a contiguous run of at most OPV_MOVE_PIECE bytes (the host un-wraps rings and cuts long runs), so
// the kernels know nothing about rings and every address they touch has been bounds-checked on the host. 16-byte moves where both
// ends are 16-byte aligned (IQ, soft symbols - their tails start at multiples of four samples / two symbols -, frame and event
// records), 4-byte moves where they are 4-byte aligned (metrics, scales, chunk log), bytes otherwise (134-byte frames).
// Bytes: every carried byte is read once and written once; a stream with one 40 ms chunk pending is ~0.4 MB.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opv_device.h"

namespace {

__device__ inline void move_run(const OpvMove m) {
    const uint32_t t = threadIdx.x;
    const uintptr_t both = (uintptr_t)m.src | (uintptr_t)m.dst;
    uint32_t done = 0;                                   // bytes moved by the wide part
    if ((both & 15u) == 0) {
        const uint32_t quads = m.bytes >> 4;
        const int4* s4 = (const int4*)m.src;
        int4* d4 = (int4*)m.dst;
        for (uint32_t i = t; i < quads; i += blockDim.x) d4[i] = s4[i];
        done = quads << 4;
    } else if ((both & 3u) == 0) {
        const uint32_t words = m.bytes >> 2;
        const int* s1 = (const int*)m.src;
        int* d1 = (int*)m.dst;
        for (uint32_t i = t; i < words; i += blockDim.x) d1[i] = s1[i];
        done = words << 2;
    }
    const uint8_t* sb = (const uint8_t*)m.src;
    uint8_t* db = (uint8_t*)m.dst;
    for (uint32_t i = done + t; i < m.bytes; i += blockDim.x) db[i] = sb[i];
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_stream_pack(const OpvMove* __restrict__ moves, uint32_t n_moves) {
    for (uint32_t w = blockIdx.x; w < n_moves; w += gridDim.x) move_run(moves[w]);
}

extern "C" __global__ __launch_bounds__(256) void k_stream_unpack(OpvStream* __restrict__ streams, int32_t* __restrict__ counts,
                                                                  const OpvUnpackItem* __restrict__ items, uint32_t n_items,
                                                                  const OpvMove* __restrict__ moves, uint32_t n_moves) {
    for (uint32_t w = blockIdx.x; w < n_items + n_moves; w += gridDim.x) {
        if (w >= n_items) { move_run(moves[w - n_items]); continue; }
        // one workgroup per imported stream: the slot's context and the part of its metrics ring that no move writes
        const OpvUnpackItem& it = items[w];
        const uint32_t cap = it.st.cap_frames, first = it.live_first, live = it.live_n;
        int32_t* const metrics = it.st.metrics;
        for (uint32_t i = threadIdx.x; i < cap; i += blockDim.x) {
            const uint32_t behind = i >= first ? i - first : i + cap - first;   // distance from the first unpopped frame, around the ring
            if (behind >= live) metrics[i] = INT32_MIN;
        }
        static_assert(sizeof(OpvStream) % 8 == 0, "OpvStream is moved in 8-byte words");
        const uint64_t* s8 = (const uint64_t*)&it.st;
        uint64_t* d8 = (uint64_t*)&streams[it.stream];
        for (uint32_t i = threadIdx.x; i < sizeof(OpvStream) / 8; i += blockDim.x) d8[i] = s8[i];
        if (threadIdx.x == 0) counts[it.stream] = (int32_t)it.st.n_frames;       // (what k_collect_counts would say: zero-copy consumers)
    }
}
