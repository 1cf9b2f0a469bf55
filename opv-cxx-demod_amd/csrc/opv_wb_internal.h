// opv_wb_internal.h — the door between the context (opv_ctx.h, opv_push.hip) and the wideband front door (opv_wideband.hip, k_wideband.hip).
// The wideband object never sees opv_ctx's fields: it asks the context to reserve room in its streams' device buffers under
// the rules of push_enqueue, launches its own kernel on the copy stream, and tells the context when it has.
#ifndef OPV_WB_INTERNAL_H
#define OPV_WB_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <memory>
#include <vector>

#include "../../include/opv_demod.h"

struct opv_ctx;

// What both front-door kernels are handed, by value, filled once by wb_push (opv_wideband.hip). Sample n of the object (0 = the first
// sample ever pushed) has the absolute index first_sample + n; this push holds samples [n_before, n_before + n_new).
struct OpvWbHead {
    const int* src;          // this push: n_new packed (I | Q << 16) samples, device-visible (pinned host, staging copy or device)
    const int* hist_in;      // the hist_len samples in front of src[0] (the carry of the pushes so far)
    int* hist_out;           // the other carry buffer: the last min(n_before + n_new, carry) samples, written by block (0, 0)
    const int16_t* lo;       // T[4096]
    const void* taps;        // the taps as the kind's kernel reads them: h[L] widened to int32 (k_wb_ddc), or the phase-major int16 table
                             // tab[U][rowlen], tab[p][j] = taps[p + j U], zero-padded, rows 8-byte aligned (k_wbr_ddc)
    const uint32_t* inc;     // inc[K]
    int* const* dst;         // dst[K]: where each channel's first output of this push goes (device-visible table)
    uint64_t n_before;       // N before this push
    uint32_t a0_lo;          // low 32 bits of first_sample + n_before: all the closed-form phase needs
    uint32_t n_new, hist_len, n_out;
    uint32_t K, S;
    uint32_t kper;           // channels per blockIdx.y
};
constexpr uint32_t OPV_WB_SPAN = 4096;     // wide samples (history included) a workgroup holds in LDS
constexpr uint32_t OPV_WB_THREADS = 256;

// Arguments of k_wb_ddc (csrc/k_wideband.hip): the integer door, carry = L - 1.
struct OpvWbArgs : OpvWbHead {
    uint64_t r0;             // first output index of this push = ceil(n_before / D)
    uint32_t D, L;
    uint32_t tile;           // outputs per workgroup (<= 256)
    uint32_t lpad;           // L - 1 rounded up to a multiple of D
    uint32_t rowlen;         // tile + lpad / D: entries per decimation phase of the workgroup's span; D * rowlen <= OPV_WB_SPAN
};
extern "C" __global__ void k_wb_ddc(OpvWbArgs a);
struct OpvWbDevSched;        // opv_wb_rules.h: one channel's LO schedule as the kernels of one push read it
extern "C" __global__ void k_wb_ddc_tuned(OpvWbArgs a, const OpvWbDevSched* sched);      // the same behind an LO schedule; a.inc is not read

// Arguments of k_wbr_ddc (csrc/k_wideband_rational.hip): the rational door, wide rate 2 168 000 x M / U, carry = J - 1. Output r of
// the object reads wide samples n_r - j, j = 0 .. J - 1, with n_r = floor(r M / U), against row p_r = (r M) mod U of the phase-major
// tap table. Output i of this push is r0 + i; the host hands over (n_r0, p_r0) and the device steps from there in 64 bits.
struct OpvWbrArgs : OpvWbHead {
    uint32_t nrel0;          // n_r0 - n_before: index within src of the first output's newest sample (< n_new when n_out > 0)
    uint32_t p0;             // p_r0
    uint32_t M, U, J;
    uint32_t rowlen;         // J rounded up to a multiple of 4
    uint32_t tile;           // outputs per workgroup (<= 256): rowlen + floor(tile M / U) <= OPV_WB_SPAN
};
extern "C" __global__ void k_wbr_ddc(OpvWbrArgs a);
extern "C" __global__ void k_wbr_ddc_tuned(OpvWbrArgs a, const OpvWbDevSched* sched);

// ---- what the context offers (defined at the end of opv_push.hip; opv_int_fail in opv_capi.hip)
int opv_int_fail(int code, const char* what, hipError_t e = hipSuccess);   // sets opv_last_error, returns code
// a failed HIP call is OPV_EHIP with the call's text and the runtime's; the create paths first destroy the half-made object:
// on_failure(error, text of the call) does that and says what to return
#define HIPCHK_OR(on_failure, expr)                                  \
    do {                                                             \
        hipError_t _e = (expr);                                      \
        if (_e != hipSuccess) return on_failure(_e, #expr);          \
    } while (0)
#define HIPCHK(expr)                                                      \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) return opv_int_fail(OPV_EHIP, #expr, _e);   \
    } while (0)
// ---- the source of a push, for every object that reads a caller's block on the copy stream (opv_wideband.hip, opv_scan.hip)
enum class OpvSrc { Host, Device };
struct OpvStage {                 // pageable sources: the block is copied here first (grow-only)
    int* d = nullptr;
    size_t cap = 0;
};
// The block of n samples as the device sees it, in *src: a device pointer as it is; pinned host memory through its device address
// (the kernel reads the caller's block across PCIe, once); pageable memory through the staging buffer, grown here if it is too
// small, after a wait for the copy stream. *staged then tells the caller to enqueue the copy into stage->d in front of its launch.
// Nothing is enqueued here, and nothing of the object's state changes.
inline int opv_int_source(const int16_t* iq, size_t n, OpvSrc kind, int device, hipStream_t copy_stream, OpvStage* stage, const int** src,
                          bool* staged) {
    *staged = false;
    if (kind == OpvSrc::Device) {
        *src = (const int*)iq;
        return 0;
    }
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, iq) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer && at.device == device) {
        *src = (const int*)at.devicePointer;
        return 0;
    }
    (void)hipGetLastError();                                            // (pageable memory: "invalid value" - not an error of ours)
    if (stage->cap < n) {
        HIPCHK(hipStreamSynchronize(copy_stream));
        if (stage->d) HIPCHK(hipFree(stage->d));
        stage->d = nullptr;
        stage->cap = 0;
        HIPCHK(hipMalloc(&stage->d, n * 4));
        stage->cap = n;
    }
    *src = stage->d;
    *staged = true;
    return 0;
}

// ---- a TYPED block (include/opv_demod.h: cs8, cu8, cf32) for the same objects: it is converted to int16 INTO the object's stage
// and the push goes on as a device-pointer push from there; the bank kernels never see a format.
// k_push_convert for one block (opv_push.hip): n samples of `fmt` at d_src (device-visible, aligned for the format) to int16 at
// d_dst, enqueued on `on`; grid_cap: the small grid of the gather kernel where d_src lies across the link
int opv_int_convert_launch(int fmt, const void* d_src, int16_t* d_dst, size_t n, hipStream_t on, uint32_t grid_cap);
// the device-visible address of a block in pinned host memory of `device`; nullptr for pageable memory and for pinned memory that
// belongs to ANOTHER device's context (whether this device may read that in a kernel depends on how it was allocated, and a wrong
// guess is a page fault, not an error code)
inline const void* opv_int_pinned_view(const void* p, int device) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) == hipSuccess && at.type == hipMemoryTypeHost && at.devicePointer && at.device == device) return at.devicePointer;
    (void)hipGetLastError();                                            // (pageable memory: "invalid value" - not an error of ours)
    return nullptr;
}
struct OpvTypedSrc {
    const void* d_raw = nullptr;  // what the convert kernel reads: the caller's pinned block in place, or its raw copy in the stage
    bool copy_raw = false;        // pageable: the raw bytes are copied behind the converted samples' place first
    size_t raw_bytes = 0;
};
// The stage grown (as opv_int_source grows it) to n converted samples and, for a pageable source, the raw block behind them.
// Nothing is enqueued here, and nothing of the object's state changes; sample_bytes: include/opv_demod.h's opv_iq_sample_bytes(fmt).
inline int opv_int_source_fmt(const void* in, size_t n, size_t sample_bytes, int device, hipStream_t copy_stream, OpvStage* stage,
                              OpvTypedSrc* out) {
    out->raw_bytes = n * sample_bytes;
    size_t need = n;                                                    // (OpvStage counts in samples of 4 bytes)
    out->d_raw = opv_int_pinned_view(in, device);
    if (!out->d_raw) {
        out->copy_raw = true;
        need = ((n + 3) & ~(size_t)3) + (out->raw_bytes + 3) / 4;       // the raw copy starts on a 16-byte boundary
    }
    if (stage->cap < need) {
        HIPCHK(hipStreamSynchronize(copy_stream));
        if (stage->d) HIPCHK(hipFree(stage->d));
        stage->d = nullptr;
        stage->cap = 0;
        HIPCHK(hipMalloc(&stage->d, need * 4));
        stage->cap = need;
    }
    if (out->copy_raw) out->d_raw = stage->d + ((n + 3) & ~(size_t)3);
    return 0;
}
// ... and the block on its way, on the copy stream in front of the object's own launch: stage->d then holds n int16 samples
inline int opv_int_convert_enqueue(const void* in, size_t n, int fmt, const OpvTypedSrc& t, OpvStage* stage, hipStream_t copy_stream) {
    if (t.copy_raw) HIPCHK(hipMemcpyAsync((void*)t.d_raw, in, t.raw_bytes, hipMemcpyHostToDevice, copy_stream));
    return opv_int_convert_launch(fmt, t.d_raw, (int16_t*)stage->d, n, copy_stream, t.copy_raw ? 2048u : 32u);
}

// What a context and its wideband objects share, and what outlives whichever of them goes first: a wideband object destroyed
// (or used) after its context finds ctx_alive false and touches nothing of the context.
struct OpvWbShared {
    std::vector<uint8_t> owned;   // [n_streams]: 1 while a live wideband object feeds the stream
    bool ctx_alive = true;
};
struct OpvWbTie {                 // the context's end: a member of opv_ctx, so the context's destruction clears the flag
    std::shared_ptr<OpvWbShared> p;
    ~OpvWbTie() { if (p) p->ctx_alive = false; }
};
struct OpvCtxDoor {
    int n_streams = 0, device = 0;
    hipStream_t copy_stream = nullptr;
    std::shared_ptr<OpvWbShared> shared;
};
int opv_int_door(opv_ctx* c, OpvCtxDoor* out);
// hipSetDevice (no host wait: pushes of wideband objects queue behind each other on the copy stream)
int opv_int_push_begin(opv_ctx* c);
// Room for n[i] samples behind what streams[i] holds, for ALL `count` streams or for none: attached / flushed streams are
// OPV_ESTATE, a stream that cannot take its share even after compaction is OPV_ECAPACITY, and in both cases nothing has changed.
// On success dst[i] is where the samples go, and n_avail / dirty are already advanced: the caller must fill the room on the
// copy stream and then call opv_int_push_end.
int opv_int_push_reserve(opv_ctx* c, int count, const int* streams, const uint32_t* n, int** dst);
// wait = true: host wait for the copy stream; false: the event opv_push_iq_batch_async records (opv_process queues behind it)
int opv_int_push_end(opv_ctx* c, bool wait);

#endif
