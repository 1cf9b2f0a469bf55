// opv_scan.hip — the host half of the wideband scan (include/opv_demod.h, opv_scan_*): the object that carries N and the samples
// from the start of the first unfinished block from push to push (the doors' double-buffered carry, only longer), the ring of
// completed rows, and the push itself: what it completes and carries is computed here (opv_scan_rules.h) and refused before
// anything is launched if the ring has no room; then ONE k_scan_probe launch and one k_scan_reduce on the context's copy stream
// serve all P probes. A push always computes whole blocks, so no partial row lives between pushes. The object reaches its context
// through opv_wb_internal.h's door like a wideband object and owns no stream of it.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <new>
#include <vector>

#include "../../include/opv_demod.h"
#include "opv_iq_format.h"
#include "opv_scan_internal.h"
#include "opv_scan_rules.h"
#include "opv_wb_internal.h"

static_assert(kScanLanes == OPV_SCAN_THREADS && kScanMaxWindow == OPV_SCAN_WINDOW, "opv_scan_rules.h shapes k_scan_probe's launch for these sizes");

struct opv_scan {
    opv_ctx* ctx = nullptr;
    opv_scan_cfg cfg{};
    OpvCtxDoor door{};
    uint64_t n_total = 0;                // N: wide samples pushed so far
    uint32_t hist_len = 0;               // samples the carry holds: those in front of sample N from the first unfinished block's start on
    int cur = 0;                         // which carry buffer holds them
    int* d_hist[2] = {nullptr, nullptr};
    int16_t* d_lo = nullptr;
    int16_t* d_window = nullptr;
    uint32_t* d_inc = nullptr;
    uint64_t* d_rows = nullptr;          // the ring: block b's row is row b % ring_blocks
    uint64_t blocks_done = 0, blocks_popped = 0;
    uint64_t* d_part = nullptr;          // the sums of a push's workgroups, before k_scan_reduce (grow-only)
    size_t part_cap = 0;
    OpvStage stage;                      // pageable sources: the block is copied here first (grow-only)
};

extern "C" int opv_scan_plan(const opv_scan_cfg* cfg, const double* probe_hz, const int16_t* window, uint32_t* inc_out) {
    const char* why = nullptr;
    if (int r = scan_plan(cfg, probe_hz, window, inc_out, &why)) return opv_int_fail(r, why);
    return OPV_OK;
}

extern "C" uint64_t opv_scan_blocks(const opv_scan_cfg* cfg, uint64_t n_wide_total) {
    return scan_cfg_refusal(cfg) ? 0 : scan_blocks(cfg, n_wide_total);
}

extern "C" long opv_scan_carriers(const uint64_t* row, int n_probes, double f0_hz, double step_hz, double half_width_hz, uint32_t ratio_q8,
                                  opv_scan_carrier* out, size_t cap) {
    const char* why = nullptr;
    const long n = scan_carriers(row, n_probes, f0_hz, step_hz, half_width_hz, ratio_q8, out, cap, &why);
    return n < 0 ? opv_int_fail((int)n, why) : n;
}

extern "C" void opv_scan_destroy(opv_scan* w) {
    if (!w) return;
    (void)hipSetDevice(w->door.device);
    if (w->door.shared && w->door.shared->ctx_alive && w->door.copy_stream) (void)hipStreamSynchronize(w->door.copy_stream);   // (a context destroyed first waited itself)
    void* ptrs[] = {w->d_hist[0], w->d_hist[1], w->d_lo, w->d_window, w->d_inc, w->d_rows, w->d_part, w->stage.d};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete w;
}

extern "C" int opv_scan_create(opv_scan** out, opv_ctx* ctx, const opv_scan_cfg* cfg, const double* probe_hz, const int16_t* window) {
    if (!out) return opv_int_fail(OPV_EINVAL, "opv_scan_create: null out");
    *out = nullptr;
    if (!ctx) return opv_int_fail(OPV_EINVAL, "opv_scan_create: null pointer");
    std::vector<uint32_t> inc(kScanMaxProbes);
    if (int r = opv_scan_plan(cfg, probe_hz, window, inc.data())) return r;
    OpvCtxDoor door;
    if (int r = opv_int_door(ctx, &door)) return r;
    opv_scan* w = new (std::nothrow) opv_scan;
    if (!w) return opv_int_fail(OPV_ENOMEM, "opv_scan_create");
    w->ctx = ctx;
    w->cfg = *cfg;
    w->door = door;
    int16_t lo[4096];
    opv_wb_lo_table(lo);
    const size_t P = (size_t)cfg->n_probes, Lw = (size_t)cfg->n_window;
    const size_t hist_bytes = (size_t)scan_span(cfg) * 4;                // (a carry is shorter than the span)
    auto undo = [&](hipError_t e, const char* what) { opv_scan_destroy(w); return opv_int_fail(OPV_EHIP, what, e); };
    HIPCHK_OR(undo, hipSetDevice(door.device));
    HIPCHK_OR(undo, hipMalloc(&w->d_hist[0], hist_bytes));
    HIPCHK_OR(undo, hipMalloc(&w->d_hist[1], hist_bytes));
    HIPCHK_OR(undo, hipMalloc(&w->d_lo, sizeof lo));
    HIPCHK_OR(undo, hipMalloc(&w->d_window, Lw * 2));
    HIPCHK_OR(undo, hipMalloc(&w->d_inc, P * 4));
    HIPCHK_OR(undo, hipMalloc(&w->d_rows, (size_t)cfg->ring_blocks * P * 8));
    HIPCHK_OR(undo, hipMemcpy(w->d_lo, lo, sizeof lo, hipMemcpyHostToDevice));
    HIPCHK_OR(undo, hipMemcpy(w->d_window, window, Lw * 2, hipMemcpyHostToDevice));
    HIPCHK_OR(undo, hipMemcpy(w->d_inc, inc.data(), P * 4, hipMemcpyHostToDevice));
    *out = w;
    return OPV_OK;
}

namespace {

using Src = OpvSrc;

// fmt != OPV_IQ_CS16 (a host block in another format): converted into the object's stage on the copy stream, then as a device push
int scan_push(opv_scan* w, const void* iq, size_t n_new, Src kind, int fmt = OPV_IQ_CS16) {
    if (!w) return opv_int_fail(OPV_EINVAL, "opv_scan_push: null object");
    if (!w->door.shared->ctx_alive) return opv_int_fail(OPV_ESTATE, "opv_scan_push: the object's context has been destroyed");
    if (int r = opv_int_push_begin(w->ctx)) return r;
    if (n_new == 0) return OPV_OK;
    if (!iq) return opv_int_fail(OPV_EINVAL, "opv_scan_push: null IQ pointer");
    const bool typed = fmt != OPV_IQ_CS16;
    if (typed && ((uintptr_t)iq & (opv_iq_align_of(fmt) - 1)) != 0)
        return opv_int_fail(OPV_EINVAL, "opv_scan_push_fmt: the block is not aligned for its format (2 bytes for cs8 / cu8, 4 for cf32)");
    if (!typed && ((uintptr_t)iq & 3u) != 0) return opv_int_fail(OPV_EINVAL, "opv_scan_push: IQ pointer must be 4-byte aligned");
    if (n_new >= (1ull << 31)) return opv_int_fail(OPV_EINVAL, "opv_scan_push: more than 2^31 - 1 samples in one push");
    if (w->n_total + n_new > (1ull << 63)) return opv_int_fail(OPV_ECAPACITY, "opv_scan_push: more than 2^63 samples");
    // ---- what can refuse the push, before anything is launched or changed: the rows it completes against the ring's free ones
    const opv_scan_cfg& cfg = w->cfg;
    const ScanPush plan = scan_push_plan(&cfg, w->n_total, n_new);
    const uint64_t blocks = plan.b1 - plan.b0;
    if (blocks > (uint64_t)cfg.ring_blocks - (w->blocks_done - w->blocks_popped))
        return opv_int_fail(OPV_ECAPACITY, "opv_scan_push: the ring has no room for the blocks this push completes (opv_scan_pop frees rows)");
    const ScanShape shape = scan_shape(&cfg, blocks);
    const uint32_t P = (uint32_t)cfg.n_probes;
    // ---- the source as the device sees it, and the scratch rows (both grow-only: nothing of the object's state changes)
    const int* src = nullptr;
    bool stage = false;
    OpvTypedSrc tsrc;
    if (typed) {
        if (int r = opv_int_source_fmt(iq, n_new, opv_iq_bytes_of(fmt), w->door.device, w->door.copy_stream, &w->stage, &tsrc)) return r;
        src = w->stage.d;
    } else if (int r = opv_int_source((const int16_t*)iq, n_new, kind, w->door.device, w->door.copy_stream, &w->stage, &src, &stage)) {
        return r;
    }
    const size_t part_rows = (size_t)(blocks * shape.runs);
    if (w->part_cap < part_rows) {
        HIPCHK(hipStreamSynchronize(w->door.copy_stream));
        if (w->d_part) HIPCHK(hipFree(w->d_part));
        w->d_part = nullptr;
        w->part_cap = 0;
        HIPCHK(hipMalloc(&w->d_part, part_rows * P * 8));
        w->part_cap = part_rows;
    }
    if (stage) HIPCHK(hipMemcpyAsync(w->stage.d, iq, n_new * 4, hipMemcpyHostToDevice, w->door.copy_stream));
    if (typed)
        if (int r = opv_int_convert_enqueue(iq, n_new, fmt, tsrc, &w->stage, w->door.copy_stream)) return r;
    // ---- the launches. A push that completes nothing still moves the carry: enough workgroups for that alone
    OpvScanArgs a{};
    a.src = src;
    a.hist_in = w->d_hist[w->cur];
    a.hist_out = w->d_hist[w->cur ^ 1];
    a.lo = w->d_lo;
    a.window = w->d_window;
    a.inc = w->d_inc;
    a.part = w->d_part;
    a.base0 = (int64_t)(plan.start - w->n_total);                       // (two's complement: negative when the block starts inside the carry)
    a.a0_lo = (uint32_t)(cfg.first_sample + w->n_total);
    a.n_new = (uint32_t)n_new; a.hist_len = w->hist_len; a.keep = plan.keep;
    a.P = P; a.Lw = (uint32_t)cfg.n_window; a.H = (uint32_t)cfg.hop; a.A = (uint32_t)cfg.n_avg; a.S = (uint32_t)cfg.out_shift;
    a.blocks = (uint32_t)blocks; a.runs = shape.runs; a.run_len = shape.run_len;
    uint32_t gx = (uint32_t)part_rows, gy = shape.pgroups;
    if (!blocks) {
        gx = (plan.keep + 4 * OPV_SCAN_THREADS - 1) / (4 * OPV_SCAN_THREADS);
        gx = gx < 1 ? 1 : gx > 1024 ? 1024 : gx;
        gy = 1;
    }
    k_scan_probe<<<dim3(gx, gy), OPV_SCAN_THREADS, 0, w->door.copy_stream>>>(a);
    HIPCHK(hipGetLastError());
    if (blocks) {
        OpvScanReduceArgs r{};
        r.part = w->d_part; r.rows = w->d_rows;
        r.head = (uint32_t)(w->blocks_done % (uint64_t)cfg.ring_blocks); r.ring = (uint32_t)cfg.ring_blocks;
        r.blocks = (uint32_t)blocks; r.runs = shape.runs; r.P = P;
        k_scan_reduce<<<(uint32_t)((blocks * P + 255) / 256), 256, 0, w->door.copy_stream>>>(r);
        HIPCHK(hipGetLastError());
    }
    // ---- N, the carry and the ring move together, once everything is enqueued
    w->cur ^= 1;
    w->n_total += n_new;
    w->hist_len = plan.keep;
    w->blocks_done += blocks;
    HIPCHK(hipStreamSynchronize(w->door.copy_stream));                  // the caller's block has been read
    return OPV_OK;
}

int scan_live(opv_scan* w, const char* null_text, const char* dead_text) {
    if (!w) return opv_int_fail(OPV_EINVAL, null_text);
    if (!w->door.shared->ctx_alive) return opv_int_fail(OPV_ESTATE, dead_text);
    return opv_int_push_begin(w->ctx);
}

}  // namespace

extern "C" int opv_scan_push(opv_scan* w, const int16_t* iq_wide, size_t n_wide) { return scan_push(w, iq_wide, n_wide, Src::Host); }
extern "C" int opv_scan_push_device(opv_scan* w, const int16_t* d_iq_wide, size_t n_wide) { return scan_push(w, d_iq_wide, n_wide, Src::Device); }
extern "C" int opv_scan_push_fmt(opv_scan* w, int fmt, const void* wide, size_t n_wide) {
    if (!opv_iq_align_of(fmt)) return opv_int_fail(OPV_EINVAL, "opv_scan_push_fmt: unknown sample format");
    return scan_push(w, wide, n_wide, Src::Host, fmt);
}

extern "C" long opv_scan_pop(opv_scan* w, uint64_t* rows, size_t cap_blocks, uint64_t* first_block) {
    if (int r = scan_live(w, "opv_scan_pop: null object", "opv_scan_pop: the object's context has been destroyed")) return r;
    if (!rows && cap_blocks) return opv_int_fail(OPV_EINVAL, "opv_scan_pop: null rows");
    HIPCHK(hipStreamSynchronize(w->door.copy_stream));
    const uint64_t ring = (uint64_t)w->cfg.ring_blocks, P = (uint64_t)w->cfg.n_probes;
    uint64_t n = w->blocks_done - w->blocks_popped;
    if (n > cap_blocks) n = cap_blocks;
    if (first_block) *first_block = w->blocks_popped;
    for (uint64_t done = 0; done < n;) {                                // at most two runs: the ring wraps once
        const uint64_t at = (w->blocks_popped + done) % ring;
        const uint64_t run = n - done < ring - at ? n - done : ring - at;
        HIPCHK(hipMemcpy(rows + done * P, w->d_rows + at * P, (size_t)(run * P * 8), hipMemcpyDeviceToHost));
        done += run;
    }
    w->blocks_popped += n;
    return (long)n;
}

extern "C" int opv_scan_reset(opv_scan* w, uint64_t first_sample) {
    if (int r = scan_live(w, "opv_scan_reset: null object", "opv_scan_reset: the object's context has been destroyed")) return r;
    HIPCHK(hipStreamSynchronize(w->door.copy_stream));
    w->cfg.first_sample = first_sample;
    w->n_total = 0;
    w->hist_len = 0;
    w->blocks_done = w->blocks_popped = 0;
    return OPV_OK;
}
