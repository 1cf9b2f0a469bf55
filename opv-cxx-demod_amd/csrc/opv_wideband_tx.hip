// opv_wideband_tx.hip — the host half of the wideband transmit bank (include/opv_demod.h, opv_wbtx_*): the object that carries the
// last H input samples of every channel and the count N from push to push, and the push itself: refused on the host before
// anything is enqueued, then one upload of the K input pointers, ONE launch on the context's stream and one wait. An object is of
// one of two kinds: the integer bank (opv_wbtx_create: interp wide samples per input, k_wbtx_duc) or the rational one
// (opv_wbtx_create_rational: down / up wide samples per input, k_wbtxr_duc). They differ in how a push's outputs are counted and in
// the kernel; the object, its carry and its door to the context are shared. Plans, refusals and every other rule that needs no
// device are opv_wb_rules.h's.
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "opv_ctx.h"
#include "opv_wb_rules.h"
#include "opv_wbtx_internal.h"

static_assert(kWbtxrTile == OPV_WBTXR_THREADS && kWbtxrMaxJ == OPV_WBTXR_MAXJ, "opv_wb_rules.h sizes k_wbtxr_duc's tile and tap rows");

struct opv_wbtx {
    opv_ctx* ctx = nullptr;
    WbtxShape shape{};                   // the kind, its ratio (Integer: interp / 1) and K
    uint32_t L = 0, S = 0;               // n_taps, out_shift
    uint64_t first_sample = 0;
    OpvCtxDoor door{};                   // what outlives the context: door.shared->ctx_alive
    hipStream_t stream = nullptr;        // the context's: the one its transmit bank uses
    uint64_t n_total = 0;                // N: input samples per channel pushed so far
    uint32_t H = 0, J = 0;               // input samples carried per channel; taps of the longest phase. Integer: ceil((L - 1) / U), floor((L - 1) / U) + 1; Rational: J - 1, ceil(L / M)
    uint32_t rowlen = 0;                 // Rational: the row length of the phase-major table
    int cur = 0;                         // which carry buffer holds the history
    int* d_hist[2] = {nullptr, nullptr};
    int16_t* d_lo = nullptr;
    int16_t* d_taps = nullptr;           // Integer: h[L]; Rational: the phase-major table [down][rowlen]
    uint32_t* d_inc = nullptr;
    const int** d_tab = nullptr;         // the push's K input pointers as the kernel reads them ...
    const int** h_tab = nullptr;         // ... and the pinned copy they are uploaded from
    WbSchedule sched;                    // the LO schedule of every channel (opv_wbtx_retune); plain until the first retune
    OpvWbDevSched* d_sched = nullptr;    // a retuned object: the push's K schedule tables as the kernel reads them ...
    OpvWbDevSched* h_sched = nullptr;    // ... and the pinned copy they are uploaded from (a push waits for its launch: one slot)
};

extern "C" int opv_wbtx_plan(const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out) {
    const char* why = nullptr;
    if (int r = wbtx_plan(cfg, centre_hz, taps, inc_out, &why)) return fail(r, why);
    return OPV_OK;
}

extern "C" void opv_wbtx_destroy(opv_wbtx* w) {
    if (!w) return;
    (void)hipSetDevice(w->door.device);
    if (w->door.shared && w->door.shared->ctx_alive && w->stream) (void)hipStreamSynchronize(w->stream);   // (a context destroyed first waited for its stream itself)
    if (w->h_tab) (void)hipHostFree(w->h_tab);
    if (w->h_sched) (void)hipHostFree(w->h_sched);
    void* ptrs[] = {w->d_hist[0], w->d_hist[1], w->d_lo, w->d_taps, w->d_inc, w->d_tab, w->d_sched};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete w;
}

// the object of either kind: `plan` is an object with the kind's own fields set by its creator (shape, L, S, first_sample, H, J,
// rowlen) and nothing else, `image` the taps as the kind's kernel reads them (h[L], or the phase-major table)
static int wbtx_make(opv_wbtx** out, opv_ctx* ctx, const char* what, const opv_wbtx& plan, const uint32_t* inc, const int16_t* image, size_t image_len) {
    OpvCtxDoor door;
    if (int r = opv_int_door(ctx, &door)) return r;
    opv_wbtx* w = new (std::nothrow) opv_wbtx(plan);
    if (!w) return fail(OPV_ENOMEM, what);
    const uint32_t K = w->shape.K;
    w->ctx = ctx;
    w->door = door;
    w->stream = ctx->stream;
    wb_sched_reset(w->sched, (int32_t)w->shape.down, (int32_t)w->shape.up, K, inc);
    int16_t lo[4096];
    opv_wb_lo_table(lo);
    auto undo = [&](hipError_t e, const char* where) { opv_wbtx_destroy(w); return fail(OPV_EHIP, where, e); };
    HIPCHK_OR(undo, hipSetDevice(door.device));
    const size_t hist_bytes = (size_t)K * (w->H ? w->H : 1) * 4;
    for (int i = 0; i < 2; ++i) {
        HIPCHK_OR(undo, hipMalloc(&w->d_hist[i], hist_bytes));
        HIPCHK_OR(undo, hipMemset(w->d_hist[i], 0, hist_bytes));                  // x[m] = 0 for m < 0: an empty history is a history of zeros
    }
    HIPCHK_OR(undo, hipMalloc(&w->d_lo, sizeof lo));
    HIPCHK_OR(undo, hipMalloc(&w->d_taps, image_len * 2));
    HIPCHK_OR(undo, hipMalloc(&w->d_inc, (size_t)K * 4));
    HIPCHK_OR(undo, hipMalloc(&w->d_tab, (size_t)K * sizeof(int*)));
    HIPCHK_OR(undo, hipHostMalloc((void**)&w->h_tab, (size_t)K * sizeof(int*), hipHostMallocDefault));
    HIPCHK_OR(undo, hipMalloc(&w->d_sched, (size_t)K * sizeof(OpvWbDevSched)));
    HIPCHK_OR(undo, hipHostMalloc((void**)&w->h_sched, (size_t)K * sizeof(OpvWbDevSched), hipHostMallocDefault));
    HIPCHK_OR(undo, hipMemcpy(w->d_lo, lo, sizeof lo, hipMemcpyHostToDevice));
    HIPCHK_OR(undo, hipMemcpy(w->d_taps, image, image_len * 2, hipMemcpyHostToDevice));
    HIPCHK_OR(undo, hipMemcpy(w->d_inc, inc, (size_t)K * 4, hipMemcpyHostToDevice));
    *out = w;
    return OPV_OK;
}

extern "C" int opv_wbtx_create(opv_wbtx** out, opv_ctx* ctx, const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps) {
    if (!out) return fail(OPV_EINVAL, "opv_wbtx_create: null out");
    *out = nullptr;
    if (!ctx) return fail(OPV_EINVAL, "opv_wbtx_create: null context");
    std::vector<uint32_t> inc(256);
    if (int r = opv_wbtx_plan(cfg, centre_hz, taps, inc.data())) return r;
    const uint32_t L = (uint32_t)cfg->n_taps, U = (uint32_t)cfg->interp;
    opv_wbtx plan;
    plan.shape = {WbtxKind::Integer, U, 1, (uint32_t)cfg->n_channels};
    plan.L = L;
    plan.S = (uint32_t)cfg->out_shift;
    plan.first_sample = cfg->first_sample;
    plan.H = (L - 1 + U - 1) / U;
    plan.J = (L - 1) / U + 1;
    return wbtx_make(out, ctx, "opv_wbtx_create", plan, inc.data(), taps, L);
}

// ---- the rational bank
extern "C" int opv_wbtxr_plan(const opv_wbtxr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out) {
    const char* why = nullptr;
    if (int r = wbtxr_plan(cfg, centre_hz, taps, inc_out, &why)) return fail(r, why);
    return OPV_OK;
}

extern "C" uint64_t opv_wbtxr_outputs(const opv_wbtxr_cfg* cfg, uint64_t n_in_total) {
    if (wbtxr_cfg_refusal(cfg) || n_in_total > kWbtxrMaxInputs) return 0;
    return wbtxr_outputs((uint32_t)cfg->down, (uint32_t)cfg->up, n_in_total);
}

extern "C" int opv_wbtx_create_rational(opv_wbtx** out, opv_ctx* ctx, const opv_wbtxr_cfg* cfg, const double* centre_hz, const int16_t* taps) {
    if (!out) return fail(OPV_EINVAL, "opv_wbtx_create_rational: null out");
    *out = nullptr;
    if (!ctx) return fail(OPV_EINVAL, "opv_wbtx_create_rational: null context");
    std::vector<uint32_t> inc(256);
    if (int r = opv_wbtxr_plan(cfg, centre_hz, taps, inc.data())) return r;
    const uint32_t J = wb_taps_per_phase(cfg->n_taps, cfg->down), rowlen = wb_row_len(J);
    std::vector<int16_t> tab((size_t)cfg->down * rowlen);                  // at most 8192 x 64 x 2 B = 1 MB
    wb_phase_table(taps, cfg->n_taps, (uint32_t)cfg->down, J, rowlen, tab.data());
    opv_wbtx plan;
    plan.shape = {WbtxKind::Rational, (uint32_t)cfg->down, (uint32_t)cfg->up, (uint32_t)cfg->n_channels};
    plan.L = (uint32_t)cfg->n_taps;
    plan.S = (uint32_t)cfg->out_shift;
    plan.first_sample = cfg->first_sample;
    plan.H = J - 1;
    plan.J = J;
    plan.rowlen = rowlen;
    return wbtx_make(out, ctx, "opv_wbtx_create_rational", plan, inc.data(), tab.data(), tab.size());
}

extern "C" uint64_t opv_wbtx_samples(const opv_wbtx* w) { return w ? w->n_total : 0; }

extern "C" int opv_wbtx_reset(opv_wbtx* w, uint64_t first_sample) {
    if (!w) return fail(OPV_EINVAL, "opv_wbtx_reset: null object");
    if (!w->door.shared->ctx_alive) return fail(OPV_ESTATE, "opv_wbtx_reset: the object's context has been destroyed");
    HIPCHK(hipSetDevice(w->door.device));
    HIPCHK(hipMemsetAsync(w->d_hist[w->cur], 0, (size_t)w->shape.K * (w->H ? w->H : 1) * 4, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    w->n_total = 0;
    w->first_sample = first_sample;
    const std::vector<uint32_t> inc = w->sched.inc;
    wb_sched_reset(w->sched, w->sched.down, w->sched.up, w->shape.K, inc.data());   // every channel back to its creation schedule
    return OPV_OK;
}

extern "C" int opv_wbtx_push(opv_wbtx* w, const int16_t* const* d_in, size_t n_in, int16_t* d_wide_out) {
    if (!w) return fail(OPV_EINVAL, "opv_wbtx_push: null object");
    if (!w->door.shared->ctx_alive) return fail(OPV_ESTATE, "opv_wbtx_push: the object's context has been destroyed");
    // ---- what can refuse the push, all of it on the host: nothing is enqueued and nothing changes before this is through
    uint64_t n_out = 0;
    const char* why = nullptr;
    if (int r = wbtx_push_plan(w->shape, w->n_total, d_in, n_in, d_wide_out, &n_out, &why)) return fail(r, why);
    if (n_in == 0) return OPV_OK;
    // ---- one upload, one launch, one wait: all on the context's stream
    const uint32_t K = w->shape.K, M = w->shape.down, U = w->shape.up;
    HIPCHK(hipSetDevice(w->door.device));
    for (uint32_t k = 0; k < K; ++k) w->h_tab[k] = (const int*)d_in[k];
    HIPCHK(hipMemcpyAsync(w->d_tab, w->h_tab, (size_t)K * sizeof(int*), hipMemcpyHostToDevice, w->stream));
    OpvWbtxHead h{};
    h.in = w->d_tab;
    h.hist_in = w->d_hist[w->cur];
    h.hist_out = w->d_hist[w->cur ^ 1];
    h.lo = w->d_lo;
    h.taps = w->d_taps;
    h.inc = w->d_inc;
    h.out = (int*)d_wide_out;
    h.n_in = (uint32_t)n_in;
    h.n_out = (uint32_t)n_out;
    h.K = K; h.S = w->S; h.H = w->H;
    // ---- the LO: an object never retuned launches the unscheduled kernel; any other one the tables of this push, whose origin
    // is the push's first wide sample
    const bool rational = w->shape.kind == WbtxKind::Rational;
    const uint64_t wide0 = rational ? wbtxr_first_output(M, U, w->n_total).n0 : w->n_total * M;
    const bool tuned = !wb_sched_plain(w->sched);
    if (tuned) {
        wb_sched_table(w->sched, w->first_sample + wide0, n_out, w->h_sched);
        HIPCHK(hipMemcpyAsync(w->d_sched, w->h_sched, (size_t)K * sizeof(OpvWbDevSched), hipMemcpyHostToDevice, w->stream));
    }
    if (rational) {
        const WbtxrFirst first = wbtxr_first_output(M, U, w->n_total);
        h.a0_lo = (uint32_t)(w->first_sample + first.n0);
        OpvWbtxrArgs a{h};
        a.M = M; a.U = U; a.J2 = (w->J + 1) / 2; a.rowlen = w->rowlen;
        a.p0 = first.phase;
        const uint32_t grid = (h.n_out + OPV_WBTXR_THREADS - 1) / OPV_WBTXR_THREADS;
        if (tuned) k_wbtxr_duc_tuned<<<grid, OPV_WBTXR_THREADS, 0, w->stream>>>(a, w->d_sched);
        else k_wbtxr_duc<<<grid, OPV_WBTXR_THREADS, 0, w->stream>>>(a);
    } else {
        const uint32_t interp = M;                                        // (the integer bank's ratio is interp / 1)
        h.a0_lo = (uint32_t)(w->first_sample + w->n_total * interp);      // the first wide sample is N interp
        OpvWbtxArgs a{h};
        a.U = interp; a.L = w->L; a.J = w->J;
        const uint32_t grid = (h.n_out + OPV_WBTX_THREADS - 1) / OPV_WBTX_THREADS;
        if (tuned) k_wbtx_duc_tuned<<<grid, OPV_WBTX_THREADS, 0, w->stream>>>(a, w->d_sched);
        else k_wbtx_duc<<<grid, OPV_WBTX_THREADS, 0, w->stream>>>(a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(w->stream));                               // (the inputs and the output are the caller's again)
    w->cur ^= 1;
    w->n_total += n_in;
    wb_sched_prune(w->sched, w->first_sample + wide0 + n_out);            // what no later push can write any more
    return OPV_OK;
}

// ---- the LO schedule (include/opv_demod.h, "per-channel retune and Doppler ramps"); the rules are opv_wb_rules.h's
extern "C" int opv_wbtx_retune(opv_wbtx* w, int count, const opv_wb_tune* tunes) {
    if (!w) return fail(OPV_EINVAL, "opv_wbtx_retune: null object");
    if (!w->door.shared->ctx_alive) return fail(OPV_ESTATE, "opv_wbtx_retune: the object's context has been destroyed");
    const uint64_t wide = w->shape.kind == WbtxKind::Rational ? wbtxr_outputs(w->shape.down, w->shape.up, w->n_total) : w->n_total * w->shape.down;
    const char* why = nullptr;
    if (int r = wb_sched_retune(w->sched, w->first_sample + wide, w->first_sample + wide, count, tunes, &why)) return fail(r, why);
    return OPV_OK;
}

extern "C" int opv_wbtx_segments(opv_wbtx* w, int channel, opv_wb_seg* out, size_t cap) {
    if (!w) return fail(OPV_EINVAL, "opv_wbtx_segments: null object");
    const int n = wb_sched_copy(w->sched, channel, out, cap);
    return n < 0 ? fail(OPV_EINVAL, "opv_wbtx_segments: channel out of range") : n;
}
