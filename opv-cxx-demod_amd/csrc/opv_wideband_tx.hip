// opv_wideband_tx.hip — the host half of the wideband transmit bank (include/opv_demod.h, opv_wbtx_*): plan and validation (host
// only; the increment rule and the LO table are the receive bank's, opv_wb_internal.h), the object that carries the last
// ceil((L - 1) / U) input samples of every channel and the count N from push to push, and the push itself: refused on the host
// before anything is enqueued, then one upload of the K input pointers, ONE k_wbtx_duc launch on the context's stream and one wait.
// An object is of one of two kinds: the integer bank (opv_wbtx_create: interp wide samples per input, k_wbtx_duc) or the rational
// one (opv_wbtx_create_rational: down / up wide samples per input, k_wbtxr_duc; its rules are opv_wbtxr_rules.h). They differ in
// how a push's outputs are counted and in the kernel; the object, its carry and its door to the context are shared.
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "opv_ctx.h"
#include "opv_wbtx_internal.h"
#include "opv_wbtxr_rules.h"

static_assert(kWbtxrTile == OPV_WBTXR_THREADS && kWbtxrMaxJ == OPV_WBTXR_MAXJ, "opv_wbtxr_rules.h sizes k_wbtxr_duc's tile and tap rows");

namespace {

int wbtx_plan(const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out) {
    if (!cfg) return fail(OPV_EINVAL, "opv_wbtx: null configuration");
    if (cfg->interp < 1 || cfg->interp > 16) return fail(OPV_EINVAL, "opv_wbtx: interp outside 1..16");
    if (cfg->n_channels < 1 || cfg->n_channels > 256) return fail(OPV_EINVAL, "opv_wbtx: n_channels outside 1..256");
    if (cfg->n_taps < 1 || cfg->n_taps > 1024) return fail(OPV_EINVAL, "opv_wbtx: n_taps outside 1..1024");
    if (cfg->out_shift < 0 || cfg->out_shift > 40) return fail(OPV_EINVAL, "opv_wbtx: out_shift outside 0..40");
    if (!centre_hz || !taps || !inc_out) return fail(OPV_EINVAL, "opv_wbtx: null pointer");
    for (int p = 0; p < cfg->interp && p < cfg->n_taps; ++p) {          // |y| <= 65535 x 32768 < 2^31: what licenses the kernel's int32
        int64_t gain = 0;
        for (int t = p; t < cfg->n_taps; t += cfg->interp) gain += taps[t] < 0 ? -(int64_t)taps[t] : (int64_t)taps[t];
        if (gain > 65535) return fail(OPV_EINVAL, "opv_wbtx: sum of |taps| of one phase exceeds 65535");
    }
    return opv_int_wb_increments(cfg->interp, cfg->n_channels, centre_hz, inc_out);
}

}  // namespace

struct opv_wbtx {
    opv_ctx* ctx = nullptr;
    opv_wbtx_cfg cfg{};
    OpvCtxDoor door{};                   // what outlives the context: door.shared->ctx_alive
    hipStream_t stream = nullptr;        // the context's: the one its transmit bank uses
    uint64_t n_total = 0;                // N: input samples per channel pushed so far
    uint32_t H = 0, J = 0;               // ceil((L - 1) / U) samples carried per channel; floor((L - 1) / U) + 1 taps of the longest phase
    int cur = 0;                         // which carry buffer holds the history
    int* d_hist[2] = {nullptr, nullptr};
    int16_t* d_lo = nullptr;
    int16_t* d_taps = nullptr;
    uint32_t* d_inc = nullptr;
    const int** d_tab = nullptr;         // the push's K input pointers as the kernel reads them ...
    const int** h_tab = nullptr;         // ... and the pinned copy they are uploaded from
    // an object made by opv_wbtx_create_rational (rules: opv_wbtxr_rules.h): cfg above holds K, L, S and first_sample, interp = 0;
    // H = J - 1, and d_taps holds the phase-major table [down][rowlen]
    bool rational = false;
    opv_wbtxr_cfg rcfg{};
    uint32_t rowlen = 0;
};

extern "C" int opv_wbtx_plan(const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out) {
    return wbtx_plan(cfg, centre_hz, taps, inc_out);
}

extern "C" void opv_wbtx_destroy(opv_wbtx* w) {
    if (!w) return;
    (void)hipSetDevice(w->door.device);
    if (w->door.shared && w->door.shared->ctx_alive && w->stream) (void)hipStreamSynchronize(w->stream);   // (a context destroyed first waited for its stream itself)
    if (w->h_tab) (void)hipHostFree(w->h_tab);
    void* ptrs[] = {w->d_hist[0], w->d_hist[1], w->d_lo, w->d_taps, w->d_inc, w->d_tab};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete w;
}

// the object of either kind: `image` is the taps as the kind's kernel reads them (h[L], or the phase-major table), H the input
// samples carried per channel
static int wbtx_make(opv_wbtx** out, opv_ctx* ctx, const char* what, const opv_wbtx_cfg& cfg, const opv_wbtxr_cfg* rcfg, uint32_t H, uint32_t J,
                     const uint32_t* inc, const int16_t* image, size_t image_len) {
    OpvCtxDoor door;
    if (int r = opv_int_door(ctx, &door)) return r;
    opv_wbtx* w = new (std::nothrow) opv_wbtx;
    if (!w) return fail(OPV_ENOMEM, what);
    const uint32_t K = (uint32_t)cfg.n_channels;
    w->ctx = ctx;
    w->cfg = cfg;
    w->door = door;
    w->stream = ctx->stream;
    w->H = H;
    w->J = J;
    if (rcfg) {
        w->rational = true;
        w->rcfg = *rcfg;
        w->rowlen = wbtxr_row_len(*rcfg);
    }
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
    if (int r = wbtx_plan(cfg, centre_hz, taps, inc.data())) return r;
    const uint32_t L = (uint32_t)cfg->n_taps, U = (uint32_t)cfg->interp;
    return wbtx_make(out, ctx, "opv_wbtx_create", *cfg, nullptr, (L - 1 + U - 1) / U, (L - 1) / U + 1, inc.data(), taps, L);
}

// ---- the rational bank: the plan's rules are opv_wbtxr_rules.cpp's
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
    const uint32_t J = wbtxr_taps_per_phase(*cfg);
    std::vector<int16_t> tab((size_t)cfg->down * wbtxr_row_len(*cfg));
    wbtxr_phase_table(*cfg, taps, tab.data());
    const opv_wbtx_cfg as_wbtx{0, cfg->n_channels, cfg->n_taps, cfg->out_shift, cfg->first_sample};   // (interp = 0: no integer push reads it)
    return wbtx_make(out, ctx, "opv_wbtx_create_rational", as_wbtx, cfg, J - 1, J, inc.data(), tab.data(), tab.size());
}

extern "C" uint64_t opv_wbtx_samples(const opv_wbtx* w) { return w ? w->n_total : 0; }

extern "C" int opv_wbtx_reset(opv_wbtx* w, uint64_t first_sample) {
    if (!w) return fail(OPV_EINVAL, "opv_wbtx_reset: null object");
    if (!w->door.shared->ctx_alive) return fail(OPV_ESTATE, "opv_wbtx_reset: the object's context has been destroyed");
    HIPCHK(hipSetDevice(w->door.device));
    HIPCHK(hipMemsetAsync(w->d_hist[w->cur], 0, (size_t)w->cfg.n_channels * (w->H ? w->H : 1) * 4, w->stream));
    HIPCHK(hipStreamSynchronize(w->stream));
    w->n_total = 0;
    w->cfg.first_sample = first_sample;
    return OPV_OK;
}

// opv_wbtx_push of a rational object: the same steps, the count and the first output by opv_wbtxr_rules.h, k_wbtxr_duc
static int wbtxr_push(opv_wbtx* w, const int16_t* const* d_in, size_t n_in, int16_t* d_wide_out) {
    // ---- what can refuse the push, all of it on the host: nothing is enqueued and nothing changes before this is through
    uint64_t n_out = 0;
    const char* why = nullptr;
    if (int r = wbtxr_push_plan(w->rcfg, w->n_total, d_in, n_in, d_wide_out, &n_out, &why)) return fail(r, why);
    if (n_in == 0) return OPV_OK;
    // ---- one upload, one launch, one wait: all on the context's stream
    const uint32_t K = (uint32_t)w->rcfg.n_channels, M = (uint32_t)w->rcfg.down, U = (uint32_t)w->rcfg.up;
    const WbtxrFirst first = wbtxr_first_output(M, U, w->n_total);
    HIPCHK(hipSetDevice(w->door.device));
    for (uint32_t k = 0; k < K; ++k) w->h_tab[k] = (const int*)d_in[k];
    HIPCHK(hipMemcpyAsync(w->d_tab, w->h_tab, (size_t)K * sizeof(int*), hipMemcpyHostToDevice, w->stream));
    OpvWbtxrArgs a{};
    a.in = w->d_tab;
    a.hist_in = w->d_hist[w->cur];
    a.hist_out = w->d_hist[w->cur ^ 1];
    a.lo = w->d_lo;
    a.tab = w->d_taps;
    a.inc = w->d_inc;
    a.out = (int*)d_wide_out;
    a.a0_lo = (uint32_t)(w->cfg.first_sample + first.n0);
    a.n_in = (uint32_t)n_in;
    a.n_out = (uint32_t)n_out;
    a.M = M; a.U = U; a.K = K; a.S = (uint32_t)w->cfg.out_shift;
    a.H = w->H; a.J2 = (w->J + 1) / 2; a.rowlen = w->rowlen;
    a.p0 = first.phase;
    k_wbtxr_duc<<<(a.n_out + OPV_WBTXR_THREADS - 1) / OPV_WBTXR_THREADS, OPV_WBTXR_THREADS, 0, w->stream>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(w->stream));                               // (the inputs and the output are the caller's again)
    w->cur ^= 1;
    w->n_total += n_in;
    return OPV_OK;
}

extern "C" int opv_wbtx_push(opv_wbtx* w, const int16_t* const* d_in, size_t n_in, int16_t* d_wide_out) {
    if (!w) return fail(OPV_EINVAL, "opv_wbtx_push: null object");
    if (!w->door.shared->ctx_alive) return fail(OPV_ESTATE, "opv_wbtx_push: the object's context has been destroyed");
    if (w->rational) return wbtxr_push(w, d_in, n_in, d_wide_out);
    // ---- what can refuse the push, all of it on the host: nothing is enqueued and nothing changes before this is through
    if (!d_in || !d_wide_out) return fail(OPV_EINVAL, "opv_wbtx_push: null pointer");
    const uint64_t K = (uint64_t)w->cfg.n_channels, U = (uint64_t)w->cfg.interp;
    if ((uint64_t)n_in >= (1ull << 31) || (uint64_t)n_in * U >= (1ull << 31)) return fail(OPV_EINVAL, "opv_wbtx_push: 2^31 or more wide samples in one push");
    if (n_in == 0) return OPV_OK;
    const uintptr_t out_lo = (uintptr_t)d_wide_out, out_hi = out_lo + (uintptr_t)(n_in * U * 4);
    if (out_lo & 3u) return fail(OPV_EINVAL, "opv_wbtx_push: output pointer must be 4-byte aligned");
    for (uint64_t k = 0; k < K; ++k) {
        const uintptr_t lo = (uintptr_t)d_in[k], hi = lo + (uintptr_t)(n_in * 4);
        if (!lo) continue;
        if (lo & 3u) return fail(OPV_EINVAL, "opv_wbtx_push: input pointer must be 4-byte aligned");
        if (lo < out_hi && out_lo < hi) return fail(OPV_EINVAL, "opv_wbtx_push: the output overlaps an input");
    }
    // ---- one upload, one launch, one wait: all on the context's stream
    HIPCHK(hipSetDevice(w->door.device));
    for (uint64_t k = 0; k < K; ++k) w->h_tab[k] = (const int*)d_in[k];
    HIPCHK(hipMemcpyAsync(w->d_tab, w->h_tab, (size_t)K * sizeof(int*), hipMemcpyHostToDevice, w->stream));
    OpvWbtxArgs a{};
    a.in = w->d_tab;
    a.hist_in = w->d_hist[w->cur];
    a.hist_out = w->d_hist[w->cur ^ 1];
    a.lo = w->d_lo;
    a.taps = w->d_taps;
    a.inc = w->d_inc;
    a.out = (int*)d_wide_out;
    a.a0_lo = (uint32_t)(w->cfg.first_sample + w->n_total * U);
    a.n_in = (uint32_t)n_in;
    a.n_out = (uint32_t)(n_in * U);
    a.U = (uint32_t)U; a.L = (uint32_t)w->cfg.n_taps; a.K = (uint32_t)K; a.S = (uint32_t)w->cfg.out_shift;
    a.H = w->H; a.J = w->J;
    k_wbtx_duc<<<(a.n_out + OPV_WBTX_THREADS - 1) / OPV_WBTX_THREADS, OPV_WBTX_THREADS, 0, w->stream>>>(a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(w->stream));                               // (the inputs and the output are the caller's again)
    w->cur ^= 1;
    w->n_total += n_in;
    return OPV_OK;
}
