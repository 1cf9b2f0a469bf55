// opv_tx_bank.hip — the host half of the transmit bank (include/opv_demod.h, opv_txb_*): the object (per stream the two numbers
// that are a modulator, the sign parity also in device memory where the round's scan carries it), its life beside its
// context's, and the round: refused or planned by txb_plan_round (opv_txb_rules.cpp) before anything is enqueued, then one
// upload, the four launches of k_tx_bank.hip on the context's stream, one wait, and the host's patch of ambiguous samples.
#include <cstring>
#include <memory>
#include <new>
#include <vector>

#include "opv_ctx.h"
#include "opv_tx_internal.h"
#include "opv_txb_rules.h"

namespace {
constexpr uint32_t kAmbCap = 4096;
constexpr size_t kStateHead = 16;        // the device state: [ambiguous-sample counter, 16 bytes][sign parity, a byte per stream]
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

struct opv_txb {
    opv_ctx* ctx = nullptr;
    OpvCtxDoor door{};                   // what outlives the context: door.shared->ctx_alive
    hipStream_t stream = nullptr;        // the context's
    std::vector<opv_txb_state> st;       // the modulators; sign_parity mirrors the device's byte (every round brings it back)
    uint8_t* d_state = nullptr;
    OpvTxbAmb* d_amb = nullptr;
    GrowBuf<uint8_t> scratch;            // the largest round so far: entries, frames, code bytes, frame parities, symbol-start phases
    std::vector<uint8_t> h_up, h_state;  // staging of the round's upload and of the state that comes back
};

static int txb_live(opv_txb* b, const char* who) {
    if (!b) return fail(OPV_EINVAL, "opv_txb: null bank");
    if (!b->door.shared->ctx_alive) return fail(OPV_ESTATE, who);
    HIPCHK(hipSetDevice(b->door.device));
    return OPV_OK;
}

extern "C" int opv_txb_plan_round(int n_streams, const opv_txb_state* states, int count, const int* streams,
                                  const size_t* n_frames, const uintptr_t* out_addr, uint32_t* first_block, uint64_t* first_symbol) {
    const char* why = nullptr;
    if (int r = txb_plan_round(n_streams, states, count, streams, n_frames, out_addr, first_block, first_symbol, &why)) return fail(r, why);
    return OPV_OK;
}

extern "C" int opv_tap_txb_patch(uint64_t symbol, int sample, int code, int16_t out_iq[2]) {
    if (!out_iq || sample < 0 || sample >= OPV_SPS || code < -2 || code > 2 || symbol >= kTxbMaxRunSymbols)
        return fail(OPV_EINVAL, "opv_tap_txb_patch: bad arguments");
    txb_patch_sample(symbol, sample, code, out_iq);
    return OPV_OK;
}

extern "C" void opv_txb_destroy(opv_txb* b) {
    if (!b) return;
    (void)hipSetDevice(b->door.device);
    if (b->door.shared && b->door.shared->ctx_alive && b->stream) (void)hipStreamSynchronize(b->stream);   // (a context destroyed first waited for its stream itself)
    if (b->d_state) (void)hipFree(b->d_state);
    if (b->d_amb) (void)hipFree(b->d_amb);
    delete b;                            // (scratch: GrowBuf's destructor, on the device made current above)
}

extern "C" int opv_txb_create(opv_txb** out, opv_ctx* ctx, int n_streams) {
    if (!out) return fail(OPV_EINVAL, "opv_txb_create: null out");
    *out = nullptr;
    if (!ctx) return fail(OPV_EINVAL, "opv_txb_create: null context");
    if (n_streams < 1 || n_streams > OPV_TXB_MAX_STREAMS) return fail(OPV_EINVAL, "opv_txb_create: n_streams outside 1..OPV_TXB_MAX_STREAMS");
    OpvCtxDoor door;
    if (int r = opv_int_door(ctx, &door)) return r;
    opv_txb* b = new (std::nothrow) opv_txb;
    if (!b) return fail(OPV_ENOMEM, "opv_txb_create");
    b->ctx = ctx;
    b->door = door;
    b->stream = ctx->stream;
    b->st.assign((size_t)n_streams, opv_txb_state{0, 0, 0});
    b->h_state.resize(kStateHead + (size_t)n_streams);
    auto undo = [&](hipError_t e, const char* what) { opv_txb_destroy(b); return fail(OPV_EHIP, what, e); };
    HIPCHK_OR(undo, hipSetDevice(door.device));
    HIPCHK_OR(undo, hipMalloc(&b->d_state, kStateHead + (size_t)n_streams));
    HIPCHK_OR(undo, hipMalloc(&b->d_amb, sizeof(OpvTxbAmb) * kAmbCap));
    HIPCHK_OR(undo, hipMemset(b->d_state, 0, kStateHead + (size_t)n_streams));
    *out = b;
    return OPV_OK;
}

static int txb_stream(opv_txb* b, int s) {
    if (s < 0 || s >= (int)b->st.size()) return fail(OPV_EINVAL, "opv_txb: stream index out of range");
    return OPV_OK;
}

extern "C" int opv_txb_get_state(opv_txb* b, int stream, opv_txb_state* out) {
    if (!b || !out) return fail(OPV_EINVAL, "opv_txb_get_state: null pointer");
    if (int r = txb_stream(b, stream)) return r;
    *out = b->st[stream];
    return OPV_OK;
}

extern "C" int opv_txb_set_state(opv_txb* b, int stream, const opv_txb_state* in) {
    if (!b || !in) return fail(OPV_EINVAL, "opv_txb_set_state: null pointer");
    if (int r = txb_stream(b, stream)) return r;
    if (const char* why = txb_state_refusal(*in)) return fail(OPV_EINVAL, why);
    if (int r = txb_live(b, "opv_txb_set_state: the bank's context has been destroyed")) return r;
    const uint8_t par = (uint8_t)in->sign_parity;
    HIPCHK(hipMemcpy(b->d_state + kStateHead + stream, &par, 1, hipMemcpyHostToDevice));   // (rounds are synchronous: nothing in flight reads it)
    b->st[stream] = *in;
    return OPV_OK;
}

extern "C" int opv_txb_reset(opv_txb* b, int stream) {
    if (!b) return fail(OPV_EINVAL, "opv_txb_reset: null bank");
    if (stream != -1)
        if (int r = txb_stream(b, stream)) return r;
    if (int r = txb_live(b, "opv_txb_reset: the bank's context has been destroyed")) return r;
    const size_t lo = stream == -1 ? 0 : (size_t)stream, n = stream == -1 ? b->st.size() : 1;
    HIPCHK(hipMemset(b->d_state + kStateHead + lo, 0, n));
    for (size_t s = lo; s < lo + n; ++s) b->st[s] = opv_txb_state{0, 0, 0};
    return OPV_OK;
}

extern "C" long opv_txb_round(opv_txb* b, int count, const int* streams, const uint8_t* const* frames134, const size_t* n_frames,
                              int16_t* const* d_iq_out, int frames_on_device) {
    if (!b) return fail(OPV_EINVAL, "opv_txb_round: null bank");
    if (!b->door.shared->ctx_alive) return fail(OPV_ESTATE, "opv_txb_round: the bank's context has been destroyed");
    // ---- what can refuse the round, all of it on the host: nothing is enqueued and nothing changes before this is through
    if (count > 0 && (!streams || !frames134 || !n_frames || !d_iq_out)) return fail(OPV_EINVAL, "opv_txb_round: null pointer");
    const size_t cnt = count > 0 ? (size_t)count : 0;
    std::vector<uintptr_t> addr(cnt);
    for (size_t i = 0; i < cnt; ++i) {
        if (n_frames[i] && !frames134[i]) return fail(OPV_EINVAL, "opv_txb_round: null frame pointer");
        addr[i] = (uintptr_t)d_iq_out[i];
    }
    std::vector<uint32_t> first_block(cnt + 1);
    std::vector<uint64_t> first_symbol(cnt + 1);
    if (int r = opv_txb_plan_round((int)b->st.size(), b->st.data(), count, streams, n_frames, addr.data(), first_block.data(), first_symbol.data())) return r;
    // ---- the round's table (entries of 0 frames left out) and what its scratch must hold
    std::vector<OpvTxbEntry> ents;
    uint64_t frames_total = 0, ivl_total = 0, reach = 0;
    for (size_t i = 0; i < cnt; ++i) {
        if (n_frames[i] == 0) continue;
        const uint64_t syms = (uint64_t)n_frames[i] * OPV_FSYMS;
        OpvTxbEntry e{};
        e.frames = frames134[i];                    // (host frames: re-pointed into the upload below)
        e.out = (int*)d_iq_out[i];
        e.first_symbol = first_symbol[i];
        e.n_frames = (uint32_t)n_frames[i];
        e.first_frame = (uint32_t)frames_total;
        e.first_block = first_block[i];
        e.first_ivl = (uint32_t)ivl_total;
        e.stream = (uint32_t)streams[i];
        ents.push_back(e);
        frames_total += n_frames[i];
        ivl_total += txb_intervals(first_symbol[i], syms, OPV_TX_CKPT_SYMS);
        if (first_symbol[i] + syms > reach) reach = first_symbol[i] + syms;
    }
    if (ents.empty()) return 0;
    opv_ctx* c = b->ctx;
    HIPCHK(hipSetDevice(b->door.device));
    if (int r = opv_tx_prepare_run(c, (size_t)reach)) return r;
    const size_t m = ents.size(), F = (size_t)frames_total;
    // parts of one allocation, each on a 256-byte boundary; the first two are one upload
    const size_t frames_off = up256(m * sizeof(OpvTxbEntry)), up_bytes = frames_off + (frames_on_device ? 0 : F * OPV_FB);
    const size_t codes_off = up256(up_bytes), fpar_off = codes_off + up256(F * OPV_FSYMS), phases_off = fpar_off + up256(F);
    const size_t need = phases_off + F * OPV_FSYMS * sizeof(double2);
    if (int r = b->scratch.grow(need, need, {b->stream})) return r;
    uint8_t* const d = b->scratch.p;
    b->h_up.resize(up_bytes);
    for (size_t k = 0, i = 0; i < cnt; ++i) {
        if (n_frames[i] == 0) continue;
        if (!frames_on_device) {
            const size_t off = frames_off + (size_t)ents[k].first_frame * OPV_FB;
            std::memcpy(b->h_up.data() + off, frames134[i], n_frames[i] * OPV_FB);
            ents[k].frames = d + off;
        }
        ++k;
    }
    std::memcpy(b->h_up.data(), ents.data(), m * sizeof(OpvTxbEntry));
    // ---- one upload, four launches, the state back: all on the context's stream
    const OpvTxbEntry* d_ents = (const OpvTxbEntry*)d;
    uint8_t *const d_codes = d + codes_off, *const d_fpar = d + fpar_off, *const d_par = b->d_state + kStateHead;
    double2* const d_phases = (double2*)(d + phases_off);
    HIPCHK(hipMemcpyAsync(d, b->h_up.data(), up_bytes, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemsetAsync(b->d_state, 0, sizeof(uint32_t), b->stream));
    k_txb_encode<<<(unsigned)F, 256, 0, b->stream>>>(d_ents, (uint32_t)m, (uint32_t)F, d_codes, d_fpar);
    k_txb_scan<<<(unsigned)((m + 3) / 4), 256, 0, b->stream>>>(d_ents, (uint32_t)m, d_fpar, d_par);
    k_txb_phases<<<(unsigned)((ivl_total + 63) / 64), 64, 0, b->stream>>>(d_ents, (uint32_t)m, (uint32_t)ivl_total, (const double2*)c->tx_ckpt.p, d_phases);
    k_txb_modulate<<<first_block[cnt], 64, 0, b->stream>>>(d_ents, (uint32_t)m, d_codes, d_fpar, d_phases, (uint32_t*)b->d_state, b->d_amb, kAmbCap,
                                                           c->tx_flat_lo, c->tx_flat_hi, c->tx_flat.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(b->h_state.data(), b->d_state, b->h_state.size(), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));                                 // (also: host frames are the caller's again)
    for (const OpvTxbEntry& e : ents) {
        b->st[e.stream].symbols += (uint64_t)e.n_frames * OPV_FSYMS;
        b->st[e.stream].sign_parity = b->h_state[kStateHead + e.stream] & 1;
    }
    uint32_t n_amb = 0;
    std::memcpy(&n_amb, b->h_state.data(), sizeof n_amb);
    if (n_amb > kAmbCap) return fail(OPV_ECAPACITY, "too many ambiguous samples (internal)");
    if (n_amb) {  // re-evaluate with libm exactly like the reference; the list says all the host needs
        std::vector<OpvTxbAmb> list(n_amb);
        HIPCHK(hipMemcpy(list.data(), b->d_amb, sizeof(OpvTxbAmb) * n_amb, hipMemcpyDeviceToHost));
        for (const OpvTxbAmb& a : list) {
            int16_t iq[2];
            txb_patch_sample(a.symbol, a.sample, a.code, iq);
            HIPCHK(hipMemcpy((void*)(uintptr_t)a.addr, iq, 4, hipMemcpyHostToDevice));
        }
    }
    return (long)n_amb;
}
