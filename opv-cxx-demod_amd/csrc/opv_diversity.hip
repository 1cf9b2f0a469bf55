// opv_diversity.hip — the receive-diversity object of include/opv_demod.h (opv_div): its groups and output rings, its round behind
// the context's rounds, its pops, state and parity tap. The kernels are k_diversity.hip's (match, combine) and the thin ones of
// k_frame_decode.hip / k_frame_link.hip (scale, decoder, link record of the combined payload); the rules are opv_div_rules.h's.
// A context without such an object allocates nothing here and launches nothing here.
#include <cmath>
#include <cstring>
#include <vector>

#include "opv_ctx.h"
#include "opv_round_rules.h"
#include "opv_stream_rules.h"

static_assert(sizeof(opv_div_meta) == 88 && sizeof(OpvDivMetaDev) == sizeof(opv_div_meta), "opv_div_meta is 88 bytes, and the device writes it");
static_assert(sizeof(opv_div_state) == 24 && sizeof(opv_div_cfg) == 16, "fixed layouts");

struct opv_div {
    opv_ctx* ctx = nullptr;                       // valid while shared->ctx_alive
    std::shared_ptr<OpvDivShared> shared;
    int device = 0;
    int n_groups = 0;
    uint32_t cap = 0;                             // slots of every output ring: the context's cap_frames
    std::vector<OpvDivGroup> groups;              // host copy: configuration and device pointers (cursors and counters live on the device)
    std::vector<std::vector<uint32_t>> seen;      // [group][branch]: the stream's restart epoch this object has acted on
    std::vector<uint32_t> popped, decoded, perfect;
    std::vector<OpvDivGroup> mirror;              // device -> host, by refresh()
    uint64_t budget_seen = 0;
    OpvDivGroup* d_groups = nullptr;
    void* d_pool = nullptr;                       // one allocation behind every ring of every group
};

namespace {

int div_alive(opv_div* d) {
    if (!d) return fail(OPV_EINVAL, "null diversity object");
    if (!d->shared || !d->shared->ctx_alive) return fail(OPV_ESTATE, "the diversity object's context has been destroyed");
    return OPV_OK;
}
int div_group(opv_div* d, int g) {
    if (int r = div_alive(d)) return r;
    if (g < 0 || g >= d->n_groups) return fail(OPV_EINVAL, "diversity group out of range");
    return OPV_OK;
}
// waits for the context's stream and brings the groups' device halves over
int div_refresh(opv_div* d) {
    HIPCHK(hipSetDevice(d->device));
    HIPCHK(hipStreamSynchronize(d->ctx->stream));
    d->mirror.resize(d->n_groups);
    HIPCHK(hipMemcpy(d->mirror.data(), d->d_groups, sizeof(OpvDivGroup) * d->n_groups, hipMemcpyDeviceToHost));
    return OPV_OK;
}
int div_ring_to_host(void* dst, const void* d_ring, uint32_t first, uint32_t n, uint32_t cap, size_t elem) {
    const RingRuns r = ring_runs(first, n, cap);
    HIPCHK(hipMemcpy(dst, (const char*)d_ring + (size_t)r.p0 * elem, (size_t)r.run0 * elem, hipMemcpyDeviceToHost));
    if (r.run1) HIPCHK(hipMemcpy((char*)dst + (size_t)r.run0 * elem, d_ring, (size_t)r.run1 * elem, hipMemcpyDeviceToHost));
    return OPV_OK;
}
size_t align256(size_t v) { return (v + 255u) & ~(size_t)255u; }

}  // namespace

extern "C" int opv_div_create(opv_div** out, opv_ctx* c, const opv_div_cfg* cfg, const int* n_branches, const int* streams) {
    if (!out || !c || !cfg || !n_branches || !streams) return fail(OPV_EINVAL, "opv_div_create: null argument");
    *out = nullptr;
    if (cfg->n_groups < 1 || cfg->n_groups > 65536) return fail(OPV_EINVAL, "opv_div_create: n_groups must be 1 .. 65536");
    if (cfg->window < 0 || cfg->window > OPV_DIV_MAX_WINDOW) return fail(OPV_EINVAL, "opv_div_create: window must be 0 .. 64 symbols");
    const int G = cfg->n_groups;
    std::vector<uint8_t> named(c->n_streams, 0);
    size_t total = 0;
    for (int g = 0; g < G; ++g) {
        if (n_branches[g] < 1 || n_branches[g] > OPV_DIV_MAX_BRANCHES) return fail(OPV_EINVAL, "opv_div_create: a group has 1 .. 8 branches");
        for (int b = 0; b < n_branches[g]; ++b, ++total) {
            const int s = streams[total];
            if (s < 0 || s >= c->n_streams) return fail(OPV_EINVAL, "opv_div_create: stream index out of range");
            if (named[s]) return fail(OPV_EINVAL, "opv_div_create: a stream is named twice");
            if (c->div.p && c->div.p->owned[s]) return fail(OPV_EINVAL, "opv_div_create: a stream is already a branch of a live diversity object");
            named[s] = 1;
        }
    }
    HIPCHK(hipSetDevice(c->cfg.device));
    if (int r = c->refresh()) return r;                                   // (the branches' frame counts as they stand: where the cursors start)
    if (!c->div.p) {
        c->div.p = std::make_shared<OpvDivShared>();
        c->div.p->owned.assign(c->n_streams, 0);
        c->div.p->epoch.assign(c->n_streams, 0);
        c->div.p->restart.assign(c->n_streams, 0);
    }
    opv_div* d = new opv_div;
    d->ctx = c;
    d->shared = c->div.p;
    d->device = c->cfg.device;
    d->n_groups = G;
    d->cap = c->cap_frames;
    d->budget_seen = d->shared->frames_budget;
    d->popped.assign(G, 0); d->decoded.assign(G, 0); d->perfect.assign(G, 0);
    // one pool: per group meta, factors, payloads, scales, frames, metrics, link records
    const size_t cap = d->cap;
    const size_t b_meta = align256(sizeof(OpvDivMetaDev) * cap), b_fac = align256(sizeof(double) * OPV_DIV_MAX_BRANCHES * cap),
                 b_pay = align256(sizeof(double) * OPV_CODED * cap), b_scale = align256(sizeof(double) * cap),
                 b_frames = align256((size_t)OPV_FB * cap), b_met = align256(sizeof(int32_t) * cap), b_link = align256(sizeof(opv_link) * cap);
    const size_t per_group = b_meta + b_fac + b_pay + b_scale + b_frames + b_met + b_link;
    auto undo = [&](hipError_t e, const char* what) {
        if (d->d_pool) (void)hipFree(d->d_pool);
        if (d->d_groups) (void)hipFree(d->d_groups);
        delete d;
        return alloc_failed(e, what, "opv_div_create: the groups' output rings");
    };
    HIPCHK_OR(undo, hipMalloc(&d->d_pool, per_group * G));
    HIPCHK_OR(undo, hipMalloc((void**)&d->d_groups, sizeof(OpvDivGroup) * G));
    HIPCHK_OR(undo, hipMemsetAsync(d->d_pool, 0, per_group * G, c->stream));
    d->groups.resize(G);
    d->seen.resize(G);
    total = 0;
    for (int g = 0; g < G; ++g) {
        OpvDivGroup& q = d->groups[g];
        std::memset(&q, 0, sizeof q);
        q.n_branches = n_branches[g];
        q.normalise = cfg->normalise != 0;
        q.window = (uint32_t)cfg->window;
        q.cap = d->cap;
        for (int b = 0; b < q.n_branches; ++b, ++total) {
            q.stream[b] = streams[total];
            q.cursor[b] = c->mirror[streams[total]].n_frames;           // frames released before the object existed are not combined
            q.w[b] = 1.0;
            d->seen[g].push_back(d->shared->epoch[streams[total]]);
        }
        char* p = (char*)d->d_pool + per_group * g;
        q.meta = (OpvDivMetaDev*)p; p += b_meta;
        q.factor = (double*)p; p += b_fac;
        q.payload = (double*)p; p += b_pay;
        q.scale = (double*)p; p += b_scale;
        q.frames = (uint8_t*)p; p += b_frames;
        q.metrics = (int32_t*)p; p += b_met;
        q.link = p;
    }
    HIPCHK_OR(undo, hipMemcpyAsync(d->d_groups, d->groups.data(), sizeof(OpvDivGroup) * G, hipMemcpyHostToDevice, c->stream));
    HIPCHK_OR(undo, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < named.size(); ++i)
        if (named[i]) d->shared->owned[i] = 1;
    *out = d;
    return OPV_OK;
}

extern "C" void opv_div_destroy(opv_div* d) {
    if (!d) return;
    (void)hipSetDevice(d->device);
    if (d->shared && d->shared->ctx_alive) {
        (void)hipStreamSynchronize(d->ctx->stream);                       // rounds still in flight read the rings
        for (const OpvDivGroup& q : d->groups)
            for (int b = 0; b < q.n_branches; ++b) d->shared->owned[q.stream[b]] = 0;
    }
    // (a detached object: its context waited for its stream before it went, and the rings were never the context's)
    if (d->d_pool) (void)hipFree(d->d_pool);
    if (d->d_groups) (void)hipFree(d->d_groups);
    delete d;
}

extern "C" int opv_div_set_weights(opv_div* d, int g, const double* w) {
    if (int r = div_group(d, g)) return r;
    if (!w) return fail(OPV_EINVAL, "opv_div_set_weights: null weights");
    OpvDivGroup& q = d->groups[g];
    for (int b = 0; b < q.n_branches; ++b)
        if (!std::isfinite(w[b]) || w[b] < 0.0) return fail(OPV_EINVAL, "opv_div_set_weights: weights must be finite and >= 0");
    HIPCHK(hipSetDevice(d->device));
    for (int b = 0; b < q.n_branches; ++b) q.w[b] = w[b];
    // in stream order: behind the rounds enqueued so far, in front of the next (the host copy is the caller-independent source)
    HIPCHK(hipMemcpyAsync(&d->d_groups[g].w[0], q.w, sizeof q.w, hipMemcpyHostToDevice, d->ctx->stream));
    HIPCHK(hipStreamSynchronize(d->ctx->stream));                         // (q.w may change again at once)
    return OPV_OK;
}

extern "C" int opv_div_round(opv_div* d) {
    if (int r = div_alive(d)) return r;
    opv_ctx* c = d->ctx;
    HIPCHK(hipSetDevice(d->device));
    // branches reset or imported since the last round: their cursors restart (rare; the reset itself waited for the stream)
    for (int g = 0; g < d->n_groups; ++g) {
        OpvDivGroup& q = d->groups[g];
        for (int b = 0; b < q.n_branches; ++b) {
            const int s = q.stream[b];
            if (d->seen[g][b] == d->shared->epoch[s]) continue;
            d->seen[g][b] = d->shared->epoch[s];
            const uint32_t v = d->shared->restart[s] + 1u;
            HIPCHK(hipMemcpyAsync(&d->d_groups[g].restart[b], &v, sizeof v, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
        }
    }
    // the estimate of group frames this round: what the context's rounds since the last one budgeted per stream (one more for a
    // frame that was waiting to become final), at most a ring; the kernels stride, so a backlog is covered whatever the estimate
    uint64_t fr = d->shared->frames_budget - d->budget_seen + 1u;
    d->budget_seen = d->shared->frames_budget;
    if (fr > d->cap) fr = d->cap;
    const uint32_t G = (uint32_t)d->n_groups;
    while (fr > 1 && !round_fits_grid(fr, (int)G)) fr = (fr + 1) / 2;
    k_div_match<<<G, 64, 0, c->stream>>>(d->d_groups, c->d_streams);
    k_div_combine<<<(unsigned)(fr * G), 256, 0, c->stream>>>(d->d_groups, c->d_streams, (uint32_t)fr);
    k_div_scale<<<(unsigned)((fr * G + 63) / 64), 64, 0, c->stream>>>(d->d_groups, (uint32_t)fr, G);
    const uint32_t pairs = (uint32_t)((fr + 1) / 2);
    k_div_decode<<<pairs * G, 64, 0, c->stream>>>(d->d_groups, pairs);
    k_div_link<<<(unsigned)(fr * G), 64, 0, c->stream>>>(d->d_groups, (uint32_t)fr);
    HIPCHK(hipGetLastError());
    return OPV_OK;
}

extern "C" long opv_div_pop_frames(opv_div* d, int g, uint8_t* out, size_t cap, opv_div_meta* meta, opv_link* link) {
    if (int r = div_group(d, g)) return r;
    if (int r = div_refresh(d)) return r;
    const OpvDivGroup& q = d->mirror[g];
    const uint32_t nf = q.n_frames;
    uint32_t f = d->popped[g];
    if (f >= nf || cap == 0) return 0;
    uint32_t n = nf - f;
    if (n > q.cap) n = q.cap;                                             // (never: a full ring stalls the group)
    std::vector<int32_t> met(n);
    std::vector<OpvDivMetaDev> rec(n);
    std::vector<opv_link> lk(n);
    std::vector<uint8_t> fr((size_t)n * OPV_FB);
    if (int r = div_ring_to_host(met.data(), q.metrics, f, n, q.cap, sizeof(int32_t))) return r;
    if (int r = div_ring_to_host(rec.data(), q.meta, f, n, q.cap, sizeof(OpvDivMetaDev))) return r;
    if (int r = div_ring_to_host(fr.data(), q.frames, f, n, q.cap, OPV_FB)) return r;
    if (link) { if (int r = div_ring_to_host(lk.data(), q.link, f, n, q.cap, sizeof(opv_link))) return r; }
    size_t w = 0;
    uint32_t k = 0;
    for (; k < n && w < cap; ++k) {
        if (met[k] == INT32_MIN) break;                                   // emitted, not decoded (cannot happen behind a whole round)
        if (met[k] < 0) continue;                                         // dropped: no branch summed, or a silent sum (ref :859)
        if (out) std::memcpy(out + w * OPV_FB, fr.data() + (size_t)k * OPV_FB, OPV_FB);
        if (meta) {
            std::memcpy(&meta[w], &rec[k], sizeof(opv_div_meta));
            meta[w].viterbi_metric = met[k];
        }
        if (link) link[w] = lk[k];
        ++d->decoded[g];
        if (met[k] == 0) ++d->perfect[g];
        ++w;
    }
    for (; k < n && met[k] < 0 && met[k] != INT32_MIN; ++k) {}            // dropped frames behind the last one handed out go too
    d->popped[g] = f + k;
    HIPCHK(hipMemcpy(&d->d_groups[g].popped, &d->popped[g], sizeof(uint32_t), hipMemcpyHostToDevice));   // (the stream is idle: refresh waited)
    return (long)w;
}

extern "C" int opv_div_get_state(opv_div* d, int g, opv_div_state* out) {
    if (int r = div_group(d, g)) return r;
    if (!out) return fail(OPV_EINVAL, "opv_div_get_state: null out");
    if (int r = div_refresh(d)) return r;
    const OpvDivGroup& q = d->mirror[g];
    std::memset(out, 0, sizeof *out);
    out->frames_emitted = q.n_frames;
    out->frames_decoded = d->decoded[g];
    out->frames_perfect = d->perfect[g];
    out->records_lost = q.records_lost;
    out->softs_lost = q.softs_lost;
    out->stalled = q.stalled;
    if (q.n_frames > d->popped[g]) {                                      // emitted, not popped yet
        uint32_t n = q.n_frames - d->popped[g];
        if (n > q.cap) n = q.cap;
        std::vector<int32_t> met(n);
        if (int r = div_ring_to_host(met.data(), q.metrics, d->popped[g], n, q.cap, sizeof(int32_t))) return r;
        for (int32_t m : met)
            if (m >= 0) { out->frames_decoded++; if (m == 0) out->frames_perfect++; }
    }
    return OPV_OK;
}

extern "C" long opv_div_tap_payload(opv_div* d, int g, uint32_t frame, double* out2144) {
    if (int r = div_group(d, g)) return r;
    if (!out2144) return fail(OPV_EINVAL, "opv_div_tap_payload: null out");
    if (int r = div_refresh(d)) return r;
    const OpvDivGroup& q = d->mirror[g];
    if (frame >= q.n_frames || q.n_frames - frame > q.cap) return fail(OPV_EINVAL, "opv_div_tap_payload: that group frame does not exist or has left the ring");
    HIPCHK(hipMemcpy(out2144, q.payload + (size_t)(frame % q.cap) * OPV_CODED, sizeof(double) * OPV_CODED, hipMemcpyDeviceToHost));
    return OPV_CODED;
}
