// opv_link.hip — the per-frame link report of include/opv_demod.h (opv_link): its ring, its launch behind the decoder, its pops
// and the stand-alone form. The kernels are k_frame_link.hip's. Off by default: a context that never enables the report
// allocates nothing here and launches nothing here.
#include <cstring>
#include <vector>

#include "opv_ctx.h"
#include "opv_stream_rules.h"

// the fifth stage of opv_process: one wave per frame of the round's estimate, strided like the scale pre-pass
void link_launch(opv_ctx* c, uint64_t fr) {
    if (!c->link_on) return;
    k_frame_link<<<(unsigned)(fr * (uint64_t)c->n_streams), 64, 0, c->stream>>>(c->d_streams, c->d_link, c->cap_frames, (uint32_t)fr);
}

int link_clear(opv_ctx* c, int lo, int hi) {
    if (!c->d_link || hi <= lo) return OPV_OK;
    HIPCHK(hipMemsetAsync(c->d_link + (size_t)c->cap_frames * lo, 0, sizeof(opv_link) * c->cap_frames * (size_t)(hi - lo), c->stream));
    return OPV_OK;
}

extern "C" int opv_enable_link_report(opv_ctx* c, int enable) {
    if (!c) return fail(OPV_EINVAL, "null context");
    HIPCHK(hipSetDevice(c->cfg.device));
    if (enable && !c->link_on) {
        if (!c->d_link) {
            const hipError_t e = hipMalloc(&c->d_link, sizeof(opv_link) * c->cap_frames * (size_t)c->n_streams);
            if (e != hipSuccess) { c->d_link = nullptr; return alloc_failed(e, "hipMalloc", "opv_enable_link_report: the record ring"); }
        }
        // every off -> on transition, in stream order behind the rounds launched so far: frames decoded while the report was off
        // read valid = 0, never a record of the frame that held the slot before. Waited for here (rare, not on the hot path): the
        // zero-fill is the ring's only initialisation, and a pop may follow with no round in between
        if (int r = link_clear(c, 0, c->n_streams)) return r;
        HIPCHK(hipStreamSynchronize(c->stream));
        c->link_epoch = ~0u;                               // (the host copy of the ring, if any, is stale)
    }
    c->link_on = enable != 0;
    return OPV_OK;
}

extern "C" int opv_device_link(opv_ctx* c, const opv_link** d_link) {
    if (!c || !d_link) return fail(OPV_EINVAL, "null argument");
    if (!c->d_link) return fail(OPV_ESTATE, "opv_device_link: the link report was never enabled (opv_enable_link_report)");
    *d_link = c->d_link;
    return OPV_OK;
}

// records [first, first + n) of stream s, and the metrics of the same frames, to the host. Like the other record pools
// (opv_ctx::ensure_pools) the ring comes over ONCE per round for all streams while the pools are small enough to be mirrored - a
// server popping thousands of streams pays no device round trip per stream - and per stream otherwise. On the context's stream,
// then waited for: behind whatever has been queued there.
static int link_to_host(opv_ctx* c, int s, uint32_t first, uint32_t n, int32_t* met, opv_link* rec) {
    const RingRuns r = ring_runs(first, n, c->cap_frames);
    const size_t base = (size_t)c->cap_frames * s;
    bool have = false;
    if (int e = c->ensure_pools(&have)) return e;
    if (have) {
        if (c->link_epoch != c->mirror_epoch) {
            c->m_link.resize((size_t)c->cap_frames * c->n_streams);
            HIPCHK(hipMemcpyAsync(c->m_link.data(), c->d_link, c->m_link.size() * sizeof(opv_link), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            c->link_epoch = c->mirror_epoch;
        }
        std::memcpy(met, c->m_metrics.data() + base + r.p0, sizeof(int32_t) * r.run0);
        std::memcpy(rec, c->m_link.data() + base + r.p0, sizeof(opv_link) * r.run0);
        if (r.run1) {
            std::memcpy(met + r.run0, c->m_metrics.data() + base, sizeof(int32_t) * r.run1);
            std::memcpy(rec + r.run0, c->m_link.data() + base, sizeof(opv_link) * r.run1);
        }
        return OPV_OK;
    }
    HIPCHK(hipMemcpyAsync(met, c->d_metrics + base + r.p0, sizeof(int32_t) * r.run0, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(rec, c->d_link + base + r.p0, sizeof(opv_link) * r.run0, hipMemcpyDeviceToHost, c->stream));
    if (r.run1) {
        HIPCHK(hipMemcpyAsync(met + r.run0, c->d_metrics + base, sizeof(int32_t) * r.run1, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(rec + r.run0, c->d_link + base, sizeof(opv_link) * r.run1, hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    return OPV_OK;
}

// opv_pop_frames, then the records of the frames it handed out: the frames consumed are [popped before, popped after) and the
// ones handed out among them are those the decoder did not drop, which the metrics ring says
extern "C" long opv_pop_frames_link(opv_ctx* c, int s, uint8_t* out, size_t cap, opv_frame_meta* meta, opv_link* link) {
    if (int r = check_stream(c, s)) return r;
    if (!link) return fail(OPV_EINVAL, "opv_pop_frames_link: null link");
    if (!c->link_on) return fail(OPV_ESTATE, "opv_pop_frames_link: the link report is off (opv_enable_link_report)");
    const uint32_t before = c->hs[s].popped;
    const long n = opv_pop_frames(c, s, out, cap, meta);
    if (n <= 0) return n;
    const uint32_t cnt = c->hs[s].popped - before;         // (<= cap_frames: a stream with a full frame ring pauses)
    std::vector<int32_t> met(cnt);
    std::vector<opv_link> rec(cnt);
    if (int r = link_to_host(c, s, before, cnt, met.data(), rec.data())) return r;
    long w = 0;
    for (uint32_t k = 0; k < cnt && w < n; ++k)
        if (met[k] >= 0) link[w++] = rec[k];
    if (w != n) return fail(OPV_EHIP, "opv_pop_frames_link: the metrics ring disagrees with the frames handed out");
    return n;
}

extern "C" int opv_link_payloads(opv_ctx* c, const double* soft, size_t n, opv_link* out) {
    if (!c || !soft || !out) return fail(OPV_EINVAL, "null argument");
    if (n == 0 || n > 0x7FFFFFFFull) return fail(OPV_EINVAL, "opv_link_payloads: n_frames must be 1 .. 2^31 - 1");
    HIPCHK(hipSetDevice(c->cfg.device));
    double *d_soft = nullptr, *d_scale = nullptr;
    uint8_t* d_out = nullptr;
    int32_t* d_met = nullptr;
    opv_link* d_rec = nullptr;
    int rc = OPV_OK;
    auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == OPV_OK) rc = fail(OPV_EHIP, w, e); };
    chk(hipMalloc(&d_soft, sizeof(double) * OPV_CODED * n), "hipMalloc soft");
    chk(hipMalloc(&d_scale, sizeof(double) * n), "hipMalloc scales");
    chk(hipMalloc(&d_out, (size_t)OPV_FB * n), "hipMalloc frames");
    chk(hipMalloc(&d_met, sizeof(int32_t) * n), "hipMalloc metrics");
    chk(hipMalloc(&d_rec, sizeof(opv_link) * n), "hipMalloc records");
    if (rc == OPV_OK) {
        chk(hipMemcpyAsync(d_soft, soft, sizeof(double) * OPV_CODED * n, hipMemcpyHostToDevice, c->stream), "H2D soft");
        chk(hipMemsetAsync(d_out, 0, (size_t)OPV_FB * n, c->stream), "memset");
        k_payload_scale<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_soft, (uint32_t)n, d_scale);
        k_decode_payloads<<<(unsigned)((n + 1) / 2), 64, 0, c->stream>>>(d_soft, (uint32_t)n, d_scale, d_out, d_met, nullptr, nullptr, nullptr);
        k_link_payloads<<<(unsigned)n, 64, 0, c->stream>>>(d_soft, (uint32_t)n, d_scale, d_out, d_met, d_rec);
        chk(hipGetLastError(), "k_link_payloads launch");
        chk(hipMemcpyAsync(out, d_rec, sizeof(opv_link) * n, hipMemcpyDeviceToHost, c->stream), "D2H records");
        chk(hipStreamSynchronize(c->stream), "sync");
    }
    void* ptrs[] = {d_soft, d_scale, d_out, d_met, d_rec};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    return rc;
}
