// opv_capi.hip — the thin C-ABI HIP shim behind include/opv_demod.h: a context's life, opv_process, pops, state and taps.
// (opv_push.hip: the serving path; opv_migrate.hip; opv_link.hip: the link report; opv_tx_device.hip; opv_rccl.hip; opv_ctx.h: what they share.)
//
// Owns device memory and the per-stream device contexts and launches the four hot-path kernels on one HIP stream. There is
// NO CPU implementation of the hot path in this library: without a usable HIP device opv_create fails with OPV_ENODEV.
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>

#include "opv_ctx.h"
#include "opv_offset_host.h"
#include "opv_round_rules.h"
#include "opv_stream_rules.h"

namespace {

thread_local std::string g_err;

// the front-end kernels by their id in opv_round_rules.h (which says when each runs and with which launch): what opv_process
// launches and names, opv_tap_occupancy asks about and opv_create prepares. k_coherent_frontend takes other arguments than the rest.
using MskFrontend = void (*)(OpvStream*, OpvGlobalCfg, int);
#define OPV_FE(k) {(const void*)k, #k}
const struct { const void* fn; const char* name; } kFrontend[FE_N] = {OPV_FE(k_coherent_frontend), OPV_FE(k_msk_frontend_rb), OPV_FE(k_msk_frontend_rb_wg4),
    OPV_FE(k_msk_frontend_x4_wg4), OPV_FE(k_msk_frontend_x16), OPV_FE(k_msk_frontend_x16_wg4), OPV_FE(k_msk_frontend_x16_wg8)};
#undef OPV_FE

__global__ void k_apply_inputs(OpvStream* streams, const StreamIn* in, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        if (in[i].dirty) {
            streams[i].iq = in[i].iq;
            streams[i].n_avail = in[i].n_avail;
            streams[i].eof = in[i].eof;
        }
        streams[i].frames_popped = in[i].frames_popped;
        streams[i].events_popped = in[i].events_popped;
    }
}

// per round: frames released so far per stream (the zero-copy consumers' counts), and whether ANY stream ended the round
// held back by back-pressure, OR-ed into a pinned host word (opv_ctx::h_stall) that the next opv_process reads without a copy
__global__ void k_collect_counts(const OpvStream* streams, int32_t* counts, int n, int* any_stalled) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        counts[i] = (int32_t)streams[i].n_frames;
        if (streams[i].stalled) *(volatile int*)any_stalled = 1;   // (every writer stores the same 1: no atomic needed across PCIe)
    }
}

__global__ void k_fill_i32(int32_t* p, int32_t v, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

}  // namespace

int opv_int_fail(int code, const char* what, hipError_t e) {
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    g_err = buf;
    return code;
}

extern "C" const char* opv_last_error(void) { return g_err.c_str(); }
extern "C" int opv_abi_version(void) { return OPV_ABI_VERSION; }

extern "C" int opv_create(opv_ctx** out, int n_streams, const opv_cfg* cfg) {
    if (!out || !cfg || n_streams <= 0 || cfg->max_samples == 0) return fail(OPV_EINVAL, "opv_create: bad arguments");
    if (cfg->max_samples >= (1ull << 31)) return fail(OPV_EINVAL, "opv_create: max_samples must be < 2^31");
    // the reference's phase wraps are `while (ph > pi) ph -= 2 pi` loops (src/opv-demod.cpp:255-262,488-493): with an infinite -o / -a / -p
    // it spins forever on its CPU; here that would be a wave that never finishes, so such values are refused up front
    if ((cfg->have_init_offset && !std::isfinite(cfg->init_offset_hz)) || !std::isfinite(cfg->afc_alpha) || (cfg->coherent && !std::isfinite(cfg->pll_bw_hz)))
        return fail(OPV_EINVAL, "opv_create: init_offset_hz / afc_alpha / pll_bw_hz must be finite");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(OPV_ENODEV, "no HIP device visible");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(OPV_ENODEV, "opv_cfg.device out of range");
    HIPCHK(hipSetDevice(cfg->device));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, cfg->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(OPV_ENODEV, "device is not gfx950 (MI355X); this library carries gfx950 code objects only");

    opv_ctx* c = new (std::nothrow) opv_ctx();
    if (!c) return fail(OPV_ENOMEM, "host allocation failed");
    c->n_streams = n_streams;
    c->cfg = *cfg;
    c->n_cu = prop.multiProcessorCount;
    c->hs.resize(n_streams);
    c->mirror.resize(n_streams);

    const uint64_t M = cfg->max_samples;
    c->cap_soft = 1;  // power-of-two ring: one opv_process worth of symbols (<= M/38) + a frame in flight
    while (c->cap_soft < M / 38 + 4096) c->cap_soft <<= 1;
    c->cap_frames = (uint32_t)(M / (uint64_t)(OPV_FSYMS * 38) + 4);
    c->cap_events = 4 * c->cap_frames + 64;
    c->cap_chunks = (uint32_t)(M / 80000 + 4);

    auto cleanup = [&](int code) { opv_destroy(c); return code; };
    auto hip_failed = [&](hipError_t e, const char* what) { return cleanup(fail(e == hipErrorOutOfMemory ? OPV_ENOMEM : OPV_EHIP, what, e)); };

    HIPCHK_OR(hip_failed, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    {   // The copy stream also carries a KERNEL (k_push_gather). The runtime has a handful of hardware queues per priority and
        // deals streams onto them round-robin: in a process with several contexts the kernel stream and the copy stream of one
        // context can land on the same queue, and the moves of round r + 1 then wait for the kernels of round r (bench.py's
        // pcie_inclusive: 109 ms instead of 70). A stream of another PRIORITY comes from another set of queues.
        int least = 0, greatest = 0;
        if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess ||
            hipStreamCreateWithPriority(&c->copy_stream, hipStreamNonBlocking, greatest) != hipSuccess) {
            (void)hipGetLastError();                       // (no priorities here: an ordinary stream - correct, the overlap is then up to the queue deal)
            c->copy_stream = nullptr;
            HIPCHK_OR(hip_failed, hipStreamCreateWithFlags(&c->copy_stream, hipStreamNonBlocking));
        }
    }
    const size_t S = (size_t)n_streams;
    HIPCHK_OR(hip_failed, hipHostMalloc(&c->h_in, sizeof(StreamIn) * S * opv_ctx::kInSlots, hipHostMallocDefault));
    for (auto& e : c->in_ev) HIPCHK_OR(hip_failed, hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK_OR(hip_failed, hipHostMalloc(&c->h_stall, sizeof(int) * opv_ctx::kInSlots, hipHostMallocDefault));
    for (int i = 0; i < opv_ctx::kInSlots; ++i) c->h_stall[i] = 0;
    HIPCHK_OR(hip_failed, hipEventCreateWithFlags(&c->done_ev, hipEventDisableTiming));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_streams, sizeof(OpvStream) * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_in, sizeof(StreamIn) * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_soft, sizeof(double) * c->cap_soft * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_frec, sizeof(OpvFrameRec) * c->cap_frames * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_events, sizeof(OpvEventRec) * c->cap_events * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_chunks, sizeof(double) * 5 * c->cap_chunks * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_frames, (size_t)OPV_FB * c->cap_frames * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_metrics, sizeof(int32_t) * c->cap_frames * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_fscale, sizeof(double) * c->cap_frames * S));
    HIPCHK_OR(hip_failed, hipMalloc(&c->d_counts, sizeof(int32_t) * S));
    {   // cos / sin(pi i / 80) x u^k / k!, u = i - 19.5: the tone tables of the offset search folded into its Taylor weights
        std::vector<double> w((size_t)OPV_SPS * 2 * OPV_OFFS_TERMS);
        for (int i = 0; i < OPV_SPS; ++i) {
            const double u = (double)i - 19.5, cs = std::cos(M_PI * i / 80.0), sn = std::sin(M_PI * i / 80.0);
            double t = 1.0;                                // u^k / k!
            for (int k = 0; k < OPV_OFFS_TERMS; ++k) {
                w[((size_t)i * 2 + 0) * OPV_OFFS_TERMS + k] = cs * t;
                w[((size_t)i * 2 + 1) * OPV_OFFS_TERMS + k] = sn * t;
                t = t * u / (double)(k + 1);
            }
        }
        HIPCHK_OR(hip_failed, hipMalloc(&c->d_offs_wtab, sizeof(double) * w.size()));
        HIPCHK_OR(hip_failed, hipMemcpy(c->d_offs_wtab, w.data(), sizeof(double) * w.size(), hipMemcpyHostToDevice));
    }
    // The library's environment switches, all TEST HOOKS (include/opv_demod.h has the table): read here, once per context,
    // and nowhere else - a context never changes its behaviour after it has been created.
    c->host_ties = opv_offset_host_libm_matches_reference() && !std::getenv("OPV_OFFSET_DISTRUST_LIBM");
    c->tx_trust_libm = opv_tx_libm_flat_tops_as_assumed() && !std::getenv("OPV_TX_DISTRUST_LIBM");
    c->push_gather = !std::getenv("OPV_PUSH_NO_GATHER");
    if (const char* e = std::getenv("OPV_PUSH_GATHER_BLOCKS")) { const int v = atoi(e); if (v > 0) c->push_gather_blocks = (uint32_t)v; }
    c->rb_fp64_ring = !std::getenv("OPV_FRONTEND_INT16_RING");
    if (const char* e = std::getenv("OPV_FRONTEND_TF_GUARD")) c->tf_guard = atoi(e) != 0;
    double timing_freq0 = 0.0;               // (strtod, not atof: the tests hand over values one ulp apart as hex floats)
    if (const char* e = std::getenv("OPV_TEST_TIMING_FREQ0")) timing_freq0 = std::strtod(e, nullptr);
    {   // k_msk_frontend_rb addresses its dynamic LDS from address 0 on: it must have no static LDS (k_frontend.hip)
        hipFuncAttributes fa;
        HIPCHK_OR(hip_failed, hipFuncGetAttributes(&fa, kFrontend[FE_RB].fn));
        if (fa.sharedSizeBytes != 0) return cleanup(fail(OPV_EHIP, "k_msk_frontend_rb was built with static LDS"));
    }
    // the fp64-ring shape asks for more dynamic LDS than a launch gets by default (one workgroup per CU)
    if (c->rb_fp64_ring) HIPCHK_OR(hip_failed, hipFuncSetAttribute(kFrontend[FE_RB].fn, hipFuncAttributeMaxDynamicSharedMemorySize, OPV_RB_LDS_F64));
    if (c->host_ties) {
        HIPCHK_OR(hip_failed, hipMalloc(&c->d_tie_list, sizeof(uint32_t) * (S + 1)));
        c->tie.slots = (uint32_t)(S < (size_t)OPV_TIE_SLOTS_MAX ? S : (size_t)OPV_TIE_SLOTS_MAX);
        // (82 MB of pinned memory for 512 slots: a host that cannot pin that much keeps working - the device then decides the ties
        // itself, and opv_offset_ties_on_host() says so)
        if (hipHostMalloc((void**)&c->tie.stage, offsetof(OpvTieStage, slot) + sizeof(OpvTieSlot) * c->tie.slots, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            c->tie.stage = nullptr;
            c->host_ties = false;
        } else {
            c->tie.stage->n = c->tie.stage->listed = c->tie.stage->beyond = 0;
        }
    }
    HIPCHK_OR(hip_failed, hipMemsetAsync(c->d_frames, 0, (size_t)OPV_FB * c->cap_frames * S, c->stream));
    HIPCHK_OR(hip_failed, hipMemsetAsync(c->d_counts, 0, sizeof(int32_t) * S, c->stream));
    k_fill_i32<<<256, 256, 0, c->stream>>>(c->d_metrics, INT32_MIN, (size_t)c->cap_frames * S);

    for (size_t i = 0; i < S; ++i) {
        OpvStream s;
        std::memset(&s, 0, sizeof s);
        s.soft = c->d_soft + c->cap_soft * i;
        s.cap_soft = c->cap_soft;
        s.frec = c->d_frec + (size_t)c->cap_frames * i;
        s.events = c->d_events + (size_t)c->cap_events * i;
        s.chunk_log = c->d_chunks + (size_t)5 * c->cap_chunks * i;
        s.frames = c->d_frames + (size_t)OPV_FB * c->cap_frames * i;
        s.metrics = c->d_metrics + (size_t)c->cap_frames * i;
        s.fscale = c->d_fscale + (size_t)c->cap_frames * i;
        s.cap_frames = c->cap_frames;
        s.cap_events = c->cap_events;
        s.cap_chunks = c->cap_chunks;
        // demod.set_freq_offset(init_offset) only in streaming mode (ref :1004-1005)
        s.freq_offset = (cfg->streaming && cfg->have_init_offset) ? cfg->init_offset_hz : 0.0;
        s.afc_alpha = cfg->afc_alpha;  // set_afc_bandwidth (ref :1009 / :1172)
        s.timing_freq = timing_freq0;  // 0 (ref :341) unless the test hook says otherwise
        s.est_offset = NAN;
        s.x40c = 1.0;  // X[40] of a (non-existent) previous symbol; only ever multiplies a zero prev
        s.trk_state = OPV_HUNTING;
        c->mirror[i] = s;
    }
    c->initial = c->mirror;
    HIPCHK_OR(hip_failed, hipMemcpyAsync(c->d_streams, c->mirror.data(), sizeof(OpvStream) * S, hipMemcpyHostToDevice, c->stream));
    HIPCHK_OR(hip_failed, hipStreamSynchronize(c->stream));
    c->mirror_valid = true;
    *out = c;
    return OPV_OK;
}

extern "C" void opv_destroy(opv_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->cfg.device);       // (a host with contexts on several GPUs: free on the context's own device)
    if (c->copy_stream) (void)hipStreamSynchronize(c->copy_stream);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (auto& e : c->in_ev)
        if (e) (void)hipEventDestroy(e);
    if (c->h_in) (void)hipHostFree(c->h_in);
    if (c->h_stall) (void)hipHostFree(c->h_stall);
    if (c->tie.stage) (void)hipHostFree(c->tie.stage);
    if (c->push_ev) (void)hipEventDestroy(c->push_ev);
    if (c->done_ev) (void)hipEventDestroy(c->done_ev);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    for (auto& h : c->hs) { (void)hipFree(h.d_iq_owned); (void)hipFree(h.d_iq_alt); }   // (a null pointer is a no-op)
    for (auto& e : c->ev)
        if (e) (void)hipEventDestroy(e);
    void* ptrs[] = {c->d_streams, c->d_in, c->d_soft, c->d_frec, c->d_events, c->d_chunks, c->d_frames, c->d_metrics, c->d_fscale, c->d_counts, c->d_link, c->d_offs_wtab, c->d_tx_cnt, c->d_tx_list, c->d_tie_list};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    if (c->stream) (void)hipStreamDestroy(c->stream);
    delete c;                                 // (its grow-only buffers free themselves: GrowBuf)
}

// The host function of one pass of the tie decision (hipLaunchHostFunc, behind k_tie_collect; k_tie_apply follows): the
// contenders of every filled slot are evaluated by the reference's loop on the host's libm (opv_offset_host.cpp). Runs on a
// thread of the runtime in stream order; touches pinned memory and the context's counter only - no HIP call.
static void tie_host_fn(void* p) {
    opv_ctx::TieWork* w = (opv_ctx::TieWork*)p;
    uint32_t n = w->stage->n;
    if (n > w->slots) n = w->slots;
    if (w->stage->beyond) w->left.fetch_add(w->stage->beyond, std::memory_order_relaxed);   // (the round's last pass reports what no pass staged)
    if (n == 0) return;
    opv_offset_decide_slots(w->stage->slot, n);
    w->decided.fetch_add(n, std::memory_order_relaxed);
}

// ---- opv_process, stage by stage. What is decided comes from opv_round_rules.h; these enqueue it on c->stream, in this order.
namespace {

struct RoundInputs { bool any; uint64_t max_new, max_tapped; };

// 1. every stream's update into the round's pinned slot; c->search_now: the streams whose offset search is due
RoundInputs collect_inputs(opv_ctx* c, StreamIn* in) {
    RoundInputs r{false, 0, 0};
    c->search_now.clear();
    for (int i = 0; i < c->n_streams; ++i) {
        const HostStream& h = c->hs[i];
        in[i] = {h.d_iq, h.n_avail, h.eof, h.dirty ? 1 : 0, h.popped, h.events_popped};
        if (h.dirty || h.tap_fresh) r.any = true;          // (tap_fresh: soft symbols staged by opv_tap_push_soft: work for the tracker and the decoder only)
        if (search_due(c->cfg.streaming, h.n_avail, h.eof, h.search_seen)) c->search_now.push_back(i);
        const uint64_t fresh = h.n_avail - h.last_round_avail;
        if (fresh > r.max_new) r.max_new = fresh;
        if (h.tap_fresh > r.max_tapped) r.max_tapped = h.tap_fresh;
    }
    return r;
}

// 2. nothing new: still run the round while a stream may be waiting behind back-pressure (it resumes by itself once
// the tracker has consumed soft symbols / the caller has popped frames; the cursors travel with every round).
// Whether one is: the last round's kernels said so in a pinned word (a caller on the zero-copy path - opv_device_frames +
// opv_sync, no pops - never refreshes the mirror); while that round is still running the answer is "maybe".
bool round_idle(opv_ctx* c, bool any) {
    if (any) return false;
    if (c->maybe_stalled && c->round_no > 0 && hipEventQuery(c->done_ev) == hipSuccess)
        c->maybe_stalled = c->h_stall[(c->round_no - 1) % opv_ctx::kInSlots] != 0;
    return !c->maybe_stalled;
}

// 4. the round will be launched: only now is the host's view of the streams advanced (a refused round leaves it untouched)
void commit_host_view(opv_ctx* c, int slot) {
    for (HostStream& h : c->hs) {
        h.last_round_avail = h.n_avail;
        h.dirty = false;
        h.tap_fresh = 0;
    }
    for (int i : c->search_now) c->hs[i].search_seen = true;
    c->mirror_valid = false;
    c->maybe_stalled = true;
    c->h_stall[slot] = 0;          // (a straggler of round_no - kInSlots could still set it: then one idle round too many, never one too few)
}

// 5. pinned -> device, in stream order behind the previous round's kernels; no host wait
int upload_inputs(opv_ctx* c, const StreamIn* in, int slot) {
    const int S = c->n_streams;
    // samples of an asynchronous batch still crossing PCIe: this round's kernels read them, so they queue behind the moves (on the device)
    if (c->push_pending) HIPCHK(hipStreamWaitEvent(c->stream, c->push_ev, 0));
    HIPCHK(hipMemcpyAsync(c->d_in, in, sizeof(StreamIn) * S, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(c->in_ev[slot], c->stream));
    ++c->round_no;
    k_apply_inputs<<<(S + 63) / 64, 64, 0, c->stream>>>(c->d_streams, c->d_in, S);
    if (c->timing) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    return OPV_OK;
}

// 6. the offset search, and its near-ties decided with the host's libm before the front-end takes the estimate, IN STREAM ORDER:
// per pass (tie_passes) of tie.slots listed streams a kernel stages their inputs in pinned memory, a host function decides them
// (opv_offset_host.cpp), a kernel carries the results back. The caller never waits.
int launch_search(opv_ctx* c, const OpvGlobalCfg& g) {
    const int S = c->n_streams;
    const size_t n_search = round_searches(c->cfg.streaming, c->cfg.have_init_offset, c->search_now.size());
    const bool host_ties = n_search != 0 && c->host_ties;
    if (host_ties) HIPCHK(hipMemsetAsync(c->d_tie_list, 0, sizeof(uint32_t), c->stream));
    k_offset_search<<<S, 256, 0, c->stream>>>(c->d_streams, g, c->d_offs_wtab, host_ties ? c->d_tie_list : nullptr);
    if (c->timing) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    if (host_ties) {
        const uint32_t K = c->tie.slots, passes = tie_passes(n_search, K);
        for (uint32_t p = 0; p < passes; ++p) {
            k_tie_collect<<<K, 256, 0, c->stream>>>(c->d_streams, c->d_tie_list, p, K, p + 1 == passes ? 1u : 0u, c->tie.stage);
            if (hipLaunchHostFunc(c->stream, tie_host_fn, &c->tie) != hipSuccess) {
                // a runtime that cannot enqueue host functions: the round goes on with the device's decisions (the staging kernel
                // left ties = 0 in every slot, so nothing would be applied anyway), and from now on the context says so
                (void)hipGetLastError();
                c->host_ties = false;
                break;
            }
            k_tie_apply<<<K, 192, 0, c->stream>>>(c->d_streams, c->tie.stage, K, S);
        }
    }
    if (c->timing) HIPCHK(hipEventRecord(c->ev[2], c->stream));
    return OPV_OK;
}

// 7. the front-end: the kernel and launch frontend_choice names
int launch_frontend(opv_ctx* c, const OpvGlobalCfg& g) {
    const int S = c->n_streams;
    const FrontendChoice ch = frontend_choice(S, c->frontend, c->cfg.coherent, c->cfg.streaming, c->rb_fp64_ring, c->n_cu);
    c->last_frontend = kFrontend[ch.kernel].name;
    if (ch.kernel == FE_COHERENT) {
        const double wn = c->cfg.pll_bw_hz * 2.0 * M_PI, zeta = 0.707, fsym = 2168000.0 / 40.0;   // set_pll_bandwidth (ref :551-558)
        k_coherent_frontend<<<ch.grid, ch.threads, ch.lds, c->stream>>>(c->d_streams, 2.0 * zeta * wn / fsym, wn * wn / (fsym * fsym));
    } else {
        ((MskFrontend)kFrontend[ch.kernel].fn)<<<ch.grid, ch.threads, ch.lds, c->stream>>>(c->d_streams, g, S);
    }
    if (c->timing) HIPCHK(hipEventRecord(c->ev[3], c->stream));
    return OPV_OK;
}

// 8. the back half: tracker, the quantiser's scale, decoder (scale_shape / decode_grid), the opt-in link report, the counts
int launch_back_half(opv_ctx* c, uint64_t fr, int slot) {
    const int S = c->n_streams;
    const bool tm = c->timing;
    if (tm) HIPCHK(hipEventRecord(c->ev[4], c->stream));
    k_sync_track<<<S, 64, 0, c->stream>>>(c->d_streams);
    if (tm) { HIPCHK(hipEventRecord(c->ev[5], c->stream)); HIPCHK(hipEventRecord(c->ev[6], c->stream)); }
    const ScaleShape sc = scale_shape(fr, S);
    if (sc.wave) k_frame_scale_wave<<<sc.grid, 64, 0, c->stream>>>(c->d_streams, (uint32_t)fr);
    else k_frame_scale<<<sc.grid, 64, 0, c->stream>>>(c->d_streams, (uint32_t)fr, (uint32_t)S);
    k_frame_decode<<<decode_grid(fr, S), 64, 0, c->stream>>>(c->d_streams, decode_pairs(fr));
    if (tm) { HIPCHK(hipEventRecord(c->ev[7], c->stream)); c->timing_valid = true; }
    link_launch(c, fr);            // the opt-in fifth stage (opv_link.hip): behind the decoder's bracket, nothing while it is off
    k_collect_counts<<<(S + 63) / 64, 64, 0, c->stream>>>(c->d_streams, c->d_counts, S, c->h_stall + slot);
    HIPCHK(hipEventRecord(c->done_ev, c->stream));
    HIPCHK(hipGetLastError());
    return OPV_OK;
}

}  // namespace

extern "C" int opv_process(opv_ctx* c) {
    if (!c) return fail(OPV_EINVAL, "null context");
    HIPCHK(hipSetDevice(c->cfg.device));
    const int S = c->n_streams;
    const int slot = (int)(c->round_no % opv_ctx::kInSlots);
    if (c->round_no >= (unsigned)opv_ctx::kInSlots) HIPCHK(hipEventSynchronize(c->in_ev[slot]));  // upload of round_no-kInSlots done
    StreamIn* in = c->h_in + (size_t)slot * S;
    const RoundInputs ri = collect_inputs(c, in);
    if (round_idle(c, ri.any)) return OPV_OK;
    // 3. the frame budget and the refusal, before anything is launched
    const uint64_t fr = round_frames(ri.max_new, ri.max_tapped, c->cap_frames);
    if (!round_fits_grid(fr, S)) return fail(OPV_EINVAL, "opv_process: streams x frames per round exceeds the grid limit");
    commit_host_view(c, slot);
    c->div.launched(fr);
    const OpvGlobalCfg g{c->cfg.streaming, c->cfg.have_init_offset, c->cfg.init_offset_hz, c->tf_guard ? 1 : 0, 0};
    if (int r = upload_inputs(c, in, slot)) return r;
    if (int r = launch_search(c, g)) return r;
    if (int r = launch_frontend(c, g)) return r;
    return launch_back_half(c, fr, slot);
}

extern "C" int opv_set_frontend(opv_ctx* c, int streams_per_wave) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (streams_per_wave != 0 && streams_per_wave != 1 && streams_per_wave != 4 && streams_per_wave != 16)
        return fail(OPV_EINVAL, "opv_set_frontend: 0 (automatic), 1, 4 or 16 streams per wave");
    c->frontend = streams_per_wave;
    return OPV_OK;
}

extern "C" const char* opv_frontend_kernel(opv_ctx* c) { return c ? c->last_frontend : ""; }

extern "C" int opv_sync(opv_ctx* c) {
    if (!c) return fail(OPV_EINVAL, "null context");
    HIPCHK(hipStreamSynchronize(c->stream));
    return OPV_OK;
}

extern "C" int opv_reset_stream(opv_ctx* c, int s) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (s != -1) { if (int r = check_stream(c, s)) return r; }
    if (int r = settle_pushes(c)) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    const int lo = (s == -1) ? 0 : s, hi = (s == -1) ? c->n_streams : s + 1;
    for (int i = lo; i < hi; ++i) c->hs[i] = reset_host_stream(c->hs[i]);
    for (int i = lo; i < hi; ++i) c->div.restarted(i, 0u);     // (a diversity group's cursor for the stream restarts at frame 0)
    HIPCHK(hipMemcpyAsync(c->d_streams + lo, &c->initial[lo], sizeof(OpvStream) * (hi - lo), hipMemcpyHostToDevice, c->stream));
    k_fill_i32<<<256, 256, 0, c->stream>>>(c->d_metrics + (size_t)c->cap_frames * lo, INT32_MIN,
                                          (size_t)c->cap_frames * (hi - lo));
    if (int r = link_clear(c, lo, hi)) return r;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->mirror_valid = false;
    return OPV_OK;
}

extern "C" int opv_enable_timing(opv_ctx* c, int enable) {
    if (!c) return fail(OPV_EINVAL, "null context");
    HIPCHK(hipSetDevice(c->cfg.device));
    if (enable)
        for (auto& e : c->ev)
            if (!e) HIPCHK(hipEventCreate(&e));
    c->timing = enable != 0;
    c->timing_valid = false;
    return OPV_OK;
}

extern "C" int opv_kernel_times(opv_ctx* c, float ms[4]) {
    if (!c || !ms) return fail(OPV_EINVAL, "null argument");
    if (!c->timing_valid) return fail(OPV_ESTATE, "no timed opv_process yet (opv_enable_timing first)");
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int k = 0; k < 4; ++k) HIPCHK(hipEventElapsedTime(&ms[k], c->ev[2 * k], c->ev[2 * k + 1]));
    return OPV_OK;
}

// the (at most two) runs `r` of a device ring of `elem`-byte slots against the linear host buffer `lin`: ring -> lin, or lin -> ring
// with hipMemcpyHostToDevice; asynchronous on `stream` where one is given
static int ring_copy(void* lin, const void* d_ring, const RingRuns& r, size_t elem, hipMemcpyKind kind, hipStream_t stream = nullptr) {
    const size_t at[2] = {(size_t)r.p0 * elem, 0}, bytes[2] = {(size_t)r.run0 * elem, (size_t)r.run1 * elem};
    for (int k = 0; k < 2 && bytes[k]; ++k) {
        void *h = (char*)lin + k * bytes[0], *d = (char*)d_ring + at[k], *dst = kind == hipMemcpyHostToDevice ? d : h, *src = dst == d ? h : d;
        HIPCHK(stream ? hipMemcpyAsync(dst, src, bytes[k], kind, stream) : hipMemcpy(dst, src, bytes[k], kind));
    }
    return OPV_OK;
}

// copies records [first, first+n) of a device ring with `cap` slots of `elem` bytes into dst (host)
static int ring_to_host(opv_ctx* c, void* dst, const void* d_ring, uint32_t first, uint32_t n, uint32_t cap, size_t elem) {
    const RingRuns r = ring_runs(first, n, cap);
    bool have = false;
    if (int r = c->ensure_pools(&have)) return r;
    if (have) {
        if (const void* h_ring = c->host_view(d_ring)) {
            std::memcpy(dst, (const char*)h_ring + r.p0 * elem, r.run0 * elem);
            if (r.run1) std::memcpy((char*)dst + r.run0 * elem, h_ring, r.run1 * elem);
            return OPV_OK;
        }
    }
    return ring_copy(dst, d_ring, r, elem, hipMemcpyDeviceToHost);
}

extern "C" long opv_pop_frames(opv_ctx* c, int s, uint8_t* out, size_t cap, opv_frame_meta* meta) {
    if (int r = check_stream(c, s)) return r;
    if (int r = c->refresh()) return r;
    const OpvStream& st = c->mirror[s];
    if (st.overflow == 2) return fail(OPV_EHIP, "front-end: the two wavefronts of a stream lost each other (hand-over timed out)");
    if (st.overflow) return fail(OPV_EINVAL, "opv_cfg.max_samples too large for the soft-symbol ring (internal limit 2^28 symbols)");
    HostStream& h = c->hs[s];
    const uint32_t nf = st.n_frames;
    if (h.popped >= nf || cap == 0) return 0;
    // candidates: at most `cap` decodable frames can be returned, dropped ones are skipped, so look at
    // the unread records in slices of up to cap and stop when the caller's buffer is full
    size_t w = 0;
    uint32_t f = h.popped;
    std::vector<int32_t> met;
    std::vector<OpvFrameRec> rec;
    std::vector<uint8_t> fr;
    while (f < nf && w < cap) {
        uint32_t n = nf - f;
        if (n > cap - w) n = (uint32_t)(cap - w);
        if (n > st.cap_frames) n = st.cap_frames;
        met.resize(n);
        rec.resize(n);
        fr.resize((size_t)n * OPV_FB);
        if (int r = ring_to_host(c, met.data(), st.metrics, f, n, st.cap_frames, sizeof(int32_t))) return r;
        if (int r = ring_to_host(c, rec.data(), st.frec, f, n, st.cap_frames, sizeof(OpvFrameRec))) return r;
        if (int r = ring_to_host(c, fr.data(), st.frames, f, n, st.cap_frames, OPV_FB)) return r;
        bool stop = false;
        for (uint32_t k = 0; k < n; ++k, ++f) {
            if (met[k] == INT32_MIN) { stop = true; break; }  // released but not decoded yet (cannot happen after opv_process)
            if (met[k] < 0) continue;                         // dropped silent frame (ref :859, :1052)
            if (out) std::memcpy(out + w * OPV_FB, fr.data() + (size_t)k * OPV_FB, OPV_FB);
            if (meta) {
                meta[w].viterbi_metric = met[k];
                meta[w].sync_ok = rec[k].sync_ok;
                meta[w].sync_quality = rec[k].quality;
                meta[w].release_symbol = rec[k].release_sym;
                meta[w].payload_symbol = rec[k].payload_sym;
            }
            ++h.decoded;
            if (met[k] == 0) ++h.perfect;
            ++w;
        }
        if (stop) break;
    }
    h.popped = f;
    return (long)w;
}

extern "C" long opv_pop_events(opv_ctx* c, int s, opv_event* out, size_t cap) {
    if (int r = check_stream(c, s)) return r;
    if (int r = c->refresh()) return r;
    const OpvStream& st = c->mirror[s];
    HostStream& h = c->hs[s];
    const uint32_t ne = st.n_events;
    if (ne - h.events_popped > st.cap_events) {  // lossy ring: the oldest unread entries have been overwritten
        h.events_dropped += (ne - h.events_popped) - st.cap_events;
        h.events_popped = ne - st.cap_events;
    }
    if (h.events_popped >= ne || cap == 0 || !out) return 0;
    uint32_t n = ne - h.events_popped;
    if (n > cap) n = (uint32_t)cap;
    static_assert(sizeof(opv_event) == sizeof(OpvEventRec), "event layouts must match");
    if (int r = ring_to_host(c, out, st.events, h.events_popped, n, st.cap_events, sizeof(OpvEventRec))) return r;
    h.events_popped += n;
    return (long)n;
}

extern "C" int opv_get_state(opv_ctx* c, int s, opv_stream_state* out) {
    if (int r = check_stream(c, s)) return r;
    if (!out) return fail(OPV_EINVAL, "null out");
    if (int r = c->refresh()) return r;
    const OpvStream& st = c->mirror[s];
    std::memset(out, 0, sizeof *out);
    out->freq_offset_hz = st.freq_offset;
    out->timing_freq = st.timing_freq;
    out->est_offset_hz = st.est_offset;
    out->mu = st.mu;
    out->total_symbols = st.n_soft;
    out->total_samples = st.total_samples;
    out->chunk_origin = st.origin + st.iq_base;  // absolute sample index
    out->sync_state = st.trk_state;
    out->frames_released = (int32_t)st.n_frames;
    out->n_chunks = (int32_t)st.n_chunks;
    out->flushed = st.tail_done;
    const HostStream& h = c->hs[s];
    out->frames_decoded = h.decoded;
    out->frames_perfect = h.perfect;
    out->events_dropped = h.events_dropped;
    if (st.n_events - h.events_popped > st.cap_events) out->events_dropped += (st.n_events - h.events_popped) - st.cap_events;
    out->edge_ties = st.edge_ties;
    out->offset_ties = (int32_t)st.est_ties;
    out->stalled = st.stalled;
    if (st.n_frames > h.popped) {  // released but not popped yet
        uint32_t n = st.n_frames - h.popped;
        if (n > st.cap_frames) n = st.cap_frames;
        std::vector<int32_t> met(n);
        if (int r = ring_to_host(c, met.data(), st.metrics, h.popped, n, st.cap_frames, sizeof(int32_t))) return r;
        for (int32_t m : met)
            if (m >= 0) { out->frames_decoded++; if (m == 0) out->frames_perfect++; }
    }
    return st.overflow ? fail(OPV_EINVAL, "opv_cfg.max_samples too large for the soft-symbol ring") : OPV_OK;
}

extern "C" int opv_device_frames(opv_ctx* c, const uint8_t** d_frames, const int32_t** d_metrics,
                                 const int32_t** d_counts, size_t* frame_capacity) {
    if (!c) return fail(OPV_EINVAL, "null context");
    if (d_frames) *d_frames = c->d_frames;
    if (d_metrics) *d_metrics = c->d_metrics;
    if (d_counts) *d_counts = c->d_counts;
    if (frame_capacity) *frame_capacity = c->cap_frames;
    return OPV_OK;
}

extern "C" void* opv_hip_stream(opv_ctx* c) { return c ? (void*)c->stream : nullptr; }

extern "C" long opv_tap_soft(opv_ctx* c, int s, uint64_t first, double* out, size_t cap) {
    if (int r = check_stream(c, s)) return r;
    if (int r = c->refresh()) return r;
    const OpvStream& st = c->mirror[s];
    if ((st.n_soft > st.cap_soft && first < st.n_soft - st.cap_soft) || (first < c->hs[s].soft_floor && first < st.n_soft))
        return fail(OPV_EINVAL, "soft symbols that old have been overwritten (the log is a ring)");
    if (first >= st.n_soft || cap == 0 || !out) return 0;
    uint64_t n = st.n_soft - first;
    if (n > cap) n = cap;
    if (int r = ring_copy(out, st.soft, ring_runs(first, n, st.cap_soft), sizeof(double), hipMemcpyDeviceToHost)) return r;
    return (long)n;
}

// Parity tap: `n` soft symbols appended to the stream's log exactly where its front-end would have written them (symbol i at
// soft[i & (cap_soft - 1)], n_soft advanced), in stream order behind the rounds launched so far. The next opv_process - the
// same launches as for pushed IQ, there is no second copy of them - runs the tracker, the scale pre-pass and the decoder over
// them. Room is the front-end's own rule (k_frontend.hip: soft_keep): nothing the tracker or a pending payload may still read
// is overwritten.
extern "C" int opv_tap_push_soft(opv_ctx* c, int s, const double* soft, size_t n) {
    if (int r = check_stream(c, s)) return r;
    if (!soft || n == 0) return fail(OPV_EINVAL, "opv_tap_push_soft: null pointer or no symbols");
    HostStream& h = c->hs[s];
    if (h.iq_seen || h.attached || h.n_avail) return fail(OPV_ESTATE, "opv_tap_push_soft: the stream has received IQ (reset it first)");
    if (h.eof) return fail(OPV_ESTATE, "opv_tap_push_soft: the stream has been flushed (reset it first)");
    if (int r = settle_pushes(c)) return r;
    if (int r = c->refresh()) return r;                    // (waits for the rounds in flight: the tracker's cursors are final)
    OpvStream& st = c->mirror[s];
    if (st.overflow) return fail(OPV_ESTATE, "opv_tap_push_soft: the stream is in an error state (opv_pop_frames reports it)");
    if (n > st.cap_soft || (st.n_soft - soft_keep(st)) + n > st.cap_soft)
        return fail(OPV_ECAPACITY, "opv_tap_push_soft: the soft-symbol ring has no room (unread symbols + this push do not fit; "
                                   "call opv_process / opv_pop_frames between pushes)");
    if (int r = ring_copy((void*)soft, st.soft, ring_runs(st.n_soft, n, st.cap_soft), sizeof(double), hipMemcpyHostToDevice, c->stream)) return r;
    st.n_soft += n;                                       // (the mirror stays valid: it is what the device holds after these copies)
    HIPCHK(hipMemcpyAsync(&c->d_streams[s].n_soft, &st.n_soft, sizeof st.n_soft, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));               // the symbols are the caller's again
    h.soft_tapped = true;
    h.tap_fresh += n;
    return OPV_OK;
}

extern "C" long opv_tap_chunks(opv_ctx* c, int s, uint32_t first, double* out5, size_t cap) {
    if (int r = check_stream(c, s)) return r;
    if (int r = c->refresh()) return r;
    const OpvStream& st = c->mirror[s];
    if (first >= st.n_chunks || cap == 0 || !out5) return 0;
    if (st.n_chunks - first > st.cap_chunks || first < c->hs[s].chunk_floor) return fail(OPV_EINVAL, "chunk log entries already overwritten (ring)");
    uint32_t n = st.n_chunks - first;
    if (n > cap) n = (uint32_t)cap;
    if (int r = ring_copy(out5, st.chunk_log, ring_runs(first, n, st.cap_chunks), 5 * sizeof(double), hipMemcpyDeviceToHost)) return r;
    return (long)n;
}

extern "C" int opv_tap_offset_energies(opv_ctx* c, int s, double* out134) {
    if (int r = check_stream(c, s)) return r;
    if (!out134) return fail(OPV_EINVAL, "null out");
    if (int r = c->refresh()) return r;
    std::memcpy(out134, c->mirror[s].energies, sizeof(double) * 134);
    return OPV_OK;
}

extern "C" int opv_offset_ties_on_host(opv_ctx* c) { return c && c->host_ties ? 1 : 0; }
extern "C" uint64_t opv_offset_ties_decided_on_host(opv_ctx* c) { return c ? c->tie.decided.load(std::memory_order_relaxed) : 0; }
extern "C" uint64_t opv_offset_ties_left_to_device(opv_ctx* c) { return c ? c->tie.left.load(std::memory_order_relaxed) : 0; }

extern "C" int opv_tap_wave_info(opv_ctx* c, int s, uint64_t out[4]) {
    if (int r = check_stream(c, s)) return r;
    if (!out) return fail(OPV_EINVAL, "null out");
    if (int r = c->refresh()) return r;
    const OpvStream& st = c->mirror[s];
    out[0] = st.dbg_hw_id; out[1] = st.dbg_xcc_id; out[2] = st.dbg_cycles; out[3] = st.dbg_ticks;
    return OPV_OK;
}

extern "C" int opv_tap_frontend_calls(opv_ctx* c, int s, uint64_t out[2]) {
    if (int r = check_stream(c, s)) return r;
    if (!out) return fail(OPV_EINVAL, "null out");
    if (int r = c->refresh()) return r;
    out[0] = c->mirror[s].fe_calls_free; out[1] = c->mirror[s].fe_calls_guarded;
    return OPV_OK;
}

extern "C" int opv_tap_occupancy(opv_ctx* c, int out[6]) {
    if (!c || !out) return fail(OPV_EINVAL, "null argument");
    HIPCHK(hipSetDevice(c->cfg.device));
    const FrontendKernel fe[4] = {FE_RB, FE_RB_WG4, FE_X16_WG4, FE_X4_WG4};       // (FE_RB: its 64-thread shape)
    for (int i = 0; i < 4; ++i)
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[i], kFrontend[fe[i]].fn, kFrontendShape[fe[i]].threads, fe[i] == FE_RB ? OPV_RB_LDS_I16 : 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[4], (const void*)k_frame_decode, 64, 0));
    HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out[5], (const void*)k_frame_scale, 64, 0));
    return OPV_OK;
}

extern "C" int opv_decode_payloads(opv_ctx* c, const double* soft, size_t n, uint8_t* out, int32_t* metrics,
                                   int8_t* q, int8_t* deint, uint8_t* bits) {
    if (!c || !soft || !out || !metrics) return fail(OPV_EINVAL, "null argument");
    if (n == 0) return OPV_OK;
    HIPCHK(hipSetDevice(c->cfg.device));
    double* d_soft = nullptr;
    uint8_t* d_out = nullptr;
    int32_t* d_met = nullptr;
    int8_t *d_q = nullptr, *d_d = nullptr;
    uint8_t* d_b = nullptr;
    double* d_scale = nullptr;
    int rc = OPV_OK;
    auto chk = [&](hipError_t e, const char* w) { if (e != hipSuccess && rc == OPV_OK) rc = fail(OPV_EHIP, w, e); };
    chk(hipMalloc(&d_soft, sizeof(double) * OPV_CODED * n), "hipMalloc soft");
    chk(hipMalloc(&d_out, (size_t)OPV_FB * n), "hipMalloc out");
    chk(hipMalloc(&d_met, sizeof(int32_t) * n), "hipMalloc metrics");
    chk(hipMalloc(&d_scale, sizeof(double) * n), "hipMalloc scales");
    if (q) chk(hipMalloc(&d_q, (size_t)OPV_CODED * n), "hipMalloc q");
    if (deint) chk(hipMalloc(&d_d, (size_t)OPV_CODED * n), "hipMalloc deint");
    if (bits) chk(hipMalloc(&d_b, (size_t)OPV_FBITS * n), "hipMalloc bits");
    if (rc == OPV_OK) {
        chk(hipMemcpyAsync(d_soft, soft, sizeof(double) * OPV_CODED * n, hipMemcpyHostToDevice, c->stream), "H2D soft");
        chk(hipMemsetAsync(d_out, 0, (size_t)OPV_FB * n, c->stream), "memset");
        k_payload_scale<<<(unsigned)((n + 63) / 64), 64, 0, c->stream>>>(d_soft, (uint32_t)n, d_scale);
        k_decode_payloads<<<(unsigned)((n + 1) / 2), 64, 0, c->stream>>>(d_soft, (uint32_t)n, d_scale, d_out, d_met, d_q, d_d, d_b);   // two payloads per wave
        chk(hipGetLastError(), "k_decode_payloads launch");
        chk(hipMemcpyAsync(out, d_out, (size_t)OPV_FB * n, hipMemcpyDeviceToHost, c->stream), "D2H out");
        chk(hipMemcpyAsync(metrics, d_met, sizeof(int32_t) * n, hipMemcpyDeviceToHost, c->stream), "D2H metrics");
        if (q) chk(hipMemcpyAsync(q, d_q, (size_t)OPV_CODED * n, hipMemcpyDeviceToHost, c->stream), "D2H q");
        if (deint) chk(hipMemcpyAsync(deint, d_d, (size_t)OPV_CODED * n, hipMemcpyDeviceToHost, c->stream), "D2H deint");
        if (bits) chk(hipMemcpyAsync(bits, d_b, (size_t)OPV_FBITS * n, hipMemcpyDeviceToHost, c->stream), "D2H bits");
        chk(hipStreamSynchronize(c->stream), "sync");
    }
    void* ptrs[] = {d_soft, d_out, d_met, d_q, d_d, d_b, d_scale};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    return rc;
}

