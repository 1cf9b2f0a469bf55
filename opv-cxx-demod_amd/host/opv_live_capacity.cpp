// opv_live_capacity.cpp — how many LIVE streams one GPU context serves in real time, measured the way the boundary's real caller
// uses it (reference `opv-modem -R`, src/opv-modem.cpp:673-838: IQ arrives at 2.168 MSPS, one frame = 86 720 samples = 40 ms).
//
// A serving round is what opv-rx-bridge does for every 40 ms of signal, for N streams at once: one 86 720-sample chunk per
// stream pushed from (pinned) host memory across PCIe (opv_push_iq_batch), one opv_process, every stream's frames popped
// (opv_pop_frames). The context keeps up with real time while a round takes less than the 40 ms of signal it consumes. This
// tool runs R rounds for a given N and prints the distribution of the round time as one JSON line; bench.py searches for the
// largest N whose p99 stays under 40 ms (extras.live_capacity). No kernel is specific to this tool: it is a caller of
// include/opv_demod.h like opv-rx-bridge, without sockets so that the number is the library's.
//
//   opv-live-capacity <n_streams> [rounds (120)] [warmup (6)] [device (0)] [--pipelined | --wideband K] [--format cs16|cs8|cu8|cf32]
//     --format F    (anywhere on the line) the same signal as a radio of format F would deliver it: quantised on the host, before the
//                   timed rounds, by the inverse of opv_iq_convert, and pushed typed (opv_push_iq_batch_fmt(_async), opv_wb_push_fmt_async):
//                   cs8 / cu8 cross PCIe at half the bytes of int16, cf32 at twice, and are widened on the device. The line
//                   printed then carries "format" and pcie_GBps counts the bytes of that format. Without it: the int16 calls.
//     --pipelined   the double-buffered server: opv_push_iq_batch_async of round r + 1 is enqueued right behind opv_process of
//                   round r, so the chunks of the next round cross PCIe while this round's kernels run and its frames are
//                   popped; a round then costs max(PCIe, kernels + pops). Reported per round: the time from one opv_push_wait
//                   to the next (steady-state period); a chunk's frames surface one round later than in the serial loop.
//
//     --wideband K  the same pipelined rounds and the same p99 criterion with the streams fed K per pinned WIDE capture through the
//                   wideband front door (opv_wb_push_async, D = 1): n_streams / K captures of 86 720 wide samples cross PCIe per
//                   round - a K-th of the bytes - and one k_wb_ddc launch per capture fills its K streams. Channel k of a capture
//                   sits at (k - (K - 1) / 2) x 100 kHz (K <= 21 fit +/-1.084 MHz) at a K-th of full scale; the bank's taps are a
//                   161-tap Hamming-windowed sinc, cut-off 50 kHz, its gain restores the amplitude to within a factor of two. n_streams must be a
//                   multiple of K. Capture g starts g frames into the wide run, so every capture lies at its own host addresses.
//
// The signal is ONE clean BERT run of N + rounds + warmup + 1 frames (the device transmit chain, bit-identical to `opv-mod -S W5NYV
// -B ...`, brought back into pinned host memory); stream k listens to it from frame k on. So in every round every stream's
// chunk lies at its own host addresses - N x 347 KB of distinct pinned memory cross PCIe per round, nothing a device cache
// could serve twice (with one shared chunk the gather kernel "moved" 1.8 TB/s: L2 hits) - and every stream decodes its own
// frame sequence. Checked: after the first round every round releases exactly one frame per stream, equal to the transmitted one.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cmath>
#include <cstring>
#include <vector>

#include <hip/hip_runtime_api.h>   // pinned host memory for the chunks (what a DMA-fed SDR server would hold them in)

#include "../../include/opv_demod.h"

int main(int argc, char** argv) {
    if (argc < 2) {
        fprintf(stderr, "Usage: %s <n_streams> [rounds] [warmup] [device]\n", argv[0]);
        return 2;
    }
    int fmt = -1;                                       // --format F: taken out of the line first; what follows parses as it always did
    for (int i = 1; i + 1 < argc; ++i)
        if (!strcmp(argv[i], "--format")) {
            const char* names[] = {"cs16", "cs8", "cu8", "cf32"};
            for (int f = 0; f < 4; ++f)
                if (!strcmp(argv[i + 1], names[f])) fmt = f;
            if (fmt < 0) { fprintf(stderr, "opv-live-capacity: --format takes cs16, cs8, cu8 or cf32\n"); return 2; }
            for (int j = i; j + 2 < argc; ++j) argv[j] = argv[j + 2];
            argc -= 2;
            break;
        }
    const bool typed = fmt > OPV_IQ_CS16;
    const size_t bps = typed ? opv_iq_sample_bytes(fmt) : 4;
    // n int16 samples as a radio of the format would have delivered them, in pinned memory (the inverse of opv_iq_convert's rule)
    auto quantised = [&](const int16_t* src, size_t n) -> unsigned char* {
        unsigned char* q = nullptr;
        if (hipHostMalloc((void**)&q, n * bps, hipHostMallocDefault) != hipSuccess) return nullptr;
        for (size_t i = 0; i < 2 * n; ++i) {
            const double v = src[i];
            if (fmt == OPV_IQ_CS8) ((int8_t*)q)[i] = (int8_t)std::min(127l, std::max(-128l, lrint(v / 256.0)));
            else if (fmt == OPV_IQ_CU8) q[i] = (uint8_t)std::min(255l, std::max(0l, lrint((v / 128.0 + 255.0) / 2.0)));
            else ((float*)q)[i] = (float)(v / 32767.0);
        }
        return q;
    };
    bool pipelined = false;
    int K = 0;                                          // --wideband K: streams per wide capture (0: one block per stream)
    if (argc > 2 && !strcmp(argv[argc - 1], "--pipelined")) { pipelined = true; --argc; }
    else if (argc > 3 && !strcmp(argv[argc - 2], "--wideband")) { K = atoi(argv[argc - 1]); pipelined = true; argc -= 2; if (K < 1 || K > 21) { fprintf(stderr, "opv-live-capacity: --wideband takes 1..21\n"); return 2; } }
    const int N = atoi(argv[1]);
    const int rounds = argc > 2 ? atoi(argv[2]) : 120, warm = argc > 3 ? atoi(argv[3]) : 6, device = argc > 4 ? atoi(argv[4]) : 0;
    if (N < 1 || rounds < 1 || warm < 1 || (K && N % K)) { fprintf(stderr, "opv-live-capacity: bad arguments\n"); return 2; }
    const int G = K ? N / K : 0;                        // wide captures per round
    const int total = rounds + warm;
    const size_t chunk = OPV_CHUNK_SAMPLES;

    // the signal: N + total + 1 frames (+ the modulator's 100 silent symbols), in pinned memory
    const size_t n_frames = (K ? (size_t)K + (size_t)G : (size_t)N) + (size_t)total + 1;
    std::vector<uint8_t> frames(n_frames * OPV_FRAME_BYTES);
    opv_tx_bert_frames("W5NYV", 0xBBAADD, 0, n_frames, frames.data());
    const size_t n_all = opv_tx_modulated_samples(n_frames);
    int16_t* iq = nullptr;
    if (hipSetDevice(device) != hipSuccess || hipHostMalloc((void**)&iq, n_all * 4, hipHostMallocDefault) != hipSuccess) {
        fprintf(stderr, "opv-live-capacity: no pinned host memory / no HIP device\n");
        return 2;
    }

    opv_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.streaming = 1;
    cfg.afc_alpha = 0.001;
    cfg.device = device;
    cfg.pll_bw_hz = 50.0;
    cfg.max_samples = 4 * chunk + 65536;               // a live server's staging buffer: a few chunks per stream
    opv_ctx* ctx = nullptr;
    if (opv_create(&ctx, N, &cfg) < 0) { fprintf(stderr, "opv-live-capacity: %s\n", opv_last_error()); return 2; }
    if (opv_tx_modulate_device_to_host(ctx, frames.data(), n_frames, iq) < 0) { fprintf(stderr, "opv-live-capacity: %s\n", opv_last_error()); return 2; }

    // --wideband: the wide run W[n] = sum_k base[n + k chunk] / K x exp(j 2 pi f_k n / Fs) in pinned memory; capture g of round r
    // is W[(r + g) chunk, + chunk), so stream g K + k listens to the base run from frame g + k on
    int16_t* wide = nullptr;
    std::vector<opv_wb*> wbs;
    if (K) {
        const size_t n_w = ((size_t)G + (size_t)total) * chunk;
        if (hipHostMalloc((void**)&wide, n_w * 4, hipHostMallocDefault) != hipSuccess) { fprintf(stderr, "opv-live-capacity: no pinned host memory\n"); return 2; }
        std::vector<double> ct(4096), sn(4096), acc(2 * n_w, 0.0);
        for (int i = 0; i < 4096; ++i) { ct[i] = cos(2 * M_PI * i / 4096.0) / K; sn[i] = sin(2 * M_PI * i / 4096.0) / K; }
        std::vector<double> centre(K);
        for (int k = 0; k < K; ++k) {
            centre[k] = (k - (K - 1) / 2.0) * 100000.0;
            const uint32_t inc = (uint32_t)(int64_t)llrint(centre[k] / 2168000.0 * 4294967296.0);
            const int16_t* b = iq + 2 * (size_t)k * chunk;
            uint32_t ph = 0;
            for (size_t n = 0; n < n_w; ++n, ph += inc) {
                const double c = ct[ph >> 20], s_ = sn[ph >> 20];
                acc[2 * n] += b[2 * n] * c - b[2 * n + 1] * s_;
                acc[2 * n + 1] += b[2 * n] * s_ + b[2 * n + 1] * c;
            }
        }
        for (size_t i = 0; i < 2 * n_w; ++i) wide[i] = (int16_t)lrint(acc[i]);
        constexpr int L = 161;                           // delay (L - 1) / 2 = 80 samples = two whole symbols: the streams' timing loops start on a symbol boundary
        int16_t taps[L];
        double h[L], sum = 0;
        for (int t = 0; t < L; ++t) {
            const double x = 2.0 * 50000.0 / 2168000.0 * (t - (L - 1) / 2.0);
            h[t] = (x == 0 ? 1.0 : sin(M_PI * x) / (M_PI * x)) * (0.54 - 0.46 * cos(2 * M_PI * t / (L - 1.0)));
            sum += h[t];
        }
        for (int t = 0; t < L; ++t) taps[t] = (int16_t)lrint(h[t] / sum * 32768.0);
        int shift = 30;                                  // unity gain (taps sum 2^15, LO 2^15); less by log2 K, rounded down
        for (int k = K; k > 1; k >>= 1) --shift;
        std::vector<int> sid(K);
        for (int g = 0; g < G; ++g) {
            opv_wb_cfg wc;
            memset(&wc, 0, sizeof wc);
            wc.decim = 1; wc.n_channels = K; wc.n_taps = L; wc.out_shift = shift; wc.first_sample = (uint64_t)g * chunk;
            for (int k = 0; k < K; ++k) sid[k] = g * K + k;
            opv_wb* w = nullptr;
            if (opv_wb_create(&w, ctx, &wc, sid.data(), centre.data(), taps) < 0) { fprintf(stderr, "opv-live-capacity: %s\n", opv_last_error()); return 2; }
            wbs.push_back(w);
        }
    }
    unsigned char* tq = nullptr;                        // --format: what is pushed instead of iq / wide
    if (typed && !(tq = quantised(K ? wide : iq, K ? ((size_t)G + (size_t)total) * chunk : n_all))) { fprintf(stderr, "opv-live-capacity: no pinned host memory\n"); return 2; }
    std::vector<const void*> tptrs(N);
    std::vector<int> ids(N);
    std::vector<const int16_t*> ptrs(N);
    std::vector<size_t> lens(N, chunk);
    for (int k = 0; k < N; ++k) ids[k] = k;
    std::vector<double> t_round, t_push, t_proc, t_pop, t_launch, t_enq;
    uint8_t out[4 * OPV_FRAME_BYTES];
    opv_frame_meta meta[4];
    long released = 0, wrong = 0, imperfect = 0, uneven = 0;
    std::vector<size_t> next(N, 0);                     // per stream: the number of the next frame it owes
    using clk = std::chrono::steady_clock;
    auto ms = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    auto set_ptrs = [&](int r) {                        // stream k is k frames into the run
        for (int k = 0; k < N; ++k) {
            ptrs[k] = iq + 2 * ((size_t)r + (size_t)k) * chunk;
            if (typed) tptrs[k] = tq + bps * ((size_t)r + (size_t)k) * chunk;
        }
    };
    auto push_async = [&](int r) -> int {               // round r's samples, enqueued: one block per stream, or one wide capture per K streams
        if (!K) {
            set_ptrs(r);
            return typed ? opv_push_iq_batch_fmt_async(ctx, fmt, N, ids.data(), tptrs.data(), lens.data()) : opv_push_iq_batch_async(ctx, N, ids.data(), ptrs.data(), lens.data());
        }
        for (int g = 0; g < G; ++g)
            if (int rc = typed ? opv_wb_push_fmt_async(wbs[g], fmt, tq + bps * ((size_t)r + (size_t)g) * chunk, chunk)
                               : opv_wb_push_async(wbs[g], wide + 2 * ((size_t)r + (size_t)g) * chunk, chunk)) return rc;
        return 0;
    };
    if (pipelined) {
        if (push_async(0) < 0) { fprintf(stderr, "push: %s\n", opv_last_error()); return 2; }
    }
    for (int r = 0; r < total; ++r) {
        const auto t0 = clk::now();
        if (pipelined) {
            if (opv_push_wait(ctx) < 0) { fprintf(stderr, "push wait: %s\n", opv_last_error()); return 2; }   // round r's chunks have landed
        } else {
            set_ptrs(r);
            if ((typed ? opv_push_iq_batch_fmt(ctx, fmt, N, ids.data(), tptrs.data(), lens.data()) : opv_push_iq_batch(ctx, N, ids.data(), ptrs.data(), lens.data())) < 0) { fprintf(stderr, "push: %s\n", opv_last_error()); return 2; }
        }
        const auto t1 = clk::now();
        if (opv_process(ctx) < 0) { fprintf(stderr, "process: %s\n", opv_last_error()); return 2; }
        const auto t1a = clk::now();
        if (pipelined && r + 1 < total) {                 // round r + 1 starts crossing PCIe behind round r's launches
            if (push_async(r + 1) < 0) { fprintf(stderr, "push: %s\n", opv_last_error()); return 2; }
        }
        const auto t1b = clk::now();
        if (opv_sync(ctx) < 0) { fprintf(stderr, "process: %s\n", opv_last_error()); return 2; }
        const auto t2 = clk::now();
        long got_round = 0;
        for (int k = 0; k < N; ++k) {
            const long g = opv_pop_frames(ctx, k, out, 4, meta);
            if (g < 0) { fprintf(stderr, "pop: %s\n", opv_last_error()); return 2; }
            for (long f = 0; f < g; ++f) {
                const size_t idx = (K ? (size_t)(k / K + k % K) : (size_t)k) + next[k]++;
                if (idx >= n_frames || memcmp(out + f * OPV_FRAME_BYTES, frames.data() + idx * OPV_FRAME_BYTES, OPV_FRAME_BYTES) != 0) ++wrong;
                if (meta[f].viterbi_metric != 0) ++imperfect;
            }
            got_round += g;
        }
        const auto t3 = clk::now();
        if (r >= 1 && got_round != N) ++uneven;         // (one frame per stream and round once the first chunk is in: the steady state)
        released += got_round;
        if (r >= warm) {
            t_round.push_back(ms(t0, t3));
            t_push.push_back(ms(t0, t1));
            t_proc.push_back(ms(t1, t2));
            t_pop.push_back(ms(t2, t3));
            t_launch.push_back(ms(t1, t1a));
            t_enq.push_back(ms(t1a, t1b));
        }
    }
    auto pct = [](std::vector<double> v, double p) {
        std::sort(v.begin(), v.end());
        const size_t i = (size_t)(p * (double)(v.size() - 1) + 0.5);
        return v[i < v.size() ? i : v.size() - 1];
    };
    const char* fmt_names[] = {"cs16", "cs8", "cu8", "cf32"};
    if (fmt >= 0) printf("{\"format\": \"%s\", ", fmt_names[fmt]);
    else printf("{");
    printf("\"streams\": %d, \"wideband\": %d, \"pipelined\": %s, \"rounds\": %d, \"signal_ms_per_round\": 40.0, \"round_ms_p50\": %.3f, \"round_ms_p99\": %.3f, \"round_ms_max\": %.3f, "
           "\"push_ms_p50\": %.3f, \"process_ms_p50\": %.3f, \"pop_ms_p50\": %.3f, \"pcie_GBps_p50\": %.2f, \"frames_released\": %ld, "
           "\"frames_wrong\": %ld, \"frames_imperfect\": %ld, \"rounds_not_one_frame_per_stream\": %ld, \"process_call_ms_p50\": %.3f, \"async_enqueue_ms_p50\": %.3f}\n",
           N, K, pipelined ? "true" : "false", rounds, pct(t_round, 0.5), pct(t_round, 0.99), pct(t_round, 1.0), pct(t_push, 0.5), pct(t_proc, 0.5), pct(t_pop, 0.5),
           // serial: the moves alone; pipelined: push_ms is only the wait for moves that ran beside the previous round - the rate over the period
           (double)(K ? G : N) * chunk * bps / (pct(pipelined ? t_round : t_push, 0.5) * 1e-3) / 1e9, released, wrong, imperfect, uneven, pct(t_launch, 0.5), pct(t_enq, 0.5));
    for (opv_wb* w : wbs) opv_wb_destroy(w);
    opv_destroy(ctx);
    if (tq) (void)hipHostFree(tq);
    if (wide) (void)hipHostFree(wide);
    (void)hipHostFree(iq);
    return wrong ? 1 : 0;
}
