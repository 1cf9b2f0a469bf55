/* include/opv_demod.h — C ABI of the MI355X-native OPV MSK receive chain.
 *
 * This is the drop-in boundary. The reference (OpenResearchInstitute/opv-cxx-demod) has no
 * library/plugin API: its hot path sits behind three C++ objects that only main() uses
 * (src/opv-demod.cpp:999-1001, :1164, :1182-1183) and behind the `opv-demod` process
 * contract. Each entry point below names the reference interface it replaces. All state
 * lives in device memory owned by an opv_ctx; signatures carry plain pointers and sizes
 * only. A context is not thread-safe; distinct contexts are independent.
 *
 * Return convention: 0 on success, negative OPV_E* on error (never a silent CPU fallback:
 * if no HIP device / kernel image is usable, opv_create fails with OPV_ENODEV).
 */
#ifndef OPV_DEMOD_H
#define OPV_DEMOD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPV_ABI_VERSION 7   /* (still 7, additive: + OPV_IQ_*, opv_push_iq_fmt / opv_push_iq_batch_fmt(_async) / opv_wb_push_fmt(_async) / opv_scan_push_fmt / opv_convert_iq_device / opv_iq_convert / opv_iq_sample_bytes (typed IQ pushes: cs8, cu8 and cf32 converted on the device);
                               still 7, additive: + opv_wb_seg_phase / opv_wb_seg_next / opv_wb_retune / opv_wb_segments / opv_wbtx_retune / opv_wbtx_segments (per-channel retune and Doppler ramps: an LO schedule per channel of the four wideband converters);
                               still 7, additive: + opv_scan_* (wideband scan: an exact probe bank on a wide capture, and the carriers in a row of its powers);
                               still 7, additive: + opv_div_* (receive diversity: the soft symbols of several streams combined per frame);
                               still 7, additive: + opv_wbtxr_plan / opv_wbtxr_outputs / opv_wbtx_create_rational (wideband transmit at any radio rate: an exact rational up-converter bank);
                               still 7, additive: + opv_wbr_plan/ opv_wbr_outputs / opv_wb_create_rational (the wideband front door at any radio rate: an exact rational resampler bank);
                               still 7, additive: + opv_wbtx_* (wideband transmit: an exact integer up-converter bank, K channels to one wide capture);
                               still 7, additive: + opv_txb_* (the transmit bank: N live modulators on the device, state carried from round to round), opv_tap_txb_patch;
                               still 7, additive: + opv_link, opv_enable_link_report / opv_pop_frames_link / opv_device_link / opv_link_payloads, the per-frame link report;
                               still 7, additive: + opv_tap_push_soft, a parity tap that stages soft symbols for the tracker and the in-context decoder;
                               still 7, additive: + opv_wb_* (the wideband front door: an exact integer DDC bank feeding a context's streams), opv_tap_iq;
                               still 7, additive: + opv_export_size / opv_export_streams / opv_import_streams / opv_blob_streams, stream migration)
                               7: opv_process never waits on the host again - the host-libm decision of offset-search near-ties runs as a host
                               function IN STREAM ORDER between the search and the front-end (+ opv_offset_ties_decided_on_host, opv_offset_ties_left_to_device); opv_set_frontend
                               takes 0 / 1 / 4 / 16 only (the comparison mappings are gone); opv_tap_occupancy's third entry is k_msk_frontend_x16_wg4;
                               6: offset-search near-ties are decided with the HOST's libm (opv_offset_ties_on_host), one host wait in the round
                               in which a stream's search runs; + opv_push_iq_batch_async / opv_push_wait; opv_push_iq_batch moves blocks in
                               pinned host memory with one gather kernel;
                               5: opv_set_frontend takes 16 (sixteen streams per wavefront; automatic from 8193 streams) and answers OPV_EINVAL to
                               the comparison mappings -1 / -2 unless built with them; opv_create refuses non-finite -o / -a / -p values;
                               an idle opv_process launches nothing for callers that never pop (zero-copy path);
                               4: + opv_tx_stream_* (the host modulator with its state carried from call to call), opv_tap_tx_frame;
                               3: + opv_frontend_kernel, opv_tx_bert_frames, opv_tx_modulate_device_to_host, opv_tap_tx_checkpoints,
                               opv_comm_* / opv_gather_frames(_all); opv_tx_modulate_device runs the whole chain on the device;
                               an opv_process with nothing new still resumes streams held back by back-pressure */

#define OPV_SAMPLES_PER_SYMBOL 40    /* src/opv-demod.cpp:39  */
#define OPV_FRAME_BYTES 134          /* :49  */
#define OPV_FRAME_BITS 1072          /* :50  */
#define OPV_ENCODED_BITS 2144        /* :51  */
#define OPV_FRAME_SYMBOLS 2168       /* :52  */
#define OPV_CHUNK_SAMPLES 86720      /* :1012 streaming chunk = one frame of samples */

enum {
    OPV_OK = 0,
    OPV_EINVAL = -1,   /* bad argument                                   */
    OPV_ENODEV = -2,   /* no usable HIP device / kernels failed to load  */
    OPV_ENOMEM = -3,   /* device or host allocation failed               */
    OPV_ECAPACITY = -4,/* per-stream capacity (opv_cfg.max_samples) exceeded: unprocessed samples + a push do not fit
                          (frames waiting to be popped hold their stream back; pop them and push again) */
    OPV_EHIP = -5,     /* a HIP runtime call failed (see opv_last_error) */
    OPV_ESTATE = -6    /* call not valid in this state (e.g. push after flush) */
};

/* Sync tracker states (enum class SyncState, src/opv-demod.cpp:73). */
enum { OPV_HUNTING = 0, OPV_VERIFYING = 1, OPV_LOCKED = 2 };

/* One entry per stderr line SyncTracker::process prints (src/opv-demod.cpp:651,677,695,699,705). */
enum {
    OPV_EV_HUNT_TO_VERIFY = 1,
    OPV_EV_VERIFY_TO_LOCK = 2,
    OPV_EV_SYNC_OK = 3,
    OPV_EV_SYNC_MISS = 4,
    OPV_EV_LOST_LOCK = 5
};

/* Replaces the flag parsing of main() (src/opv-demod.cpp:944-974) for the flags that reach
 * the hot path: -s, -o <hz>, -a <alpha>, and -c / -p <hz> (the batch coherent demodulator :365-572, prefix parity
 * only - its loop is chaotic); -q/-r only affect host printing. */
typedef struct opv_cfg {
    int32_t streaming;        /* 1: -s chunked semantics (:995-1125); 0: batch (:1132-1216) */
    int32_t have_init_offset; /* -o given: skip the offset search in streaming mode (:1004,:1031) */
    double init_offset_hz;    /* -o value */
    double afc_alpha;         /* -a value; 0.001 if <= 0 is NOT substituted: pass 0.001 for the default (:945) */
    int32_t device;           /* HIP device ordinal */
    int32_t coherent;         /* -c: Costas-loop demodulator instead of the energy detector; honoured in batch mode only,
                                 like the reference (:1144; with -s it merely changes the banner, :983-984,995) */
    uint64_t max_samples;     /* per-stream DEVICE BUFFER capacity in IQ samples (< 2^31). Pushed streams may be
                                 arbitrarily long: consumed samples / soft symbols are dropped when the buffer
                                 fills (>= ~3 chunks + the largest push is enough); an attached capture must fit */
    double pll_bw_hz;         /* -p value (coherent mode, set_pll_bandwidth :551-558); the reference's default is 50 */
} opv_cfg;

/* Per decoded frame: what main() knows when it prints/writes a frame
 * (src/opv-demod.cpp:1048-1062: metric, res.sync_quality, sym index of release). The two symbol indices are absolute and
 * 64-bit (see "Long-lived streams" at opv_stream_state). */
typedef struct opv_frame_meta {
    int32_t viterbi_metric;   /* ViterbiDecoder::decode return (:845); 0 == "perfect" (:910) */
    int32_t sync_ok;          /* 1: the sync word in front of this payload passed its check (HUNTING hit :642, or
                                 LOCKED corr >= 0.70 :688); 0: flywheel frame released after a sync MISS (:709-712) */
    double sync_quality;      /* SyncTracker::Result::sync_quality (:611) */
    uint64_t release_symbol;  /* global symbol index at which the frame was released (:1046) */
    uint64_t payload_symbol;  /* global symbol index of the first payload symbol */
} opv_frame_meta;

typedef struct opv_event {
    int32_t kind;             /* OPV_EV_* */
    int32_t count;            /* frame number (VERIFY_TO_LOCK) or miss number (SYNC_MISS) */
    uint64_t sym_idx;         /* the [%zu] printed by the reference */
    double corr;              /* normalised correlation */
    double raw;               /* raw correlation (HUNT_TO_VERIFY line) */
} opv_event;

/* What the status / summary lines of main() read (src/opv-demod.cpp:1080-1082,1117-1120).
 *
 * Long-lived streams. Every SYMBOL index (total_symbols; opv_frame_meta.release_symbol / payload_symbol; opv_event.sym_idx;
 * the `first` of opv_tap_soft) and every SAMPLE index (total_samples, chunk_origin, the `first` of opv_tap_iq) is absolute and
 * 64-bit. At 2 168 000 S/s the sample count passes 2^31 after 16.5 minutes and 2^32 after 33, the symbol count after 11 and 22
 * hours; across both, and beyond 2^40, a stream is held to the oracle on every stream-to-wave mapping, with the boundary inside a
 * demodulate() call, a payload, the tracker's 24-symbol window (LOCKED and HUNTING), a flywheel frame, a silence gap and a
 * compaction (tests/test_gpu_far_positions.py). The frame, event and chunk COUNTS (frames_released, frames_decoded,
 * frames_perfect, n_chunks, events_dropped, and the cursors behind opv_pop_frames / opv_pop_events / opv_tap_chunks) are 32-bit:
 * at one frame and one demodulate() call per 40 ms, 2^31 is reached after 2.7 years of uninterrupted reception (a LOCKED stream
 * logs one event per frame: the same); no test takes a stream across their wrap. */
typedef struct opv_stream_state {
    double freq_offset_hz;    /* MSKDemodulatorAFC::get_freq_offset (:331) */
    double timing_freq;       /* get_timing_freq (:332) */
    double est_offset_hz;     /* estimate_offset result (:1032/:1166); NaN if it did not run */
    double mu;                /* fractional timing carry (:343) */
    uint64_t total_symbols;   /* symbols demodulated so far */
    uint64_t total_samples;   /* samples consumed by completed demodulate() calls (:1027) */
    uint64_t chunk_origin;    /* sample index at which the next chunk starts */
    int32_t sync_state;       /* OPV_HUNTING / VERIFYING / LOCKED (:738) */
    int32_t frames_released;  /* SyncTracker::get_total_frames (:739) */
    int32_t frames_decoded;   /* frames with metric >= 0 (`decoded`, :1053) */
    int32_t frames_perfect;   /* metric == 0 (`perfect`, :1054) */
    int32_t n_chunks;         /* demodulate() calls made */
    int32_t flushed;
    uint32_t events_dropped;  /* tracker events overwritten before opv_pop_events read them (the event log is lossy) */
    uint32_t edge_ties;       /* symbols whose tone choice the reference decides by the rounding of its own LO: a window
                                 with exactly one non-zero tap next to digital silence. Each may move the AFC by one
                                 step (<= 27 Hz, decaying) away from the reference; 0 on any capture without exact zeros */
    int32_t stalled;          /* back-pressure after the last opv_process: bit 0 = soft-symbol ring full, bit 1 = ring of
                                 unpopped frames full. The stream resumes at the next opv_process after opv_pop_frames */
    int32_t offset_ties;      /* offset-search candidates that were within 1e-11 (relative energy) of the winner and were
                                 therefore re-evaluated in the reference's own order of operations (estimate_offset :143-159): on
                                 the device, and once more on the host with the host's sin / cos (the reference's libm) if two of
                                 them are then still within 2e-13 of each other and opv_offset_ties_on_host() is 1. Both bands are
                                 scaled by the input's power where the correlation is weak against it (csrc/k_offset_search.hip) */
} opv_stream_state;

typedef struct opv_ctx opv_ctx;

/* ---- lifetime: replaces constructing MSKDemodulatorAFC + SyncTracker + FrameDecoder
 *      (src/opv-demod.cpp:999-1001 / :1164,:1182-1183) for n_streams independent captures */
int opv_create(opv_ctx** out, int n_streams, const opv_cfg* cfg);
/* Environment variables. The library reads SEVEN, all of them TEST HOOKS - never set in production -, all of them in opv_create
 * and nowhere else (a context's behaviour is fixed when it is created; grep getenv csrc/):
 *   OPV_OFFSET_DISTRUST_LIBM  (any value) the offset search's last-place ties are decided by the device's sincos although the host's
 *                             libm reproduces the reference's (opv_offset_ties_on_host() == 0): moves a stream whose search ties
 *                             from the class "decided like the reference" to "decided by another libm". The fallback's tests use it.
 *   OPV_TX_DISTRUST_LIBM      (any value) the device transmit chain takes every symbol's flat-top bits from the host's libm instead of
 *                             the zone rule its one-time probe of sin / cos allows: same samples, slower set-up. The fallback's test uses it.
 *   OPV_PUSH_NO_GATHER        (any value) opv_push_iq_batch(_async) moves pinned blocks with one copy per block instead of one gather
 *                             kernel: same bytes, the path pageable sources take anyway. Its test runs both. A typed batch
 *                             (opv_push_iq_batch_fmt) then sends every block through the context's device stage.
 *   OPV_PUSH_GATHER_BLOCKS    (a number > 0) workgroups of that gather kernel (default 32; a measurement knob, results unaffected).
 *   OPV_FRONTEND_INT16_RING   (any value) k_msk_frontend_rb keeps its int16 sample ring at every stream count, instead of the fp64 ring
 *                             a helper wave fills while the context has no more streams than the device has CUs: same results
 *                             bit for bit, slower. Its parity test runs both.
 *   OPV_FRONTEND_TF_GUARD     (a number != 0) k_msk_frontend_rb / _rb_wg4 keep the timing loop's clamp in every demodulate() call, instead
 *                             of dropping it in calls that provably cannot reach it (csrc/opv_tf_rule.h): same results bit for bit.
 *                             tests/test_gpu_trip8_tf_proof.py runs both.
 *   OPV_TEST_TIMING_FREQ0     (a double, strtod: hex floats welcome) the timing_freq every stream starts from at creation and reset,
 *                             0 otherwise like the reference's. Nothing else puts a stream near the +/-0.1 clamp: with the reference's
 *                             loop gains timing_freq moves by about 2e-4 per call whatever the input. */
void opv_destroy(opv_ctx* ctx);
const char* opv_last_error(void);
int opv_abi_version(void);

/* ---- host-buffer path -----------------------------------------------------------------
 * opv_push_iq replaces the stdin reader + chunker (src/opv-demod.cpp:1021-1026 streaming,
 * :1132-1135 batch): host-endian interleaved int16 I,Q. The caller keeps ownership; the
 * samples are copied to the stream's device buffer. Nothing is computed until opv_process. */
int opv_push_iq(opv_ctx* ctx, int stream, const int16_t* iq_interleaved, size_t n_samples);
/* The same for several streams of a multi-stream server in one call (what N copies of the reader loop
 * :1021-1026 do in N reference processes): all copies are enqueued, then awaited once. Stops at the first
 * error; streams before it have been pushed.
 * Blocks that lie in PINNED host memory (hipHostMalloc / hipHostRegister; 4-byte aligned) cross PCIe together, read by one
 * gather kernel through their device-visible addresses - 55 GB/s for 1536 blocks of 347 KB where one copy per stream reaches 21
 * (scripts/microbench/h2d_many.hip) - and staging buffers that fill in the same round are compacted by one launch; pageable
 * blocks take one hipMemcpyAsync each, as opv_push_iq does. Results do not depend on the route. */
int opv_push_iq_batch(opv_ctx* ctx, int count, const int* streams, const int16_t* const* iq_interleaved,
                      const size_t* n_samples);
/* The same without the wait at its end, for a server that double-buffers its host memory: returns once the moves are ENQUEUED; the
 * blocks must stay valid and unchanged until opv_push_wait returns (every other opv_push_* call and opv_reset_stream wait first
 * by themselves). opv_process may be called in between - its kernels queue behind every move enqueued so far, on the device - so
 * that round r + 1 crosses PCIe while the kernels of round r run and the frames of round r are popped:
 *     opv_push_iq_batch_async(r = 0);  loop: opv_push_wait; opv_process; opv_push_iq_batch_async(r + 1); opv_sync; opv_pop_frames...
 * A serving round then costs max(PCIe, kernels + pops) instead of their sum (bin/opv-live-capacity --pipelined). */
int opv_push_iq_batch_async(opv_ctx* ctx, int count, const int* streams, const int16_t* const* iq_interleaved,
                            const size_t* n_samples);
int opv_push_wait(opv_ctx* ctx);
/* ---- wideband front door: ONE wide capture in, K of a context's streams fed ------------------------------------------------
 * Replaces nothing in the reference, which starts at one channel's baseband. A radio delivers one wideband capture with many OPV
 * channels side by side; an opv_wb object is a bank of K digital down-converters on the device, so that the capture crosses PCIe
 * once and each channel arrives in its stream's device buffer as if it had been pushed with opv_push_iq. The arithmetic is
 * integer-exact and independent of summation order (tests/test_gpu_wideband.py holds the device to the numpy int64 model of tests/wideband_models.py with ==):
 *   wide samples x[n] = (I, Q) int16 at decim x 2 168 000 S/s, n = 0 at the first sample pushed into the object, a = first_sample + n;
 *   per channel k: inc_k = (uint32) llrint(centre_hz[k] / (decim x 2 168 000) x 2^32) (modulo 2^32: negative centres wrap),
 *     phi = (uint32)(a x inc_k) (a closed form: no accumulator is carried), i = phi >> 20, c = T[i], s = T[(i - 1024) & 4095] with
 *     T[i] = (int16) lrint(32767 cos(2 pi i / 4096)) (opv_wb_lo_table); the channel at +centre_hz comes down to 0:
 *     mr = I c + Q s, mi = Q c - I s (int32); acc[r] = sum_t taps[t] m[r decim - t], m[n] = 0 for n < 0, for r = 0 .. ceil(N / decim) - 1
 *     after N wide samples in all; output per component clamp(floor((acc + 2^(out_shift - 1)) / 2^out_shift), -32768, 32767) (out_shift = 0: no rounding term).
 *   Limits (anything else is OPV_EINVAL from opv_wb_plan / opv_wb_create): 1 <= decim <= 16, 1 <= n_taps <= 1024, 1 <= n_channels <= 256,
 *     0 <= out_shift <= 40, sum |taps| <= 2^21 (so |acc| < 2^52: exact in int64 and in fp64 alike), finite centres.
 * The only state between pushes is the last n_taps - 1 wide samples and the count N: any split of a capture into pushes gives the
 * bytes of one push. The object does NOT migrate (opv_export_streams moves its streams like any others): rebuild it at the
 * destination with first_sample + N as its first_sample - and mind that its n = 0 then starts with an empty filter history.
 * opv_wb_plan (host only, no device): validates cfg, centres and taps and writes the K increments. opv_wb_lo_table, opv_wb_outputs
 * (ceil(N / decim): outputs per channel after n_wide_total samples; 0 for a bad cfg): host only.
 * opv_wb_create: streams[k] of ctx is fed by channel k. OPV_EINVAL for an index out of range, a stream named twice, or a stream a
 * live wideband object of the context feeds already. Destroy the object before its context; one that outlives it is
 * detached: its pushes and opv_wb_flush answer OPV_ESTATE, and opv_wb_destroy frees only what is the object's own.
 * opv_wb_push / _async / _device: n_wide samples (4-byte aligned; host memory pinned or pageable - a pinned block is read in place
 * across PCIe by the one k_wb_ddc launch that serves all K channels, a pageable one is staged first - or a device pointer). Every
 * channel's output count is known on the host, and room for it is reserved in all K streams before anything is launched, under the
 * rules of opv_push_iq: a flushed or attached stream is OPV_ESTATE, a stream without room even after compaction OPV_ECAPACITY - and
 * the call has then changed NOTHING, in any stream or in the object. opv_wb_push and opv_wb_push_device return when the block
 * has been read; opv_wb_push_async returns once the work is enqueued, like opv_push_iq_batch_async: the block stays valid until
 * opv_push_wait, opv_process may be called in between and queues behind the push on the device. Asynchronous pushes - of one
 * object or of several objects of a context - queue behind each other on the device without a host wait in between.
 * Streams fed this way are ordinary pushed streams for pop, state, taps and export; opv_reset_stream on one is allowed, the
 * object goes on feeding it. opv_wb_flush: opv_flush on each of its streams. */
typedef struct opv_wb_cfg {
    int32_t decim;            /* D: wide samples per output sample */
    int32_t n_channels;       /* K */
    int32_t n_taps;           /* L */
    int32_t out_shift;        /* S */
    uint64_t first_sample;    /* absolute index of the first wide sample pushed (the LO phase is a function of it) */
} opv_wb_cfg;
typedef struct opv_wb opv_wb;
int opv_wb_plan(const opv_wb_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out);
void opv_wb_lo_table(int16_t out4096[4096]);
size_t opv_wb_outputs(const opv_wb_cfg* cfg, uint64_t n_wide_total);
int opv_wb_create(opv_wb** out, opv_ctx* ctx, const opv_wb_cfg* cfg, const int* streams, const double* centre_hz, const int16_t* taps);
void opv_wb_destroy(opv_wb* wb);
int opv_wb_push(opv_wb* wb, const int16_t* iq_wide, size_t n_wide);
int opv_wb_push_async(opv_wb* wb, const int16_t* iq_wide, size_t n_wide);
int opv_wb_push_device(opv_wb* wb, const int16_t* d_iq_wide, size_t n_wide);
int opv_wb_flush(opv_wb* wb);
/* ---- the front door at any radio rate: an exact rational resampler bank ----------------------------------------------------
 * 2 168 000 = 2^6 x 5^3 x 271, so no common radio rate is an integer multiple of it (2.5 MS/s = 625/542, 4 MS/s = 500/271, 10 MS/s =
 * 1250/271, 20 MS/s = 2500/271, 30.72 MS/s = 3840/271, 61.44 MS/s = 7680/271). opv_wb_create_rational makes an opv_wb whose wide
 * rate is Fw = 2 168 000 x down / up S/s; it is an ordinary opv_wb: opv_wb_push / _async / _device, opv_wb_flush and opv_wb_destroy
 * serve it, stream ownership, detachment and refusals are opv_wb_create's and opv_wb_push's (a refused push changes NOTHING), and
 * its streams behave as any pushed stream. Same contract: integer-exact, held to a numpy int64 model with == (tests/
 * test_gpu_wideband_rational.py), any split into pushes gives the same bytes. Write M = down, U = up, L = n_taps, J = ceil(L / U)
 * the taps per phase, taps[t] = 0 for t >= L; wide samples x[n] = (I, Q) int16, n = 0 at the first sample pushed, a = first_sample + n:
 *   increment: fw = (double)M x 2 168 000.0 / (double)U; inc_k = (uint32) llrint(centre_hz[k] / fw x 2^32), modulo 2^32 (these
 *     double operations in this order; for U = 1 they are opv_wb_plan's for decim = M, bit for bit);
 *   mix (the DDC's): phi = (uint32)(a x inc_k), i = phi >> 20, c = T[i], s = T[(i - 1024) & 4095] (opv_wb_lo_table),
 *     mr = I c + Q s, mi = Q c - I s (int32);
 *   resample (zero-stuff m by U, filter with taps at U x Fw, keep every M-th): for output r >= 0, n_r = floor(r M / U),
 *     p_r = (r M) mod U, acc[r] = sum over j = 0 .. J - 1 of taps[p_r + j U] x m[n_r - j], m[n] = 0 for n < 0 (int64);
 *   output count: output r exists once wide sample n_r has arrived: after N wide samples a channel has ceil(N U / M) outputs
 *     (opv_wbr_outputs: no overflow for any uint64 N);
 *   output value, per component: clamp(floor((acc + 2^(S-1)) / 2^S), -32768, 32767) (S = out_shift; S = 0: no rounding term), packed I | Q << 16;
 *   state between pushes: the last J - 1 wide samples and N.
 *   Limits (anything else is OPV_EINVAL, decided on the host by opv_wbr_plan): 1 <= up <= 1024, up <= down <= 32 x up,
 *     gcd(down, up) = 1, 1 <= n_taps and J <= 1024, 1 <= n_channels <= 256, 0 <= out_shift <= 40, reserved = 0, finite centres, and
 *     for EVERY phase p sum_j |taps[p + j U]| <= 2^21 (with |m| < 2^31: |acc| < 2^52, exact in int64).
 *   With U = 1 every formula above is opv_wb_create's with decim = M: such an object (down <= 16) delivers the same bytes.
 * opv_wbr_plan, opv_wbr_outputs (0 for a bad cfg): host only, no device. */
typedef struct opv_wbr_cfg {
    int32_t down, up;          /* M, U: wide rate = 2 168 000 x down / up */
    int32_t n_channels;        /* K */
    int32_t n_taps;            /* L, prototype filter at up x wide rate */
    int32_t out_shift;         /* S */
    int32_t reserved;          /* 0 */
    uint64_t first_sample;
} opv_wbr_cfg;                 /* 32 bytes */
int opv_wbr_plan(const opv_wbr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out);
size_t opv_wbr_outputs(const opv_wbr_cfg* cfg, uint64_t n_wide_total);
int opv_wb_create_rational(opv_wb** out, opv_ctx* ctx, const opv_wbr_cfg* cfg, const int* streams, const double* centre_hz, const int16_t* taps);
/* ---- per-channel retune and Doppler ramps: an LO schedule per channel -------------------------------------------------------
 * The four converters above and below (opv_wb_create, opv_wb_create_rational, opv_wbtx_create, opv_wbtx_create_rational) fix a
 * channel's LO at creation. A schedule lets it move while the object runs - a carrier found by opv_scan_carriers handed to a running
 * door, a LEO pass followed through tens of kHz, an uplink pre-compensated - without emptying the filter history and without a
 * jump of the LO's phase: piecewise-linear frequency, continuous phase, closed form, no carried accumulator. Same contract:
 * integer-exact, held to a numpy model with == (tests/test_gpu_wideband_tune.py), any split into pushes gives the same bytes
 * provided each retune is made before its `at` is pushed, and an object that is never retuned produces the bytes it produced
 * before, from the same kernels.
 *   schedule: per channel a list of segments with ascending `start`, an ABSOLUTE wide-sample index: the a = first_sample + n of
 *     the formulas above, on the transmit side the absolute index of the wide sample WRITTEN. Sample a uses the last segment with
 *     start <= a.
 *   phase, in turns / 2^64, with d = a - start: phi64(a) = phase + d x inc + ramp x tri(d), all modulo 2^64;
 *     tri(d) = d (d - 1) / 2 as an integer (the even factor halved first), then modulo 2^64: defined for every uint64 d.
 *     phi64(a + 1) - phi64(a) = inc + ramp x d: a frequency that moves linearly.
 *   mix: i = phi64 >> 52, c = T[i], s = T[(i - 1024) & 4095] (opv_wb_lo_table); mix, filter, round, clamp, output counts and
 *     history of each converter are exactly as written for it.
 *   creation: one segment {start 0, phase 0, inc = (uint64)inc_k << 32, ramp 0}: ((a x inc_k << 32) mod 2^64) >> 52 ==
 *     ((a x inc_k) mod 2^32) >> 20, the phase of the formulas above. The new rule contains the old one.
 * opv_wb_seg_phase (host only): phi64(a) of a segment. opv_wb_seg_next (host only, no device): the segment that follows `prev`
 *   from sample `at` on: start = at; phase = opv_wb_seg_phase(prev, at), which is what makes the phase continuous;
 *   inc = (uint64)inc32 << 32 with inc32 by opv_wbr_plan's increment rule for (down, up, centre_hz), bit for bit (the integer
 *   door and the integer bank: down = decim resp. interp, up = 1: one definition serves all converters);
 *   ramp = (int64) llrint(rate_hz_s / fw / fw x 18446744073709551616.0), fw = (double)down x 2 168 000.0 / (double)up, these double
 *   operations in this order. From `at` on the channel sits at centre_hz + rate_hz_s x (a - at) / fw. OPV_EINVAL for a null
 *   pointer, down or up below 1, a centre or rate that is not finite, |rate_hz_s| > OPV_WB_TUNE_MAX_RATE.
 * opv_wb_retune / opv_wbtx_retune (both kinds of either object): appends one segment per entry, opv_wb_seg_next's from the
 *   channel's last segment; with phase_given != 0 the entry's `phase` is taken as is instead (a rebuilt object at a migration
 *   destination continues in phase; a deliberate phase reset). It never waits and enqueues nothing, applies to pushes enqueued
 *   after the call, and may be called between opv_wb_push_async calls without opv_push_wait: pushes in flight keep the tables
 *   they were launched with. Write A for the next wide sample the object reads or writes: first_sample + N on the receive side,
 *   first_sample + W(N) on the transmit side. Decided on the host before anything changes; a batch applies whole or not at all:
 *     OPV_ESTATE for at < A (the past cannot be retuned) and for a detached object;
 *     OPV_EINVAL for at < start of the channel's last segment + OPV_WB_TUNE_GAP (the creation segment imposes no gap; on an
 *       object with N = 0 a tune at at = first_sample replaces it), a channel out of range, two entries for one channel that
 *       violate the gap, a centre or rate that is not finite, |rate_hz_s| > OPV_WB_TUNE_MAX_RATE, a null pointer, count < 0;
 *     OPV_ECAPACITY when a channel would hold more than OPV_WB_TUNE_SEGS segments. A segment is dropped, at a push or a retune,
 *       once its successor starts at or before the oldest sample the object can still mix: A - min(N, carry) on the receive
 *       side, which mixes its carried history again every push, and A on the transmit side.
 *   So every segment with a successor, except the creation segment, is at least OPV_WB_TUNE_GAP samples long, and a workgroup,
 *   whose span is at most 4096 wide samples, meets at most two segments of a channel.
 * opv_wb_segments / opv_wbtx_segments: copies the channel's live segments, oldest first, at most `cap` of them, and returns
 *   their count (negative: OPV_EINVAL for a null object or a channel out of range).
 * opv_wbtx_reset returns every channel to its creation schedule. The schedule does not migrate: rebuild the object at the
 *   destination and retune it with phase_given. */
#define OPV_WB_TUNE_GAP  4096      /* wide samples between the starts of two segments of a channel (= a workgroup's largest span) */
#define OPV_WB_TUNE_SEGS 16        /* segments a channel holds at a time */
#define OPV_WB_TUNE_MAX_RATE 1.0e7 /* |rate_hz_s| */
typedef struct opv_wb_seg  { uint64_t start, phase, inc; int64_t ramp; } opv_wb_seg;                  /* 32 bytes */
typedef struct opv_wb_tune { int32_t channel, phase_given; uint64_t at; double centre_hz, rate_hz_s; uint64_t phase; } opv_wb_tune; /* 40 bytes */
uint64_t opv_wb_seg_phase(const opv_wb_seg* seg, uint64_t a);
int opv_wb_seg_next(const opv_wb_seg* prev, int32_t down, int32_t up, uint64_t at, double centre_hz, double rate_hz_s, opv_wb_seg* out);
int opv_wb_retune(opv_wb* wb, int count, const opv_wb_tune* tunes);
int opv_wb_segments(opv_wb* wb, int channel, opv_wb_seg* out, size_t cap);
/* ---- wideband scan: which carriers are in a wide capture, and where ------------------------------------------------------
 * The doors above take their channels' centres as given, and the receive chain behind them acquires a carrier only within the
 * reference's coarse search (-1500 .. +1500 Hz) of where it is told to look; a radio's oscillator is off by far more. An opv_scan
 * object is a bank of P probes on the wide capture - a Welch periodogram at P arbitrary frequencies - and opv_scan_carriers turns
 * a row of probe powers into carrier centres good enough to hand to opv_wb_create / opv_wb_create_rational. Same contract as the
 * doors: integer-exact, independent of summation order and of the split into pushes, held to a numpy int64 model with ==
 * (tests/scan_model.py, tests/test_gpu_scan.py). Write P = n_probes, Lw = n_window, H = hop, A = n_avg, S = out_shift; wide samples
 * x[n] = (I, Q) int16 at Fw = 2 168 000 x down / up S/s (the doors' pair; up = 1 is the integer door's decim = down), n = 0 at the
 * first sample pushed into the object, a = first_sample + n:
 *   increment: inc_p from probe_hz[p] by opv_wbr_plan's rule for the same (down, up), bit for bit (one definition serves both);
 *   mix (the DDC's): phi = (uint32)(a x inc_p), i = phi >> 20, c = T[i], s = T[(i - 1024) & 4095] (opv_wb_lo_table),
 *     mr = I c + Q s, mi = Q c - I s (int32);
 *   segments: segment s >= 0 covers samples [s H, s H + Lw): z_p[s] = sum over t < Lw of window[t] x m_p[s H + t] (int64; sum |window|
 *     <= 2^21, so |z| < 2^52); it exists once sample s H + Lw - 1 has arrived. Per component y = clamp(floor((z + 2^(S-1)) / 2^S),
 *     -2^24, 2^24 - 1) (S = 0: no rounding term), and e_p[s] = yr^2 + yi^2 (<= 2^49);
 *   blocks: block b is segments [b A, b A + A): E[b][p] = sum of e_p[s] over them (uint64, <= 2^61), and exists once its last segment
 *     does. After N samples there are segs = N < Lw ? 0 : (N - Lw) / H + 1 segments and segs / A blocks (opv_scan_blocks). Samples
 *     behind the last whole block never produce output: there is no flush;
 *   state between pushes: N and the samples from the start of the first unfinished block on (fewer than a block's span,
 *     (A - 1) H + Lw): any split of a capture into pushes gives the same rows.
 *   Limits (anything else is OPV_EINVAL, decided on the host by opv_scan_plan): down and up as opv_wbr_plan's, 1 <= P <= 1024,
 *     1 <= Lw <= 4096, 1 <= H <= 65536, 1 <= A <= 4096, (A - 1) H + Lw <= 2^20, 0 <= S <= 40, 1 <= ring_blocks <= 4096,
 *     sum |window| <= 2^21, finite probe frequencies.
 * opv_scan_plan (validates cfg, probes and window and writes the P increments), opv_scan_blocks (0 for a bad cfg): host only.
 * opv_scan_create: the object belongs to ctx - its device and its copy stream, like a wideband object, so that a block of device
 * memory can be scanned and pushed through a door in stream order - and owns no stream of it. Destroy it before its context; one
 * that outlives it is detached: push, pop and reset answer OPV_ESTATE, and opv_scan_destroy frees only what is the object's own.
 * opv_scan_push / _device: n_wide samples, as opv_wb_push (4-byte aligned, fewer than 2^31; pinned memory is read in place, pageable
 * memory is staged). The blocks a push completes go to a ring of ring_blocks rows; a push whose completed blocks do not fit its free
 * rows is OPV_ECAPACITY and has changed NOTHING, as is a push that would take N beyond 2^63. Both return when the block has been read;
 * there is no asynchronous push.
 * opv_scan_pop: waits for the object's queued work, copies the oldest completed rows (at most cap_blocks, P uint64 each) and frees
 * them; returns their count, and in *first_block (may be null) the block index of the first.
 * opv_scan_reset: empties the carry and the ring, sets N = 0 (blocks count from 0 again) and takes a new first_sample.
 * opv_scan_carriers (host only, plain C++): the probes are uniformly spaced, f_p = f0_hz + p x step_hz (step_hz > 0), and `row` is
 * one row or several rows added together. floor = element P / 2 of the ascending sort of the row; W = max(1, ceil(half_width_hz /
 * step_hz)); box[i] = the sum of row[j] over |j - i| <= W inside the row, n_i terms (128-bit integers). Probe i is a candidate
 * when box[i] x 256 > ratio_q8 x n_i x floor (integers). Candidates are taken in descending box order, the lower index first on a tie,
 * skipping any with |i - i'| <= 2 W of one already taken, until cap. For each one taken, over the same j in ascending order and in
 * double: e_j = row[j] > floor ? row[j] - floor : 0, num += (double)e_j x (double)(j - i), den += (double)e_j, and centre_hz =
 * f0_hz + ((double)i + (den > 0 ? num / den : 0.0)) x step_hz, probe = i, excess = den. Returns the count, strongest first;
 * OPV_EINVAL for P outside 1..1024, an f0_hz that is not finite, a step that is not finite and positive, a half width that is not finite and >= 0, or a null pointer.
 *   With a 1024-tap window the probes should lie no more than about 17 kHz apart for the centre to land inside the reference's
 *   +/-1500 Hz search (float experiment, four MSK carriers 4 - 11 kHz off their raster in an 8.672 MS/s capture, 20 - 80 ms: worst
 *   error 786 Hz with probes 8.5 or 16.9 kHz apart, 1.3 - 3.1 kHz with probes 33.9 kHz apart: too coarse).
 *   A noise-free capture has floor = 0, so every probe with any power is a candidate: cap is what bounds the list. */
typedef struct opv_scan_cfg {
    int32_t down, up;          /* wide rate = 2 168 000 x down / up */
    int32_t n_probes;          /* P */
    int32_t n_window;          /* Lw */
    int32_t hop;               /* H */
    int32_t n_avg;             /* A: segments per block */
    int32_t out_shift;         /* S */
    int32_t ring_blocks;       /* rows the object holds until they are popped */
    uint64_t first_sample;
} opv_scan_cfg;                /* 40 bytes */
typedef struct opv_scan_carrier {
    double centre_hz;
    double excess;             /* den: the power above the floor inside the box */
    int32_t probe;             /* i */
    int32_t reserved;          /* 0 */
} opv_scan_carrier;            /* 24 bytes */
typedef struct opv_scan opv_scan;
int opv_scan_plan(const opv_scan_cfg* cfg, const double* probe_hz, const int16_t* window, uint32_t* inc_out);
uint64_t opv_scan_blocks(const opv_scan_cfg* cfg, uint64_t n_wide_total);
int opv_scan_create(opv_scan** out, opv_ctx* ctx, const opv_scan_cfg* cfg, const double* probe_hz, const int16_t* window);
void opv_scan_destroy(opv_scan* scan);
int opv_scan_push(opv_scan* scan, const int16_t* iq_wide, size_t n_wide);
int opv_scan_push_device(opv_scan* scan, const int16_t* d_iq_wide, size_t n_wide);
long opv_scan_pop(opv_scan* scan, uint64_t* rows, size_t cap_blocks, uint64_t* first_block);
int opv_scan_reset(opv_scan* scan, uint64_t first_sample);
long opv_scan_carriers(const uint64_t* row, int n_probes, double f0_hz, double step_hz, double half_width_hz, uint32_t ratio_q8,
                       opv_scan_carrier* out, size_t cap);
/* ---- typed IQ pushes: cs8, cu8 and cf32 converted on the device ---------------------------------------------------------------
 * Replaces nothing in the reference, whose contract is int16. Radios deliver other formats (RTL-SDR unsigned 8-bit, HackRF and many
 * network front-ends signed 8-bit, USRP / SoapySDR float32); a typed push takes the block AS THE RADIO DELIVERED IT, carries it
 * across PCIe in its own format - an 8-bit capture at half the bytes of int16 - and widens it behind the link, in the kernel that
 * writes the stream's device buffer (csrc/opv_push.hip: k_push_convert). From there on the samples are int16 like any other:
 * formats mix freely within one stream, and capacity, compaction, opv_tap_iq and every index count samples, as before.
 *
 * The rule per component (I and Q alike), with an int16 result (csrc/opv_iq_format.h is its one definition, host and device):
 *   format        bytes / sample   source alignment   result
 *   OPV_IQ_CS16   4                4                  identity (the int16 path itself: the old kernel with the old arguments)
 *   OPV_IQ_CS8    2                2                  x * 256             (-32768 .. 32512)
 *   OPV_IQ_CU8    2                2                  (2 u - 255) * 128   (-32640 .. 32640)
 *   OPV_IQ_CF32   8                4                  see below
 *   CS8:  a full-scale 8-bit capture is a full-scale 16-bit one, so out_shift and the offset search's power scaling mean what they
 *         mean today.
 *   CU8:  the centre is 127.5, exactly, with no DC term.
 *   CF32: t = x * 32767.0f as ONE fp32 multiplication, round to nearest even; r = rint(t) with ties to even; the result is
 *         clamp(r, -32767, 32767); NaN gives 0 and +-Inf gives +-32767.
 *
 * opv_push_iq_fmt / opv_push_iq_batch_fmt / _async: opv_push_iq / opv_push_iq_batch / _async for blocks of ONE format per call,
 *   n_samples counted in samples. A block in pinned host memory of this device (aligned for its format, below 2^32 bytes) is read
 *   in place by the convert kernel; anything else - pageable memory, pinned memory of another device, every block while
 *   OPV_PUSH_NO_GATHER is set - is copied raw into a grow-only device stage of the context and converted from there by the same
 *   launch. Results never depend on the route. Refusals are opv_push_iq's (OPV_ESTATE, OPV_ECAPACITY) plus OPV_EINVAL for a format
 *   that does not exist or a pointer that is not aligned for it; a refused block changes nothing, and in a batch the streams before
 *   the error have been pushed, as today. The asynchronous form is settled by opv_push_wait like the int16 one.
 * opv_wb_push_fmt / _async, opv_scan_push_fmt: the block is converted into the object's device stage (a pinned source is read in
 *   place by the convert kernel, a pageable one copied raw first) and the call continues as opv_wb_push_device / opv_scan_push_device:
 *   the wide capture crosses PCIe once, in its own format, and the bank kernels are the int16 ones. Refusals as opv_wb_push /
 *   opv_scan_push (a refused push changes NOTHING), plus the two above.
 * opv_convert_iq_device: n_samples of `fmt` at d_in (device-visible, aligned for the format) to int16 at d_out (4-byte aligned) on
 *   the context's stream, asynchronously like opv_channel_device; the ranges must not overlap. CS16 is a device copy.
 * opv_iq_convert: the rule itself on the host, no device needed; `in` aligned for the format. opv_iq_sample_bytes: 4, 2, 2, 8; 0
 *   for a format that does not exist. */
enum { OPV_IQ_CS16 = 0, OPV_IQ_CS8 = 1, OPV_IQ_CU8 = 2, OPV_IQ_CF32 = 3 };
int opv_push_iq_fmt(opv_ctx* ctx, int stream, int fmt, const void* samples, size_t n_samples);
int opv_push_iq_batch_fmt(opv_ctx* ctx, int fmt, int count, const int* streams, const void* const* samples, const size_t* n_samples);
int opv_push_iq_batch_fmt_async(opv_ctx* ctx, int fmt, int count, const int* streams, const void* const* samples,
                                const size_t* n_samples);
int opv_wb_push_fmt(opv_wb* wb, int fmt, const void* wide, size_t n_wide);
int opv_wb_push_fmt_async(opv_wb* wb, int fmt, const void* wide, size_t n_wide);
int opv_scan_push_fmt(opv_scan* scan, int fmt, const void* wide, size_t n_wide);
int opv_convert_iq_device(opv_ctx* ctx, int fmt, const void* d_in, int16_t* d_out, size_t n_samples);
int opv_iq_convert(int fmt, const void* in, int16_t* out, size_t n_samples);
size_t opv_iq_sample_bytes(int fmt);
/* EOF on a stream: enables the tail processing of :1088-1113 (streaming) or the single
 * whole-capture demodulate of :1166-1173 (batch) at the next opv_process. */
int opv_flush(opv_ctx* ctx, int stream);

/* ---- device-resident path -------------------------------------------------------------
 * Zero-copy variant of push+flush for captures already in HBM (bench, multi-stream
 * servers): d_iq is a DEVICE pointer (16-byte aligned) to n_samples interleaved int16 IQ
 * that must stay valid until the context is destroyed or the stream is reset. */
int opv_attach_device_iq(opv_ctx* ctx, int stream, const int16_t* d_iq, size_t n_samples, int eof);

/* Runs the hot path on everything that is ready, for all streams, in four launches on the
 * context's HIP stream: offset search (estimate_offset :131-202), MSK front-end
 * (demodulate :206-329 incl. the chunker :1026-1076), sync tracker (:615-736) and frame
 * decode (FrameDecoder::decode :854-898). Asynchronous in every round; opv_sync waits. (A search whose candidates tie in the
 * last places of sin / cos is decided with the host's libm before the front-end starts - by a host function enqueued on the
 * context's stream between the two kernels, not by the caller: see opv_offset_ties_on_host.) */
int opv_process(opv_ctx* ctx);
int opv_sync(opv_ctx* ctx);
/* Stream-to-wavefront mapping of the front-end kernel (no counterpart in the reference, which is one thread
 * per process): 1 = one wavefront per stream (lowest per-symbol latency; right while the GPU has idle SIMDs),
 * 4 = four streams per wavefront (fewer issued instructions per symbol; right when every SIMD has work),
 * 16 = sixteen streams per wavefront, one per DPP quad (fewest issued instructions per symbol and stream: 38 against 88 and 156;
 *      right from ~8 000 streams per context, where 16 per wave still put a wave on every second SIMD),
 * 0 = automatic, by the context's stream count (csrc/opv_round_rules.h: frontend_kernel; measured cross-overs on MI355X).
 * Anything else is OPV_EINVAL. Results do not depend on the mapping beyond the fp64 re-association level of the soft symbols
 * (all decisions identical; the tests run every mapping and every launch shape against the oracle). */
int opv_set_frontend(opv_ctx* ctx, int streams_per_wave);
/* Name of the front-end kernel the LAST opv_process launched ("k_msk_frontend_rb", "..._rb_wg4", "k_msk_frontend_x4_wg4", "k_msk_frontend_x16_wg4", ...;
 * "" before the first round): what a profile or a bench line should be read against. No counterpart in the reference. */
const char* opv_frontend_kernel(opv_ctx* ctx);
/* Restores a stream (stream = -1: every stream) to its freshly-created state (keeps buffers). */
int opv_reset_stream(opv_ctx* ctx, int stream);

/* ---- stream migration: a live stream out of one context and into another -------------------------------------------
 * Replaces nothing in the reference: its streams are processes, and a process cannot be checkpointed. Here a
 * stream is its carry (csrc/opv_device.h: OpvStream) plus the tails of its rings, so a server can drain a GPU, re-balance contexts,
 * move from a 256-stream context (one wavefront per stream) to a 4096-stream one (four per wavefront) or restart a process without
 * dropping lock or the frame in flight: the moved stream decodes as if it had never moved (tests/test_gpu_stream_migration.py).
 * opv_export_streams writes ONE self-describing blob for `count` streams into host memory (pinned or pageable; a file or a socket
 * may carry it to another context, process or device) and returns its size in bytes; opv_export_size is an upper bound for the
 * same arguments (0 on error; it holds until the next push or opv_process). Both imply opv_push_wait + opv_sync. The export is a
 * SNAPSHOT: the source stream goes on as before, free its slot with opv_reset_stream. What travels per stream: the OpvStream carry
 * with every absolute index (samples, symbols, frames, events, chunks); the unconsumed IQ from the point compaction keeps, pushed
 * but unprocessed samples included, and the EOF mark; the soft symbols the tracker and the decoder can still read; the unpopped
 * frames with their records, metrics and scales; the unread events; the chunk log; the pop cursors and frame counters.
 * A stream with a released but undecoded frame is refused (OPV_ESTATE; cannot happen after opv_process); a blob buffer that is
 * too small is OPV_ECAPACITY. An ATTACHED (zero-copy) capture is exported as its unconsumed tail and becomes an owned, pushed
 * stream at the destination: the caller's device buffer does not travel.
 * opv_import_streams is opv_reset_stream on each of the `count` destination slots followed by a load, re-based onto the
 * destination's pools and rings, whose capacities (max_samples) may differ; other streams are untouched and rounds in flight
 * are ordered in front of it. The blob format is private to one build of the library. Everything that can refuse an import is
 * decided on the host before anything is launched, and a refused import leaves the context unchanged and usable: OPV_EINVAL for a
 * truncated or malformed blob, a blob of another build, a count other than opv_blob_streams(blob), an index out of range or named
 * twice, or streaming / coherent / have_init_offset / init_offset_hz / pll_bw_hz other than the blob's; OPV_ECAPACITY if the IQ
 * tail, the soft-symbol tail or the unpopped frames do not fit the destination. opv_tap_soft / opv_tap_chunks answer for an
 * imported stream as for any long pushed one: history older than what travelled is gone. Zero-copy consumers
 * (opv_device_frames): the counts entry of an imported slot jumps to the stream's absolute frame number, frame i at slot
 * i % frame_capacity. One launch packs all requested streams (k_stream_pack) in front of one copy, one launch behind one copy
 * unpacks them (k_stream_unpack), whatever the count. Under opv_enable_timing a migration call brackets its copy + kernel the
 * way a round brackets its first kernel: opv_kernel_times [0], the rest ~0.
 * opv_blob_streams: streams in a blob, or OPV_EINVAL; reads the header only - host only, needs no device. */
size_t opv_export_size(opv_ctx* ctx, int count, const int* streams);
long opv_export_streams(opv_ctx* ctx, int count, const int* streams, void* blob, size_t cap);
int opv_import_streams(opv_ctx* ctx, int count, const int* dst_streams, const void* blob, size_t bytes);
int opv_blob_streams(const void* blob, size_t bytes);

/* Measurement hook: when enabled, opv_process brackets each of its four hot-path kernels
 * with HIP events on the context's stream. opv_kernel_times (implies opv_sync) returns the
 * durations in milliseconds of the LAST opv_process: [0] offset search, [1] MSK front-end,
 * [2] sync tracker, [3] frame decode. */
int opv_enable_timing(opv_ctx* ctx, int enable);
int opv_kernel_times(opv_ctx* ctx, float ms_out[4]);

/* ---- results --------------------------------------------------------------------------
 * opv_pop_frames replaces the frame writer (src/opv-demod.cpp:1052-1062): frames whose
 * decoder returned -1 (silent frame, :859) are skipped exactly as the reference skips
 * them. Copies up to cap_frames not-yet-popped frames (134 B each, in release order) and
 * their meta; returns the number copied or a negative error. Implies opv_sync.
 * Frames are never dropped: a stream whose ring of unpopped frames is full pauses (opv_stream_state.stalled)
 * and resumes at the next opv_process after a pop.
 * opv_pop_events returns the tracker lines the reference prints to stderr (:651,677,695,699,705). Reading them
 * is OPTIONAL (opv-modem discards the child's stderr): the log is a ring of the most recent entries per stream
 * (4 per frame of capacity + 64); lines not read in time are overwritten and counted in
 * opv_stream_state.events_dropped, nothing else is affected. */
long opv_pop_frames(opv_ctx* ctx, int stream, uint8_t* out134, size_t cap_frames, opv_frame_meta* meta);
long opv_pop_events(opv_ctx* ctx, int stream, opv_event* out, size_t cap_events);
int opv_get_state(opv_ctx* ctx, int stream, opv_stream_state* out);

/* Device-side views for zero-copy consumers (RCCL gather of decoded frames): frames are
 * [n_streams][frame_capacity][134] uint8, metrics [n_streams][frame_capacity] int32 (-1 =
 * dropped, INT32_MIN = not decoded yet), counts [n_streams] int32 = frames released. */
int opv_device_frames(opv_ctx* ctx, const uint8_t** d_frames, const int32_t** d_metrics,
                      const int32_t** d_counts, size_t* frame_capacity);
void* opv_hip_stream(opv_ctx* ctx);

/* ---- per-frame link report: corrected channel bits and soft-symbol moments (opt-in, OFF by default) -------------------
 * Replaces nothing in the reference, which prints the Viterbi metric and the sync quality of a frame and discards the rest. When
 * the decoder returns, the frame's 2144 soft symbols are still in the soft log and the decoded bytes say what they should have
 * been: re-encoding the frame and holding it against what was received gives the channel bits the decoder corrected (a raw BER
 * in front of the decoder, with no knowledge of the transmitted data) and a decision-directed amplitude and noise power.
 * Definitions, in on-air order i = 0 .. 2143 over the frame's payload soft[payload_symbol + i]:
 *   q_i    the 3-bit value the decoder used for symbol i (src/opv-demod.cpp:862-866; 0 = confident bit 0 .. 7 = confident bit 1);
 *   enc_i  bit i of the transmit chain (randomise, K=7 r=1/2 encode, interleave: opv_tap_tx_frame's interleaved2144) applied to
 *          the 134 decoded bytes - on the receive side the trellis of :815-822 from state 0, read through deinterleave_addr;
 *   bit_errors = #{ i : (q_i >= 4) != enc_i },  weak = #{ i : q_i == 3 or q_i == 4 },  nonfinite = #{ i : soft_i is NaN or +-Inf };
 *   m1 = the decoder's scale (the sequential sum of |soft_i| of :856-858, / 2144),  m2 = sum soft_i^2 / 2144,
 *   ma = sum soft_i e_i / 2144 with e_i = +1 where enc_i == 0 and -1 where enc_i == 1.
 * The four integers are exact. m2 and ma are fp64 sums in a fixed order: the same bits from run to run and from the in-context and
 * the stand-alone form, within 2146 x 2^-53 x (m2, resp. m1) of the exact sums. A frame with nonfinite > 0 leaves m1 / m2 / ma
 * unspecified. A frame the decoder drops (metric -1, :859) has valid = 0, and so has every frame the report did not see (below);
 * every other field of such a record is 0.
 * opv_enable_link_report: the first enable allocates a device ring [n_streams][frame_capacity] of opv_link, zero-filled, indexed
 * like the frame ring (frame f at slot f % frame_capacity); while the report is on, opv_process computes the record of every frame
 * it decodes, with one more launch behind the decoder (opv_kernel_times[3] still brackets the decoder alone). Every later
 * off -> on transition zero-fills the ring again, in stream order: frames decoded while the report was off read valid = 0, never a
 * stale record. An enabling call waits for that zero-fill (it implies opv_sync): a pop may follow it with no round in between.
 * A context that never enables the report allocates and launches nothing for it.
 * opv_pop_frames_link: opv_pop_frames plus the records of the same frames in the same order (dropped frames skipped alike);
 * OPV_ESTATE while the report is off, OPV_EINVAL for a null `link`.
 * opv_device_link: the ring's device view for zero-copy / gather consumers, beside opv_device_frames; OPV_ESTATE if the report was
 * never enabled.
 * opv_link_payloads: the stand-alone form, like opv_decode_payloads and independent of opv_enable_link_report: n_frames payloads
 * of 2144 host doubles each, one record per payload (valid = 0 for payloads the decoder drops). n_frames == 0 is OPV_EINVAL.
 * Reset and migration: opv_reset_stream clears the records of the streams it resets. LINK RECORDS DO NOT MIGRATE:
 * opv_import_streams clears the records of its destination slots like a reset - unpopped frames that arrive by import read
 * valid = 0, frames decoded after the import are reported normally (the blob and the carry of a stream know nothing of the report). */
typedef struct opv_link {
    int32_t valid;       /* 1: computed for this frame; 0: not (see above) - every other field is then 0 */
    int32_t bit_errors;  /* 0..2144 channel bits the decoder corrected */
    int32_t weak;        /* received values with q == 3 or q == 4 */
    int32_t nonfinite;   /* payload values that are NaN or +-Inf */
    double  m1;          /* the decoder's scale: mean |soft|, the SEQUENTIAL sum of ref :856-858 */
    double  m2;          /* mean soft^2 */
    double  ma;          /* mean soft_i * e_i, e_i = +1 where the re-encoded bit is 0, -1 where it is 1 */
} opv_link;              /* 40 bytes */
int opv_enable_link_report(opv_ctx* ctx, int enable);
long opv_pop_frames_link(opv_ctx* ctx, int stream, uint8_t* out134, size_t cap_frames, opv_frame_meta* meta, opv_link* link);
int opv_device_link(opv_ctx* ctx, const opv_link** d_link);
int opv_link_payloads(opv_ctx* ctx, const double* soft, size_t n_frames, opv_link* out);

/* ---- receive diversity: several streams of one context that carry the SAME transmission, decoded as one ------------------
 * (RHCP + LHCP feeds, two antennas, the voting receivers of a repeater; no counterpart in the reference, which decodes every stream
 * alone). The soft value is |c2|^2 - |c1|^2, so summing it over branches is post-detection (square-law) combining; a frame that only
 * some branches found is decoded from those (selection diversity). The front-end, the trackers and the per-stream decoder are not
 * touched: the branches stay ordinary streams - opv_pop_frames, the taps, export and the wideband door behave on them as ever - and
 * a context without a diversity object allocates and launches nothing for it.
 *
 * An object holds n_groups GROUPS of 1..8 BRANCH streams each. opv_div_round, enqueued on the context's stream behind the rounds
 * (opv_process) launched so far, never waiting, does per group:
 *   match    From each branch's cursor into its frame records (payload_symbol, sync_quality, sync_ok: what opv_frame_meta shows):
 *            ANCHOR p0 = the smallest payload_symbol among the branches' next unconsumed records. The group frame is FINAL once every
 *            branch without an unconsumed record can no longer release a payload starting at or before p0 + window - its earliest
 *            possible future payload E_b (read off its tracker: a pending payload's start; behind the next window a HUNTING tracker
 *            will examine; behind the next sync word a LOCKED one will check; infinite once the stream is flushed and its tracker is
 *            done) is > p0 + window. Until then the group waits for a later round. MEMBERS are the branches whose next record starts
 *            within `window` symbols of p0; their records are consumed. Frames are 2168 symbols apart and window <= 64, so the match is
 *            unambiguous, and the emitted sequence is a pure function of the branches' complete record lists: how the input was
 *            split into pushes and rounds decides only WHEN a frame appears.
 *   combine  payload[i] = e_b0 soft_b0[p_b0 + i], then + e_b soft_b[p_b + i] for the other summed members in ascending branch order,
 *            i < 2144: separate IEEE multiplications and additions (no FMA), so the same doubles in give the same bits out. e_b = w_b
 *            (opv_div_set_weights, 1 at creation), in normalised mode w_b / scale_b with scale_b the branch frame's own quantiser scale
 *            (mean |soft| of its payload). A member with w_b == 0, in normalised mode one whose scale is not positive and finite, and
 *            one whose payload has already left its soft ring (counted in softs_lost) stays in `members` and is left out of `summed`.
 *            A frame with summed == 0 is emitted with a zero payload and metric -1.
 *   decode   scale, decoder and link record of the combined payload: the very code of opv_decode_payloads / opv_link_payloads.
 * Losses are counted, never silent: records_lost = branch records overwritten in the stream's record ring before the group consumed
 * them (the caller popped that branch and it ran more than frame_capacity records ahead of the group); the cursor moves forward.
 * Each group's output ring has the context's frame_capacity slots; when it is full of unpopped frames the group STALLS (stalled = 1 in
 * its state, nothing emitted, nothing lost) and resumes with the first round after a pop.
 * opv_div_pop_frames implies opv_sync; it hands out the unpopped group frames in order, skipping those the decoder dropped (metric
 * -1) exactly as opv_pop_frames does; `link` may be null. opv_div_tap_payload (parity tap): the 2144 combined doubles of group frame
 * `frame` (0 = the first ever emitted, dropped ones count) while it is among the last frame_capacity; returns 2144.
 * Weights (finite, >= 0) apply to frames emitted by rounds enqueued after the call.
 * Reset and import: after opv_reset_stream or opv_import_streams on a branch the group's cursor for that branch restarts at the
 * stream's new frame count (0 after a reset, the imported stream's count of released frames after an import): the context notes
 * the restart per stream, and the next opv_div_round carries it to the device in front of its match. Frames already emitted stay;
 * nothing is combined across the restart. The object does not migrate: rebuild it at the destination, as with opv_wb.
 * Refusals, OPV_EINVAL: null arguments, n_groups < 1, a branch count outside 1..8, window outside 0..64, a stream out of range,
 * a stream named twice or already in a live diversity object of the context, weights that are not finite or negative, a group out
 * of range. An object that outlives its context is detached like an opv_wb: its calls answer OPV_ESTATE and opv_div_destroy frees
 * only what is the object's own.
 * opv_div_match: the matching rule alone, on the host, no device needed: branch b has n_recs[b] records recs[b] (ascending
 * payload_symbol) and the earliest future payload earliest[b] (OPV_DIV_ENDED: none will come); from cursors[b] (in / out) it writes
 * the final group frames in order, at most cap, and returns their number. opv_div_earliest: E_b off a tracker's carry. */
#define OPV_DIV_MAX_BRANCHES 8
#define OPV_DIV_MAX_WINDOW 64
#define OPV_DIV_ENDED 0xFFFFFFFFFFFFFFFFull
typedef struct opv_div opv_div;
typedef struct opv_div_cfg { int32_t n_groups, window, normalise, reserved; } opv_div_cfg;   /* window in symbols, 0..64 (8 is a good default) */
typedef struct opv_div_meta {            /* 88 bytes */
    uint64_t payload_symbol[8];          /* per branch; valid where the members bit is set */
    uint32_t members, summed;            /* bit b = branch b */
    int32_t  viterbi_metric, sync_ok;    /* sync_ok = OR over the summed members */
    double   sync_quality;               /* max over the summed members */
} opv_div_meta;
typedef struct opv_div_state {           /* 24 bytes */
    uint32_t frames_emitted;             /* group frames matched so far (dropped ones included) */
    uint32_t frames_decoded, frames_perfect;   /* among them: metric >= 0, metric == 0 */
    uint32_t records_lost, softs_lost;
    int32_t  stalled;                    /* the last round stopped in front of a full output ring */
} opv_div_state;
typedef struct opv_div_rec { uint64_t payload_symbol; double sync_quality; int32_t sync_ok, reserved; } opv_div_rec;
typedef struct opv_div_frame { uint64_t anchor; uint64_t payload_symbol[8]; uint32_t members, reserved; } opv_div_frame;
int  opv_div_create(opv_div** out, opv_ctx* ctx, const opv_div_cfg* cfg, const int* n_branches /*[n_groups]*/, const int* streams /*concatenated*/);
void opv_div_destroy(opv_div* div);
int  opv_div_set_weights(opv_div* div, int group, const double* w /*[branches of the group]*/);
int  opv_div_round(opv_div* div);
long opv_div_pop_frames(opv_div* div, int group, uint8_t* out134, size_t cap_frames, opv_div_meta* meta, opv_link* link);
int  opv_div_get_state(opv_div* div, int group, opv_div_state* out);
long opv_div_tap_payload(opv_div* div, int group, uint32_t frame, double* out2144);
long opv_div_match(int n_branches, uint32_t window, const opv_div_rec* const* recs, const uint32_t* n_recs, const uint64_t* earliest,
                   uint32_t* cursors, opv_div_frame* out, size_t cap);
uint64_t opv_div_earliest(int32_t collecting, int32_t sync_state, uint64_t anchor_symbol, uint64_t next_symbol, int32_t ended);

/* ---- multi-GPU (BASELINE configs[4]; no counterpart in the reference, whose streams are separate processes) -----------
 * Streams shard contiguously over GPUs - one context per GPU, no data-path collective - and the decoded frames return to one
 * rank with ONE gather: ncclGather (/opt/rocm/include/rccl/rccl.h:745) of every context's [n_streams][frame_capacity][134]
 * frame buffer and [n_streams] counts, on the context's HIP stream behind the kernels of the last opv_process
 * (asynchronous; opv_sync waits). d_frames_all / d_counts_all: DEVICE buffers on the root's GPU of world x that size, in
 * rank = global stream order (ignored on other ranks). All contexts of a communicator must have the same n_streams and
 * max_samples. `comm` is an ncclComm_t: the caller's own (a C++ host that links RCCL), or one made here - RCCL is bound with
 * dlopen at first use, so that callers need no RCCL headers and single-GPU callers no RCCL at all:
 *   one process per GPU:   rank 0: opv_comm_unique_id(id), hand the 128 bytes to the other ranks, everyone opv_comm_init,
 *                          then opv_gather_frames once per round;
 *   one process, N GPUs:   opv_comm_init_all(comms, N, devices) (rank i on devices[i]), then opv_gather_frames_all(ctxs, comms,
 *                          N, ...) once per round: the N ranks' gathers issued by one thread inside one RCCL group. */
int opv_comm_unique_id(char out128[128]);
int opv_comm_init(void** comm, int world, int rank, const char id128[128], int device);
int opv_comm_init_all(void** comms, int n_devices, const int* devices);
void opv_comm_destroy(void* comm);
int opv_gather_frames(opv_ctx* ctx, void* comm, int root, uint8_t* d_frames_all, int32_t* d_counts_all);
int opv_gather_frames_all(opv_ctx* const* ctxs, void* const* comms, int n, int root, uint8_t* d_frames_all,
                          int32_t* d_counts_all);

/* ---- parity taps (debug): the intermediates the 1e-5 contract is checked on ------------ */
/* soft symbols by absolute symbol index; only the retained tail of a long pushed stream is available */
long opv_tap_soft(opv_ctx* ctx, int stream, uint64_t first_symbol, double* out, size_t cap);
/* the IQ a pushed (or wideband-fed) stream holds on the device, by absolute sample index: up to cap samples (2 int16 each) from
 * first_sample; returns the number copied - 0 outside what the stream's buffer still retains. Implies opv_push_wait + opv_sync. */
long opv_tap_iq(opv_ctx* ctx, int stream, uint64_t first_sample, int16_t* out, size_t cap);
/* The other direction: n soft symbols (host doubles, any values - NaN and infinities included) are appended to the stream's
 * soft-symbol log exactly where its front-end would have written them, behind the rounds launched so far, and the next
 * opv_process runs the tracker, the scale pre-pass and the decoder over them with the very launches it uses for pushed IQ.
 * Test infrastructure: it lets a checker hand the back half of the receive chain a made soft log. opv_get_state,
 * opv_pop_frames, opv_pop_events and opv_tap_soft answer for such a stream as for any other (total_symbols counts the staged
 * symbols; the front-end's fields stay as created). Room follows the front-end's own back-pressure rule: symbols the tracker
 * or a pending payload may still read are never overwritten - a push that does not fit is OPV_ECAPACITY and stages nothing
 * (opv_process / opv_pop_frames make room). A stream takes EITHER IQ or staged symbols between two opv_reset_stream: this call
 * answers OPV_ESTATE on a stream that has received IQ (pushed, attached, wideband-fed, imported) or has been flushed, and
 * opv_push_iq*, opv_attach_device_iq, opv_flush, the wideband pushes and opv_export_streams answer OPV_ESTATE on a stream
 * that holds staged symbols; the context stays usable either way. Null pointers, a stream out of range or n == 0: OPV_EINVAL.
 * Waits for the rounds in flight. */
int opv_tap_push_soft(opv_ctx* ctx, int stream, const double* soft, size_t n);
/* per demodulate() call, starting at call number first_chunk: {freq_offset, timing_freq, mu,
 * leftover, n_symbols}. The log is a ring of the most recent calls. */
long opv_tap_chunks(opv_ctx* ctx, int stream, uint32_t first_chunk, double* out5, size_t cap_chunks);
/* 134 candidate energies of the offset search in scan order (121 coarse, 13 fine) */
int opv_tap_offset_energies(opv_ctx* ctx, int stream, double* out134);
/* Who decides the offset search's last-place ties (estimate_offset's strict '>' between candidates whose energies, evaluated in
 * the reference's order of operations, are within 2e-13 of each other - what the last places of sin / cos can move - or equal,
 * src/opv-demod.cpp:161,195): 1 = the host, with the contenders evaluated by the reference's own loop on the
 * host's libm - opv_create found that this process's sin / cos reproduce a pinned reference energy (csrc/opv_offset_host.cpp);
 * 0 = the device's sincos (another libm on the host, a host that cannot pin the staging area or enqueue host functions, or the
 * test hook OPV_OFFSET_DISTRUST_LIBM, see opv_create): still the reference's order of
 * operations, counted in offset_ties, but an exact tie is then decided by a different libm than the reference's. */
int opv_offset_ties_on_host(opv_ctx* ctx);
/* Streams whose tie the host has decided so far in this context (they are decided in stream order behind their search kernel,
 * opv_process does not wait for them: the number is final for a round after opv_sync). Diagnostic. */
uint64_t opv_offset_ties_decided_on_host(opv_ctx* ctx);
/* Streams that were listed for the host beyond what one round stages (8 passes x min(n_streams, 512) slots = up to 4096 streams of
 * ONE context whose search ties at the last-place level in ONE round) and therefore kept the device's decision, as under
 * opv_offset_ties_on_host() == 0. Exact mirror ties (real-valued captures: the one systematic source) come out the same either
 * way; for others this is a parity class to report. 0 in every test and bench run. Diagnostic. */
uint64_t opv_offset_ties_left_to_device(opv_ctx* ctx);

/* Where and how fast the wavefront that served `stream` ran in the LAST front-end launch (with four streams per
 * wave, the four share these numbers): out[0] = HW_REG_HW_ID, out[1] = HW_REG_XCC_ID, out[2] = shader-clock cycles (s_memtime) and
 * out[3] = 100 MHz ticks (s_memrealtime) spent inside the kernel. Diagnostic: placement census and the clock the
 * chip held (cycles / ticks x 100 MHz); no counterpart in the reference. */
int opv_tap_wave_info(opv_ctx* ctx, int stream, uint64_t out[4]);

/* demodulate() calls of `stream` since its reset that k_msk_frontend_rb / _rb_wg4 ran out[0] = without the timing loop's clamp (the
 * per-call proof of csrc/opv_tf_rule.h held) and out[1] = with it. The four- and sixteen-streams-per-wave mappings always clamp and
 * count nothing; an imported stream starts at 0. Diagnostic; no counterpart in the reference. */
int opv_tap_frontend_calls(opv_ctx* ctx, int stream, uint64_t out[2]);

/* Workgroups of each hot-path kernel the runtime can keep resident per CU (hipOccupancyMaxActiveBlocksPerMultiprocessor), in the
 * order k_msk_frontend_rb, _rb_wg4, k_msk_frontend_x16_wg4, k_msk_frontend_x4_wg4, k_frame_decode, k_frame_scale. Diagnostic. */
int opv_tap_occupancy(opv_ctx* ctx, int out[6]);

/* Stand-alone FrameDecoder::decode (src/opv-demod.cpp:854-898) on n_frames payloads of
 * 2144 host doubles each. Optional taps: q (quantised, :862-866), deint (:869-871),
 * bits (Viterbi hard decisions, :874-875). metrics[i] = path metric or -1. */
int opv_decode_payloads(opv_ctx* ctx, const double* soft, size_t n_frames, uint8_t* out134,
                        int32_t* metrics, int8_t* q, int8_t* deint, uint8_t* bits);

/* ---- signal source (reference src/opv-mod.cpp) ---------------------
 * Host-side, bit-identical to `opv-mod`: BERT frames (:339-361) and the whole
 * encode->interleave->MSK chain incl. 100 trailing zero symbols (:473-529). */
void opv_tx_bert_frame(const char* callsign, uint32_t token, uint32_t frame_num, uint8_t out134[OPV_FRAME_BYTES]);
/* n_frames consecutive BERT frames (frame numbers first_frame, first_frame + 1, ...) into out134[n_frames][134] */
void opv_tx_bert_frames(const char* callsign, uint32_t token, uint32_t first_frame, size_t n_frames, uint8_t* out134);
size_t opv_tx_modulated_samples(size_t n_frames);
size_t opv_tx_modulate(const uint8_t* frames134, size_t n_frames, int16_t* iq_out);
/* The same modulator as an object that carries its state from call to call (the reference's HDLModulator,
 * src/opv-mod.cpp:219-291: two free-running NCOs, the differential sign, the symbol parity), for a source that produces frames
 * as it goes - `opv-mod -R` on a live pipe (:473-498), `opv-mod -c` (:503-524: one reset per pass over the BERT frames).
 * create = a modulator after reset() (:221-226); opv_tx_stream_frames appends n_frames x 2168 x 40 samples to iq_out and
 * returns that count; opv_tx_stream_tail writes the 100 silent symbols that end a run (:528-529; 4000 samples, no state).
 * Any split of a run into calls gives the bytes of one opv_tx_modulate call. Host only, needs no device. */
/* Parity tap of the bit-level half (src/opv-mod.cpp:158-213): one frame after the randomiser (134 bytes), after the
 * convolutional encoder (2144 bits, one per byte, encoder order) and after the interleaver (on-air order). Any output may be
 * NULL. What `opv-mod -v` prints the first bytes / bits of (:171-183,198-209,326-329). */
void opv_tap_tx_frame(const uint8_t* frame134, uint8_t* randomized134, uint8_t* coded2144, uint8_t* interleaved2144);
typedef struct opv_tx_stream opv_tx_stream;
opv_tx_stream* opv_tx_stream_create(void);
void opv_tx_stream_reset(opv_tx_stream* st);
size_t opv_tx_stream_frames(opv_tx_stream* st, const uint8_t* frames134, size_t n_frames, int16_t* iq_out);
size_t opv_tx_stream_tail(int16_t* iq_out);
void opv_tx_stream_destroy(opv_tx_stream* st);
/* Device-side transmit chain: same result as opv_tx_modulate, written straight into HBM
 * (d_iq_out: device pointer, 16-byte aligned, opv_tx_modulated_samples(n_frames) samples). The whole chain of
 * src/opv-mod.cpp:97-291 runs on the device: randomiser, convolutional encoder, interleaver and sync word per frame
 * (k_tx_encode), the differential sign as a parity prefix over the run (k_tx_scan_frames), the two free-running NCOs
 * (k_tx_expand_phases, from a build-time table of their state every 128th symbol; once per context and run length, shared by
 * every stream), sample synthesis (k_tx_modulate). `frames134` is a host pointer (134 bytes per frame cross PCIe). Samples
 * whose truncation could differ between device sincos and libm are re-evaluated on the host. Returns the number of samples so
 * patched (>= 0, normally 0) or a negative error. Synchronous. */
long opv_tx_modulate_device(opv_ctx* ctx, const uint8_t* frames134, size_t n_frames, int16_t* d_iq_out);
/* The same chain for a host that wants the samples back (`opv-mod -G`): a temporary device buffer, then D2H into iq_out
 * (host, opv_tx_modulated_samples(n_frames) samples). */
long opv_tx_modulate_device_to_host(opv_ctx* ctx, const uint8_t* frames134, size_t n_frames, int16_t* iq_out);
/* Parity tap: entries [first, first + count) of the NCO checkpoint sequence the device transmit chain starts from - (ph1, ph2)
 * of src/opv-mod.cpp:274-279 at symbol 128 * entry of a run - from the build-time table, beyond it (4096 frames) from the host
 * continuation. Host only, needs no device. */
void opv_tap_tx_checkpoints(size_t first, size_t count, double* out2);
/* ---- transmit bank: N live modulators on the device, their state carried from round to round ----------------------------
 * Replaces N HDLModulator objects (src/opv-mod.cpp:219-291), each driven frame by frame as `opv-mod -R` drives its one
 * (:473-498): a gateway that transmits many channels hands a few frames per channel and round to ONE set of launches and gets
 * every channel's samples in device memory - the bytes the host modulator (opv_tx_stream_frames, `opv-mod`) makes.
 * State of a modulator: `symbols`, the symbols it has put on the air since its reset, and `sign_parity`, the parity of all on-air
 * bits sent since then: the differential sign T (:232-239) is -1 where it is odd (T = 0 holds only for symbol 0 of a run, which is
 * silent), and b_n (:246-257) follows from the parity of `symbols`. The NCO phases (:274-279) are no part of the state: they are
 * a function of `symbols` alone (opv_tap_tx_checkpoints every 128 symbols, replayed from there with the same adds and wraps).
 * The two numbers are the whole modulator, so opv_txb_get_state / opv_txb_set_state also move a stream between banks.
 * opv_txb_create: replaces N constructions + reset() (:221-226): n_streams (1 .. OPV_TXB_MAX_STREAMS) modulators as after reset,
 *   tied to `ctx` (its device, its HIP stream, its NCO checkpoints and flat-top bits; the bank adds a byte of device state per
 *   stream and a scratch area sized by the largest ROUND - nothing that grows with the length of a run).
 * opv_txb_destroy: before its context. A bank whose context went first is detached: every call that needs the device answers
 *   OPV_ESTATE, opv_txb_get_state still answers, and destroy frees what is the bank's own.
 * opv_txb_reset: replaces reset() (:221-226) of one modulator, or of all (stream = -1): the next frame starts with the silent symbol.
 * opv_txb_get_state / opv_txb_set_state: no counterpart in the reference (its modulator cannot be moved). set_state refuses
 *   (OPV_EINVAL) a sign_parity outside {0, 1}, a non-zero `reserved` and symbols beyond OPV_TXB_MAX_RUN_FRAMES frames.
 * opv_txb_round: replaces one pass of the sending loop (:473-498) for `count` of the modulators: entry i lets stream streams[i]
 *   modulate the n_frames[i] frames at frames134[i] (0 is allowed and changes nothing) and writes n_frames[i] x 86720 samples to
 *   the device pointer d_iq_out[i] (16-byte aligned). Frames are read from host memory, or - frames_on_device != 0 - from
 *   device memory in stream order on the context's HIP stream (slices of opv_device_frames: a repeater needs no host copy; a
 *   ring wrap is two rounds). Streams not named stand still. Synchronous; returns the number of samples re-evaluated on the host
 *   with libm (>= 0, normally 0) or a negative error. For every stream, what its rounds wrote since its last reset equals the
 *   first F x 86720 samples of opv_tx_modulate on the same F frames, for any split into rounds and any company in the bank. The
 *   100 silent symbols that end a run are 4000 zero samples and carry no state (opv_tx_stream_tail): the caller's to write.
 *   Refusals are decided before anything is enqueued and change nothing: OPV_EINVAL for a null pointer, count < 0, a stream out
 *   of range or named twice, an output that is misaligned or overlaps another entry's, a round of more than 2^31 / 34 frames;
 *   OPV_ECAPACITY for a stream whose run would pass OPV_TXB_MAX_RUN_FRAMES frames (reset it, as `opv-mod -c` resets once per
 *   pass, :503-524); OPV_ESTATE for a detached bank.
 * opv_txb_plan_round: those refusals plus the launch geometry, host only (needs no device; what opv_txb_round itself calls):
 *   states[n_streams] as opv_txb_get_state gives them, out_addr[i] the address d_iq_out[i]; first_block[count + 1]: entry i owns
 *   workgroups [first_block[i], first_block[i + 1]) of the modulate grid (64 symbols each: ceil(n_frames[i] x 2168 / 64), the last
 *   one partial; none for an entry of 0 frames), first_symbol[count]: the entry's first symbol as an index into its stream's run.
 * opv_tap_txb_patch (parity tap, host only): the int16 (I, Q) of ONE sample as the round's host patch evaluates an entry of the
 *   device's list of ambiguous samples - sample `sample` (0..39) of symbol `symbol` of a run, tone / sign `code` (+-1 tone 1,
 *   +-2 tone 2, 0 silent) - with libm, as the reference computes it (:268-279). */
#define OPV_TXB_MAX_RUN_FRAMES 65536   /* 43.7 minutes on the air: 17.8 MB of NCO checkpoints at the far end */
#define OPV_TXB_MAX_STREAMS 65536
typedef struct opv_txb opv_txb;
typedef struct opv_txb_state { uint64_t symbols; int32_t sign_parity; int32_t reserved; } opv_txb_state;
int opv_txb_create(opv_txb** out, opv_ctx* ctx, int n_streams);
void opv_txb_destroy(opv_txb* txb);
int opv_txb_reset(opv_txb* txb, int stream);
int opv_txb_get_state(opv_txb* txb, int stream, opv_txb_state* out);
int opv_txb_set_state(opv_txb* txb, int stream, const opv_txb_state* in);
long opv_txb_round(opv_txb* txb, int count, const int* streams, const uint8_t* const* frames134,
                   const size_t* n_frames, int16_t* const* d_iq_out, int frames_on_device);
int opv_txb_plan_round(int n_streams, const opv_txb_state* states, int count, const int* streams,
                       const size_t* n_frames, const uintptr_t* out_addr, uint32_t* first_block, uint64_t* first_symbol);
int opv_tap_txb_patch(uint64_t symbol, int sample, int code, int16_t out_iq[2]);
/* ---- wideband transmit: K per-channel captures in, ONE wide capture out --------------------------------------------------
 * The mirror image of opv_wb_*, and the stage behind the transmit bank: opv_txb_round leaves per-channel int16 captures at
 * 2 168 000 S/s in device memory; an opv_wbtx object is a bank of K digital up-converters on the device that puts them on one
 * carrier raster at interp x 2 168 000 S/s. The arithmetic is integer-exact and independent of summation order
 * (tests/test_gpu_wideband_tx.py holds the device to the numpy int64 model of tests/wideband_models.py with ==):
 *   every channel delivers the same number of input samples x_k[m] = (I, Q) int16 per push, m = 0 at the first sample pushed into the
 *   object, x_k[m] = 0 for m < 0; after N input samples per channel the object has written exactly N x interp wide samples.
 *   Wide sample n = q interp + p (0 <= p < interp) has the absolute index a = first_sample + n. Per channel k and component:
 *     y_k[n] = sum over j >= 0 with p + j interp < n_taps and q - j >= 0 of taps[p + j interp] x_k[q - j] (zero-stuffing, then an FIR; int32);
 *     inc_k, phi = (uint32)(a x inc_k), i = phi >> 20, c = T[i], s = T[(i - 1024) & 4095] are the DDC's above with decim = interp:
 *     one increment rule and one table (opv_wb_lo_table) serve both banks; the channel goes UP to +centre_hz, the conjugate of the DDC's mix:
 *     wr += yr c - yi s, wi += yi c + yr s (int64, summed over k);
 *   output per component clamp(floor((w + 2^(out_shift - 1)) / 2^out_shift), -32768, 32767) (out_shift = 0: no rounding term), packed
 *   I | Q << 16 like every capture here.
 *   Limits (anything else is OPV_EINVAL from opv_wbtx_plan / opv_wbtx_create): 1 <= interp <= 16, 1 <= n_taps <= 1024, 1 <= n_channels <= 256,
 *     0 <= out_shift <= 40, for every phase p sum_j |taps[p + j interp]| <= 65535 (so |y| < 2^31: exact in int32; and
 *     |sum_k w| < 256 x 2 x 2^31 x 2^15 = 2^55: exact in int64), finite centres.
 * The only state between pushes is the last ceil((n_taps - 1) / interp) input samples of every channel and the count N: any split of
 * the inputs into pushes gives the bytes of one push. The object does NOT migrate: rebuild it at the destination with
 * first_sample + N x interp as its first_sample - and mind that its n = 0 then starts with an empty filter history.
 * opv_wbtx_plan (host only, no device): validates cfg, centres and taps and writes the K increments.
 * opv_wbtx_create: tied to ctx (its device and the HIP stream its transmit bank uses). Destroy the object before its context;
 *   one that outlives it is detached: pushes and opv_wbtx_reset answer OPV_ESTATE, opv_wbtx_samples still answers, and
 *   opv_wbtx_destroy frees only what is the object's own.
 * opv_wbtx_push: d_in[k] is a device pointer to n_in packed samples (4-byte aligned), or null: an absent channel contributes zeros
 *   for that push - its earlier samples still ring out through the filter, and zeros enter its history (a transmit-bank stream that
 *   stands still in a round; an all-null push of 4000 samples is the silent tail of a run). The same buffer may serve several
 *   channels. d_wide_out: device pointer to n_in x interp packed samples (4-byte aligned). One k_wbtx_duc launch in stream order
 *   on the context's HIP stream (behind the opv_txb_round that made the inputs); synchronous like opv_txb_round. Refusals are
 *   decided before anything is enqueued and change nothing: OPV_EINVAL for a null table or output, a misaligned pointer, an output
 *   that overlaps an input, n_in x interp >= 2^31; OPV_ESTATE for a detached object. n_in = 0 is allowed and changes nothing.
 * opv_wbtx_samples: N. opv_wbtx_reset: empties the history, sets N = 0 and first_sample. */
typedef struct opv_wbtx_cfg {
    int32_t interp;           /* U: wide samples per input sample */
    int32_t n_channels;       /* K */
    int32_t n_taps;           /* L */
    int32_t out_shift;        /* S */
    uint64_t first_sample;    /* absolute index of the first wide sample written (the LO phase is a function of it) */
} opv_wbtx_cfg;
typedef struct opv_wbtx opv_wbtx;
int opv_wbtx_plan(const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out);
int opv_wbtx_create(opv_wbtx** out, opv_ctx* ctx, const opv_wbtx_cfg* cfg, const double* centre_hz, const int16_t* taps);
void opv_wbtx_destroy(opv_wbtx* wbtx);
int opv_wbtx_push(opv_wbtx* wbtx, const int16_t* const* d_in, size_t n_in, int16_t* d_wide_out);
uint64_t opv_wbtx_samples(const opv_wbtx* wbtx);
int opv_wbtx_reset(opv_wbtx* wbtx, uint64_t first_sample);
/* ---- wideband transmit at any radio rate: an exact rational up-converter bank ----------------------------------------------
 * The mirror image of opv_wb_create_rational. opv_wbtx_create_rational makes an opv_wbtx whose wide rate is
 * Fw = 2 168 000 x down / up S/s (10 MS/s = 1250/271, 61.44 MS/s = 7680/271: the SAME pair the radio's opv_wbr_cfg carries); it is an
 * ordinary opv_wbtx: opv_wbtx_push, opv_wbtx_samples, opv_wbtx_reset and opv_wbtx_destroy serve it, detachment and refusals are
 * opv_wbtx_push's (a refused push changes NOTHING). Same contract: integer-exact, independent of summation order, held to a numpy
 * int64 model with == (tests/test_gpu_wideband_tx_rational.py), any split of the inputs into pushes gives the bytes of one push.
 * Write M = down, U = up, L = n_taps, J = ceil(L / M) the taps per phase, taps[t] = 0 for t >= L; every channel delivers the same
 * number of inputs x_k[m] = (I, Q) int16 per push, m = 0 at the first sample pushed, x_k[m] = 0 for m < 0:
 *   increment: opv_wbr_plan's for the same (down, up, centre), bit for bit (one definition serves both): a channel sent up through
 *     this bank comes down through a rational door with the same (down, up, centre_hz);
 *   resample (zero-stuff x by M, filter with taps at M x 2 168 000 S/s = U x Fw, keep every U-th): for wide sample n >= 0,
 *     q_n = floor(n U / M), p_n = (n U) mod M, y_k[n] = sum over j = 0 .. J - 1 of taps[p_n + j M] x x_k[q_n - j], per component (int32);
 *   mix up and sum: a = first_sample + n, phi = (uint32)(a x inc_k), i = phi >> 20, c = T[i], s = T[(i - 1024) & 4095]
 *     (opv_wb_lo_table), wr += yr c - yi s, wi += yi c + yr s (int64, summed over k);
 *   output value: opv_wbtx_push's: clamp(floor((w + 2^(S-1)) / 2^S), -32768, 32767) (S = out_shift; S = 0: no rounding term), packed I | Q << 16;
 *   output count: wide sample n exists once input q_n has arrived: after N inputs per channel the object has written
 *     W(N) = ceil(N M / U) wide samples (opv_wbtxr_outputs). A push of n_in inputs behind N writes W(N + n_in) - W(N) samples to
 *     d_wide_out, the first with index W(N), input q = N and phase p = W(N) U - N M. One frame (86 720 = 320 x 271 inputs) at up = 271
 *     is a whole number of wide samples;
 *   state between pushes: the last J - 1 inputs of every channel (zeros for a channel absent from a push, as in opv_wbtx_push) and N.
 *   Limits (anything else is OPV_EINVAL, decided on the host by opv_wbtxr_plan): 1 <= up <= down <= 8192, down <= 32 x up,
 *     gcd(down, up) = 1, 1 <= n_taps and J <= 64 (so n_taps <= 524 288), 1 <= n_channels <= 256, 0 <= out_shift <= 40, reserved = 0,
 *     finite centres, non-null pointers, and for EVERY phase p sum_j |taps[p + j M]| <= 65535 (so |y| < 2^31: exact in int32; and
 *     |sum_k w| < 2^55: exact in int64).
 *   Push refusals, decided before anything is enqueued: OPV_EINVAL for a null table or output, a misaligned pointer, an output range of
 *     (W(N + n_in) - W(N)) x 4 bytes that overlaps an input, n_in >= 2^31 or 2^31 or more wide samples in one push; OPV_ECAPACITY for
 *     a push that would take N past 2^50 (16 years of signal; it keeps N M + U inside uint64); OPV_ESTATE for a detached object.
 *     n_in = 0 is allowed and changes nothing.
 *   With U = 1 every formula above is opv_wbtx_create's with interp = M: for M <= 16 and L <= min(1024, 64 M) such an object
 *     delivers the same bytes.
 *   opv_wbtx_reset(first_sample) empties the history and sets N = 0. The object does NOT migrate: rebuild it at the destination
 *     where N is a multiple of up (a frame boundary, for instance) with first_sample + N x down / up as its first_sample - elsewhere
 *     the phase p does not restart at 0 - and mind that its n = 0 then starts with an empty filter history.
 * opv_wbtxr_plan, opv_wbtxr_outputs (0 for a bad cfg or N > 2^50): host only, no device. */
typedef struct opv_wbtxr_cfg {
    int32_t down, up;          /* M, U: wide rate = 2 168 000 x down / up - the SAME pair a radio's opv_wbr_cfg carries */
    int32_t n_channels;        /* K */
    int32_t n_taps;            /* L, prototype filter at down x 2 168 000 S/s (= up x wide rate: the rate the rational door's prototype runs at) */
    int32_t out_shift;         /* S */
    int32_t reserved;          /* 0 */
    uint64_t first_sample;     /* absolute index of the first wide sample written */
} opv_wbtxr_cfg;               /* 32 bytes, the layout of opv_wbr_cfg */
int opv_wbtxr_plan(const opv_wbtxr_cfg* cfg, const double* centre_hz, const int16_t* taps, uint32_t* inc_out);
uint64_t opv_wbtxr_outputs(const opv_wbtxr_cfg* cfg, uint64_t n_in_total);
int opv_wbtx_create_rational(opv_wbtx** out, opv_ctx* ctx, const opv_wbtxr_cfg* cfg, const double* centre_hz, const int16_t* taps);
/* the LO schedule of an up-converter bank of either kind: the rule, the refusals and the structs are opv_wb_retune's above, with
 * A = first_sample + W(N) (the integer bank: N interp), the next wide sample the object writes */
int opv_wbtx_retune(opv_wbtx* wbtx, int count, const opv_wb_tune* tunes);
int opv_wbtx_segments(opv_wbtx* wbtx, int channel, opv_wb_seg* out, size_t cap);
/* Device-side channel tool for synthetic multi-stream workloads:
 * d_out[n] = clip(rint(gain * d_in[n] * exp(j 2 pi f0 n / Fs) + sigma * N(0,1)+jN(0,1))),
 * noise from a counter-based generator keyed by (seed, n). d_in/d_out: device int16 IQ. */
int opv_channel_device(opv_ctx* ctx, const int16_t* d_in, int16_t* d_out, size_t n_samples,
                       double gain, double f0_hz, double sigma, uint64_t seed);
/* Sample-clock error for the same tool chain: d_out[n] = rint(linear interpolation of d_in
 * at n (1 + clock_ppm 1e-6)), i.e. the capture as an ADC running clock_ppm parts per million fast would have
 * taken it. Returns the number of samples written, floor(n_in / (1 + clock_ppm 1e-6)) <= out_capacity, or a
 * negative error. Asynchronous on the context's stream like opv_channel_device. */
long opv_resample_device(opv_ctx* ctx, const int16_t* d_in, size_t n_in, int16_t* d_out, size_t out_capacity,
                         double clock_ppm);

#ifdef __cplusplus
}
#endif
#endif /* OPV_DEMOD_H */
