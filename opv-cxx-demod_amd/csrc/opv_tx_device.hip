// opv_tx_device.hip — the device transmit chain behind the C ABI (opv_tx_modulate_device: frames -> code bytes -> samples,
// bit-identical to the host modulator) and the channel / resampler entry points that test signals are made with.
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

#include "opv_ctx.h"
#include "opv_tx_internal.h"

// k_tx_modulate.hip decides the flat tops of the transmit NCOs by the symbol index: |sin| / |cos| at a quarter-period point
// +/- eps is exactly 1.0 while eps < kFlatExact and below 1.0 from kFlatBelow on. True of glibc's correctly rounded-in-practice
// sin / cos (1 - eps^2/2 rounds to 1.0 while eps^2/2 < 2^-54); a libm with 1 ulp of slack may answer differently, so it is
// asked, once per process: 5 tops x 2 sides x 2 x 256 offsets.
constexpr double kFlatExact = 0.90e-8, kFlatBelow = 1.25e-8;
bool opv_tx_libm_flat_tops_as_assumed() {
    static const bool ok = [] {
        const double pi = 3.14159265358979323846;
        const struct { bool is_sin; double x0; } tops[] = {{true, pi / 2}, {true, -pi / 2}, {false, 0.0}, {false, pi}, {false, -pi}};
        for (const auto& t : tops)
            for (int k = 0; k <= 256; ++k) {
                const double e = kFlatExact * k / 256.0;                                       // must be exactly +/-1
                const double b = kFlatBelow * std::pow(1.0e-5 / kFlatBelow, k / 256.0);       // must be below: 1.25e-8 .. 1e-5, log-spaced
                for (double sgn : {1.0, -1.0}) {
                    const double ve = std::fabs(t.is_sin ? std::sin(t.x0 + sgn * e) : std::cos(t.x0 + sgn * e));
                    const double vb = std::fabs(t.is_sin ? std::sin(t.x0 + sgn * b) : std::cos(t.x0 + sgn * b));
                    if (ve != 1.0 || !(vb < 1.0)) return false;
                }
            }
        return true;
    }();
    return ok;
}

extern "C" int opv_channel_device(opv_ctx* c, const int16_t* d_in, int16_t* d_out, size_t n, double gain,
                                  double f0_hz, double sigma, uint64_t seed) {
    if (!c || !d_in || !d_out) return fail(OPV_EINVAL, "null argument");
    if ((n & 3u) || (((uintptr_t)d_in | (uintptr_t)d_out) & 15u))
        return fail(OPV_EINVAL, "opv_channel_device: n must be a multiple of 4 and pointers 16-byte aligned");
    HIPCHK(hipSetDevice(c->cfg.device));
    const uint64_t quads = n / 4;
    unsigned blocks = (unsigned)((quads + 255) / 256);
    if (blocks > 256u * 8u) blocks = 256u * 8u;  // 8 blocks per CU, grid-stride the rest
    if (blocks == 0) return OPV_OK;
    k_channel<<<blocks, 256, 0, c->stream>>>((const int4*)d_in, (int4*)d_out, quads, gain, f0_hz / 2168000.0, sigma, seed);
    HIPCHK(hipGetLastError());
    return OPV_OK;
}

extern "C" long opv_resample_device(opv_ctx* c, const int16_t* d_in, size_t n_in, int16_t* d_out, size_t out_cap,
                                    double clock_ppm) {
    if (!c || !d_in || !d_out) return fail(OPV_EINVAL, "null argument");
    if (n_in < 2) return fail(OPV_EINVAL, "opv_resample_device: at least two input samples");
    if (!(clock_ppm > -5e5 && clock_ppm < 5e5)) return fail(OPV_EINVAL, "opv_resample_device: |clock_ppm| must be below 5e5");
    HIPCHK(hipSetDevice(c->cfg.device));
    const double rate = 1.0 + clock_ppm * 1e-6;
    const uint64_t n_out = (uint64_t)((double)n_in / rate);
    if (n_out > out_cap) return fail(OPV_ECAPACITY, "opv_resample_device: output buffer too small");
    if (n_out == 0) return 0;
    unsigned blocks = (unsigned)((n_out + 255) / 256);
    if (blocks > 256u * 8u) blocks = 256u * 8u;
    k_resample_clock<<<blocks, 256, 0, c->stream>>>((const int*)d_in, (uint64_t)n_in, (int*)d_out, n_out, rate);
    HIPCHK(hipGetLastError());
    return (long)n_out;
}

// What a run of nsym symbols needs on the device besides its frames - the NCO checkpoints under it, the flat-top zone limits and
// the flat bits up to its end - for whoever modulates it: opv_tx_modulate_device (one run from a reset) and a transmit bank's
// round (opv_tx_bank.hip: nsym = the largest symbol any of its streams reaches). Grow-only, per context; both are synchronous
// on the context's stream, so nothing on it reads these tables while they are extended.
int opv_tx_prepare_run(opv_ctx* c, size_t nsym) {
    // ---- checkpoints: from the build-time table (beyond it from the host continuation)
    const size_t need_ck = (nsym + OPV_TX_CKPT_SYMS - 1) / OPV_TX_CKPT_SYMS;
    if (c->tx_ckpt_have < need_ck) {
        // (grow-only, by half again: a bank's streams lengthen their runs a frame per round, and a new buffer is filled from entry 0)
        const size_t ck_bytes = sizeof(double) * 2 * need_ck;
        if (c->tx_ckpt.cap < ck_bytes) c->tx_ckpt_have = 0;
        if (int r = c->tx_ckpt.grow(ck_bytes, ck_bytes + ck_bytes / 2, {c->stream})) return r;
        std::vector<double> ck(2 * (need_ck - c->tx_ckpt_have));
        opv_tx_checkpoint_range(c->tx_ckpt_have, need_ck - c->tx_ckpt_have, ck.data());
        HIPCHK(hipMemcpy(c->tx_ckpt.p + 2 * c->tx_ckpt_have, ck.data(), sizeof(double) * ck.size(), hipMemcpyHostToDevice));
        c->tx_ckpt_have = need_ck;
    }
    // ---- flat tops: the zone limits from the checkpoint sequence (the drift is monotone), the bits in between from libm.
    // Both zone limits are statements about THIS process's libm (glibc: exactly 1.0 while eps < 1.05e-8); they are probed once
    // per process (libm_flat_tops_as_assumed), and the partition the binary search relies on is spot-checked. If either fails -
    // another libm, a drift that is not monotone - every symbol's bits come from libm (flat_lo = 0, no upper zone): slower to
    // set up (two sincos per symbol of the run on the host), identical to `opv-mod` on this machine by construction.
    if (c->tx_flat_hi == ~0ull) {                            // (both limits found: final - the sequence is data-independent)
        const size_t n_ck = need_ck;
        auto drift = [](size_t j) {                          // distance of checkpoint j's phases from a multiple of pi/2
            double p[2];
            opv_tx_checkpoint_range(j, 1, p);
            const double q = 1.57079632679489661923;
            const double d1 = std::fabs(p[0] - std::nearbyint(p[0] / q) * q), d2 = std::fabs(p[1] - std::nearbyint(p[1] / q) * q);
            return d1 > d2 ? d1 : d2;
        };
        auto first_at = [&](double thr) -> size_t {         // smallest checkpoint index with drift >= thr, n_ck if none
            size_t lo = 0, hi = n_ck;
            while (lo < hi) { const size_t mid = lo + (hi - lo) / 2; if (drift(mid) >= thr) hi = mid; else lo = mid + 1; }
            return lo;
        };
        const size_t j_lo = n_ck ? first_at(kFlatExact) : 0, j_hi = n_ck ? first_at(kFlatBelow) : 0;
        bool ok = c->tx_trust_libm;
        for (size_t t = 0; ok && n_ck && t < 16; ++t) {     // the partition the search assumed, at 16 places across the run
            const size_t j = t * (n_ck - 1) / 15;
            const double d = drift(j);
            ok = (d >= kFlatExact) == (j >= j_lo) && (d >= kFlatBelow) == (j >= j_hi);
        }
        if (ok) {
            c->tx_flat_lo = j_lo >= n_ck ? ~0ull : (uint64_t)(j_lo ? j_lo - 1 : 0) * OPV_TX_CKPT_SYMS;
            c->tx_flat_hi = j_hi >= n_ck ? ~0ull : (uint64_t)(j_hi + 1) * OPV_TX_CKPT_SYMS;
        } else {
            c->tx_flat_lo = 0;
            c->tx_flat_hi = ~0ull - 1;                       // (not the "unknown" value: final)
        }
    }
    if (c->tx_flat_lo != ~0ull && nsym > c->tx_flat_lo) {
        const uint64_t want = c->tx_flat_hi < (uint64_t)nsym ? c->tx_flat_hi : (uint64_t)nsym;   // bits for [flat_lo, want)
        if (c->tx_flat_have < want) {
            // The symbol-start phases of the zone, replayed on the host from the checkpoints (flat_lo is one: the adds and wraps
            // the device makes), and libm's answer at each. Bits already made stay; a bank's streams cross the zone a frame per
            // round, so the buffer grows by half again and only the new symbols are asked.
            const size_t cnt = (size_t)(want - c->tx_flat_lo);
            size_t from = c->tx_flat_have > c->tx_flat_lo ? (size_t)(c->tx_flat_have - c->tx_flat_lo) : 0;
            if (c->tx_flat.cap < cnt) {
                from = 0;
                c->tx_flat_have = 0;
                if (int r = c->tx_flat.grow(cnt, cnt + cnt / 2, {c->stream})) return r;
            }
            from -= from % OPV_TX_CKPT_SYMS;                                 // (whole intervals: each starts at a checkpoint)
            std::vector<uint8_t> bits(cnt - from);
            const size_t iv0 = from / OPV_TX_CKPT_SYMS, iv1 = (cnt + OPV_TX_CKPT_SYMS - 1) / OPV_TX_CKPT_SYMS, ck0 = (size_t)(c->tx_flat_lo / OPV_TX_CKPT_SYMS);
            auto work = [&](size_t a, size_t b) {                            // checkpoint intervals [a, b) of the zone
                double ph[2 * OPV_TX_CKPT_SYMS];
                for (size_t iv = a; iv < b; ++iv) {
                    const size_t k0 = iv * OPV_TX_CKPT_SYMS, n = cnt - k0 < OPV_TX_CKPT_SYMS ? cnt - k0 : OPV_TX_CKPT_SYMS;
                    double p[2];
                    opv_tx_checkpoint_range(ck0 + iv, 1, p);
                    opv_tx_symbol_phases(0, n, &p[0], &p[1], ph);
                    for (size_t k = 0; k < n; ++k) {
                        const double p1 = ph[2 * k], p2 = ph[2 * k + 1];
                        const bool e1 = std::fabs(std::sin(p1)) == 1.0 || std::fabs(std::cos(p1)) == 1.0;
                        const bool e2 = std::fabs(std::sin(p2)) == 1.0 || std::fabs(std::cos(p2)) == 1.0;
                        bits[k0 + k - from] = (uint8_t)((e1 ? 1 : 0) | (e2 ? 2 : 0));
                    }
                }
            };
            unsigned nt = std::thread::hardware_concurrency();
            if (nt == 0) nt = 1;
            if (nt > 16) nt = 16;
            if (cnt - from < 65536) nt = 1;
            std::vector<std::thread> pool;
            const size_t per = (iv1 - iv0 + nt - 1) / nt;
            for (unsigned t = 1; t < nt; ++t) { const size_t a = iv0 + t * per, b = a + per < iv1 ? a + per : iv1; if (a < b) pool.emplace_back(work, a, b); }
            work(iv0, iv0 + per < iv1 ? iv0 + per : iv1);
            for (auto& th : pool) th.join();
            HIPCHK(hipMemcpy(c->tx_flat.p + from, bits.data(), bits.size(), hipMemcpyHostToDevice));
            c->tx_flat_have = want;
        }
    }
    return OPV_OK;
}

extern "C" long opv_tx_modulate_device(opv_ctx* c, const uint8_t* frames, size_t n_frames, int16_t* d_iq_out) {
    if (!c || !d_iq_out || (!frames && n_frames)) return fail(OPV_EINVAL, "null argument");
    if (((uintptr_t)d_iq_out & 15u) != 0) return fail(OPV_EINVAL, "device IQ pointer must be 16-byte aligned");
    if (n_frames > 0x7FFFFFFFull / OPV_FSYMS) return fail(OPV_EINVAL, "opv_tx_modulate_device: too many frames for one call");
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t nsym = n_frames * OPV_FSYMS, nsym_total = nsym + 100;  // + 100 silent symbols (opv-mod.cpp:528-529)
    constexpr uint32_t kAmbCap = 4096;
    if (int r = opv_tx_prepare_run(c, nsym)) return r;
    // ---- symbol-start phases: from the checkpoints, expanded on the device, once per context and run length
    if (c->tx_phases_have < nsym) {
        const size_t need_ck = (nsym + OPV_TX_CKPT_SYMS - 1) / OPV_TX_CKPT_SYMS;
        size_t first_ck = c->tx_phases_have / OPV_TX_CKPT_SYMS;            // whole intervals already expanded stay
        const size_t ph_bytes = sizeof(double) * 2 * nsym;
        if (c->tx_phases.cap < ph_bytes) c->tx_phases_have = first_ck = 0;
        if (int r = c->tx_phases.grow(ph_bytes, ph_bytes, {c->stream})) return r;   // (an earlier modulation may still read the old table)
        const size_t n_new = need_ck - first_ck;
        k_tx_expand_phases<<<(unsigned)((n_new + 63) / 64), 64, 0, c->stream>>>((const double2*)c->tx_ckpt.p, (uint32_t)need_ck, first_ck,
                                                                                 nsym, (double2*)c->tx_phases.p);
        HIPCHK(hipGetLastError());
        c->tx_phases_have = nsym;
    }
    // ---- scratch (grow-only)
    // three parts of one allocation, each on a 256-byte boundary: [frames][134], one code byte per symbol, a byte per frame
    const size_t fcap = n_frames ? n_frames : 1, codes_off = (fcap * OPV_FB + 255) & ~(size_t)255, fpar_off = codes_off + ((fcap * OPV_FSYMS + 255) & ~(size_t)255);
    if (int r = c->tx_scratch.grow(fpar_off + fcap, fpar_off + fcap, {c->stream})) return r;
    // (carved by THIS call's frame count: a larger buffer of an earlier call is simply used in part)
    uint8_t *const d_tx_frames = c->tx_scratch.p, *const d_tx_codes = c->tx_scratch.p + codes_off, *const d_tx_fpar = c->tx_scratch.p + fpar_off;
    if (!c->d_tx_cnt) HIPCHK(hipMalloc(&c->d_tx_cnt, sizeof(uint32_t)));
    if (!c->d_tx_list) HIPCHK(hipMalloc(&c->d_tx_list, sizeof(uint64_t) * kAmbCap));
    // ---- frames -> code bytes + frame prefixes -> samples, all on the context's stream
    if (n_frames) HIPCHK(hipMemcpyAsync(d_tx_frames, frames, n_frames * OPV_FB, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(c->d_tx_cnt, 0, sizeof(uint32_t), c->stream));
    if (n_frames) {
        k_tx_encode<<<(unsigned)n_frames, 256, 0, c->stream>>>(d_tx_frames, (uint32_t)n_frames, d_tx_codes, d_tx_fpar);
        k_tx_scan_frames<<<1, 1024, 0, c->stream>>>(d_tx_fpar, (uint32_t)n_frames);
    }
    k_tx_modulate<<<(unsigned)((nsym_total + 63) / 64), 64, 0, c->stream>>>(d_tx_codes, d_tx_fpar, (const double2*)c->tx_phases.p, nsym,
                                                                          nsym_total, (int*)d_iq_out, c->d_tx_cnt, c->d_tx_list, kAmbCap,
                                                                          c->tx_flat_lo, c->tx_flat_hi, c->tx_flat.p);
    HIPCHK(hipGetLastError());
    uint32_t n_amb = 0;
    HIPCHK(hipMemcpyAsync(&n_amb, c->d_tx_cnt, sizeof n_amb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));                                // (also: `frames` is the caller's again)
    if (n_amb > kAmbCap) return fail(OPV_ECAPACITY, "too many ambiguous samples (internal)");
    if (n_amb) {  // re-evaluate with libm exactly like the reference: tone / sign and phases of those symbols on the host
        std::vector<uint64_t> list(n_amb);
        HIPCHK(hipMemcpy(list.data(), c->d_tx_list, sizeof(uint64_t) * n_amb, hipMemcpyDeviceToHost));
        std::vector<int8_t> amp(nsym_total, 0);
        opv_tx_symbol_codes(frames, n_frames, amp.data());
        std::vector<double> ph(2 * OPV_TX_CKPT_SYMS);
        for (uint64_t n : list) {
            const size_t sym = n / OPV_SPS, ck = sym / OPV_TX_CKPT_SYMS, in = sym - ck * OPV_TX_CKPT_SYMS;
            double p[2];
            opv_tx_checkpoint_range(ck, 1, p);
            opv_tx_symbol_phases(0, in + 1, &p[0], &p[1], ph.data());
            int16_t iq[2];
            opv_tx_sample_exact(ph[2 * in], ph[2 * in + 1], amp[sym], (int)(n % OPV_SPS), &iq[0], &iq[1]);
            HIPCHK(hipMemcpy(d_iq_out + 2 * n, iq, 4, hipMemcpyHostToDevice));
        }
    }
    return (long)n_amb;
}

extern "C" long opv_tx_modulate_device_to_host(opv_ctx* c, const uint8_t* frames, size_t n_frames, int16_t* iq_out) {
    if (!c || !iq_out) return fail(OPV_EINVAL, "null argument");
    HIPCHK(hipSetDevice(c->cfg.device));
    const size_t n = (n_frames * OPV_FSYMS + 100) * (size_t)OPV_SPS;
    int16_t* d = nullptr;
    HIPCHK(hipMalloc(&d, n * 4));
    long rc = opv_tx_modulate_device(c, frames, n_frames, d);
    if (rc >= 0 && hipMemcpy(iq_out, d, n * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(OPV_EHIP, "D2H of the modulated samples");
    (void)hipFree(d);
    return rc;
}

