// k_tx_modulate.hip — the OPV transmit chain on the device: everything `opv-mod` does between a
// 134-byte frame and int16 I/Q (reference src/opv-mod.cpp:97-291), written for HBM. Four kernels:
//
//   k_tx_encode         one workgroup per FRAME: CCSDS randomiser (:97-113), K=7 r=1/2 encoder (:120-136; last byte first,
//                       MSB first :186-196), 67x32 interleaver with in-byte bit reversal (:142-153), sync word in front
//                       (:315-321) -> one code byte per on-air symbol: bit 0 = the symbol's bit, bit 1 = XOR of the frame's
//                       bits in front of it; + the frame's parity. The encoder is a sliding window (coded bit t depends on
//                       input bits t-6..t only), so all 1072 steps of a frame run in parallel.
//   k_tx_scan_frames    exclusive XOR scan of the frame parities: the modulator's differential sign T' = d T
//                       (:232-239) is a running +/-1 product over the whole run, i.e. a parity prefix.
//   k_tx_expand_phases  the two NCOs free-run through every sample with rounded additions (:274-279): data-independent but
//                       strictly sequential. Their state at every 128th symbol is tabulated at build time
//                       (tools/gen_tx_checkpoints.cpp); one thread per table entry replays the 128 x 40 additions that
//                       follow (bit-identical IEEE adds and wraps) and leaves (ph1, ph2) at every symbol start. Once per
//                       context and run length; every stream modulated afterwards shares it.
//   k_tx_modulate       one thread per symbol: tone / sign from the code byte and the frame prefix (:241-257), 40 samples
//                       with sin / cos of the ACTIVE tone only, truncation like the reference (:268-272), 64 symbols per
//                       workgroup staged through LDS so that HBM sees 16-byte-per-lane stores (4 B/sample, nothing else).
//
// Exactness: device sincos and glibc agree to ~1 ulp, so 16383*x can only truncate differently when it lies within ~1e-11
// of an integer. Such samples (none in practice) are reported in a small list and re-evaluated by the host with libm, so
// the result is identical to `opv-mod` by construction, not by luck.
// One place is not "in practice none": the FLAT TOPS. A symbol lasts a quarter period of either tone, so at every symbol
// start sin or cos of each NCO sits at +/-1 up to the phase's accumulated rounding drift eps (6.74e-12 rad per frame, from
// the recurrence itself: data-independent and monotone), i.e. at 1 - eps^2/2 - and 16383 x truncates to 16383 only if the
// library returns exactly 1.0. glibc does while eps^2/2 < 2^-54 (eps < 1.05e-8: 1563 frames into a run) and returns
// 1 - 2^-53 from there on (16382). The kernel therefore decides flat tops by the symbol index, not by its own sincos:
// 16383 before `flat_lo` (eps < 0.90e-8: within 0.37 ulp of 1.0), 16382 from `flat_hi` on (eps > 1.25e-8: 0.70 ulp below),
// and in the ~500 frames between by a bit per symbol and tone that the host made with libm itself (opv_capi.hip; once per
// context and run length). tests/test_capi_and_host.py::test_flat_top_zones_hold_for_this_libm scans both zones on the
// host's libm.
//
// Roofline: HBM write, 4 B/sample (a 1000-frame run: 347 MB); the phase table adds 16 B/symbol of reads (35 MB).
// The frame code of k_tx_encode and the sample loop of k_tx_modulate live in k_tx_common.h: the transmit bank (k_tx_bank.hip) runs the same two.
#include "k_tx_common.h"

// frames: [n_frames][134]; codes: [n_frames * 2168] (bit 0: symbol bit, bit 1: parity of the frame's bits before it);
// frame_par: [n_frames] parity of all 2168 bits of the frame
extern "C" __global__ __launch_bounds__(256) void k_tx_encode(const uint8_t* __restrict__ frames, uint32_t n_frames,
                                                               uint8_t* __restrict__ codes, uint8_t* __restrict__ frame_par) {
    const uint32_t f = blockIdx.x;
    if (f >= n_frames) return;
    tx_encode_frame(frames + (size_t)f * OPV_FB, codes + (size_t)f * OPV_FSYMS, frame_par + f);
}

// in place: frame_par[f] <- XOR of the parities of frames 0..f-1 (one workgroup; runs of any length in slices of 1024)
extern "C" __global__ __launch_bounds__(1024) void k_tx_scan_frames(uint8_t* __restrict__ frame_par, uint32_t n_frames) {
    __shared__ uint32_t s[1024];
    __shared__ uint32_t carry_s;
    const int tid = threadIdx.x;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_frames; base += 1024u) {
        const uint32_t i = base + tid;
        const uint32_t own = i < n_frames ? frame_par[i] : 0u;
        s[tid] = own;
        __syncthreads();
        for (int off = 1; off < 1024; off <<= 1) {
            const uint32_t v = tid >= off ? s[tid - off] : 0u;
            __syncthreads();
            s[tid] ^= v;
            __syncthreads();
        }
        const uint32_t carry = carry_s;
        if (i < n_frames) frame_par[i] = (uint8_t)(s[tid] ^ own ^ carry);
        __syncthreads();
        if (tid == 1023) carry_s = carry ^ s[1023];
        __syncthreads();
    }
}

// ckpt: [n_ckpt] (ph1, ph2) at symbol j * OPV_TX_CKPT_SYMS; phases: [nsym] (ph1, ph2) at every symbol start
extern "C" __global__ __launch_bounds__(64) void k_tx_expand_phases(const double2* __restrict__ ckpt, uint32_t n_ckpt,
                                                                     uint64_t first_ckpt, uint64_t nsym,
                                                                     double2* __restrict__ phases) {
    const uint64_t j = first_ckpt + (uint64_t)blockIdx.x * 64u + threadIdx.x;
    if (j >= n_ckpt) return;
    double2 p = ckpt[j];
    const uint64_t s0 = j * OPV_TX_CKPT_SYMS;
    for (uint32_t s = 0; s < OPV_TX_CKPT_SYMS && s0 + s < nsym; ++s) {
        phases[s0 + s] = p;
        for (int i = 0; i < OPV_SPS; ++i) { advance(p.x, kInc1); advance(p.y, kInc2); }
    }
}

// codes: [nsym] from k_tx_encode, frame_pre: [n_frames] from k_tx_scan_frames, phases: [nsym] (ph1, ph2) pairs;
// symbols nsym .. nsym_total-1 are the silent tail (opv-mod.cpp:528-529); out: packed int16 I | Q << 16
extern "C" __global__ __launch_bounds__(64) void k_tx_modulate(const uint8_t* __restrict__ codes,
                                                                const uint8_t* __restrict__ frame_pre,
                                                                const double2* __restrict__ phases, uint64_t nsym,
                                                                uint64_t nsym_total, int* __restrict__ out,
                                                                uint32_t* __restrict__ amb_count,
                                                                uint64_t* __restrict__ amb_list, uint32_t amb_cap,
                                                                uint64_t flat_lo, uint64_t flat_hi,
                                                                const uint8_t* __restrict__ flat_bits) {
    __shared__ __attribute__((aligned(16))) int stage[64 * OPV_SPS];
    const uint64_t sym0 = (uint64_t)blockIdx.x * 64u;
    const uint64_t sym = sym0 + threadIdx.x;
    int a = 0;                                      // +/-1: tone 1 with that sign, +/-2: tone 2, 0: silent
    double ph1 = 0.0, ph2 = 0.0;
    if (sym < nsym && sym != 0) {                   // (symbol 0: T = 0 right after the modulator's reset, :221-226 - silent)
        a = tx_symbol_code(codes[sym], frame_pre[sym / OPV_FSYMS], sym);
        const double2 p = phases[sym];
        ph1 = p.x; ph2 = p.y;
    }
    tx_symbol_samples(a, ph1, ph2, sym, flat_lo, flat_hi, flat_bits, stage + threadIdx.x * OPV_SPS, [&](int i) {
        const uint32_t k = atomicAdd(amb_count, 1u);
        if (k < amb_cap) amb_list[k] = sym * OPV_SPS + (uint64_t)i;
    });
    __syncthreads();
    // 64 symbols x 40 samples = 2560 dwords = 10 x (64 lanes x 16 B)
    const uint64_t base = sym0 * OPV_SPS;
    const uint64_t total = nsym_total * OPV_SPS;
    const int4* s4 = reinterpret_cast<const int4*>(stage);
    int4* o4 = reinterpret_cast<int4*>(out + base);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const int q = r * 64 + threadIdx.x;
        if (base + 4u * q + 3u < total) o4[q] = s4[q];
    }
}
