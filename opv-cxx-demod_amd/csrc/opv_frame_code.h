// opv_frame_code.h — the frame code, one definition per rule: randomiser table, K=7 r=1/2 polynomials, 67x32 interleaver address,
// the decoder's 3-bit quantiser and the per-lane gather of a payload. Plain C++17 for g++ and for hipcc, host and device alike:
// the host modulator (opv_tx.cpp), the device one (k_tx_modulate.hip), the decoder (k_frame_decode.hip) and the link report
// (k_frame_link.hip) all read these, so what one side encodes is by construction what the other side expects.
// Line cites: reference src/opv-mod.cpp (transmit) and src/opv-demod.cpp ("ref", receive). The sync word is OPV_SYNC_WORD (opv_device.h).
#pragma once
#include <math.h>
#include <stdint.h>

#include "opv_device.h"

#ifdef __HIPCC__
#define OPV_HD __host__ __device__
#else
#define OPV_HD
#endif

#ifdef OPV_DEMOD_H   // the public header's names for the same sizes
static_assert(OPV_FB == OPV_FRAME_BYTES && OPV_FBITS == OPV_FRAME_BITS && OPV_CODED == OPV_ENCODED_BITS && OPV_FSYMS == OPV_FRAME_SYMBOLS &&
              OPV_SPS == OPV_SAMPLES_PER_SYMBOL, "opv_device.h and include/opv_demod.h agree on the frame");
#endif

// the CCSDS randomiser's byte sequence (opv-mod.cpp:97-113, ref :887-893: state 0xFF, taps 7 6 4 2, MSB first, reset per frame):
// a constant table. Every code object keeps its own `__constant__ OpvLfsrTable ... = opv_make_lfsr();`
struct OpvLfsrTable { uint8_t b[OPV_FB]; };
constexpr OpvLfsrTable opv_make_lfsr() {
    OpvLfsrTable t{};
    unsigned st = 0xFF;
    for (int i = 0; i < OPV_FB; ++i) {
        unsigned v = 0;
        for (int k = 0; k < 8; ++k) {
            v = (v << 1) | ((st >> 7) & 1u);
            st = ((st << 1) | (((st >> 7) ^ (st >> 6) ^ (st >> 4) ^ (st >> 2)) & 1u)) & 0xFFu;
        }
        t.b[i] = (uint8_t)v;
    }
    return t;
}

// the interleaver's address map: 67 x 32, low three bits reversed (opv-mod.cpp:145-149, ref :792-795). ONE function for both
// directions: the transmit side writes coded bit i to on-air position opv_interleave_addr(i), the receive side reads value i of
// the decoder's input from payload symbol opv_interleave_addr(i).
OPV_HD inline uint32_t opv_interleave_addr(uint32_t i) {
    const uint32_t p = (i & 31u) * 67u + (i >> 5);
    return (p & ~7u) + (7u - (p & 7u));
}

// the code's two polynomials on reg = (in << 6) | sr: the step's input bit on top of the six-bit state, whose bit 0 is the newest
// earlier bit (opv-mod.cpp:124-128, ref :819-824). G1 gives code bit 2 t, G2 code bit 2 t + 1.
#define OPV_CODE_G1 0x4Fu
#define OPV_CODE_G2 0x6Du
OPV_HD inline unsigned opv_code_g1(unsigned reg) { return (unsigned)__builtin_parity(reg & OPV_CODE_G1); }
OPV_HD inline unsigned opv_code_g2(unsigned reg) { return (unsigned)__builtin_parity(reg & OPV_CODE_G2); }

// The quantiser (ref :862-866: q = 0 confident bit 0 ... q = 7 confident bit 1) behind the frame's scale; inv = -3.5 / scale.
// The reference's expression per value (:864-865) is int((-soft / scale) * 3.5 + 3.5 + 0.5), four rounded operations of which
// the IEEE division alone costs a wave ~30 fp64 instructions. Its result is decided by ONE multiply-add,
// x = fma(soft, -3.5 / scale, 4.0), whenever x is not within 1e-6 of an integer: both expressions are within ~1e-14 of
// the exact value 4 - 3.5 soft / scale for |x| < 9 (|soft / scale| <= 2144 while the scale is finite: nothing overflows), hence
// they truncate alike unless the exact value is within 1e-14 of an integer - and then x is within the guard band and the
// reference's own sequence is evaluated (about one value in 10^5 on noise; every value of a few-level input). Outside
// (-1, 9) both clamp to the same end. An infinite scale (an Inf in the payload, a sum that overflows) gives x = 4.0, in the band,
// or NaN; NaN converts to 0 on both paths like the reference's cvttsd2si + clamp (tests/test_gpu_soft_log.py holds all of it).
// Every TU that calls this is compiled with -ffp-contract=off. The value before the clamp to 0..7 is a function of its own for
// the link report, whose thresholds (>= 4; 3 or 4) cannot see the clamp: asked for the clamped value, hipcc keeps 68 v_med3_i32
// per frame and lane in k_frame_link that decide nothing.
OPV_HD inline int opv_quantise3_unclamped(double soft, double scale, double inv) {
    const double x = fma(soft, inv, 4.0);
    int v = (int)x;
    if (__builtin_expect(fabs(x - rint(x)) < 1.0e-6 && x > -1.0 && x < 9.0, 0)) {
        const double nrm = (-soft / scale) * 3.5 + 3.5;
        v = (int)(nrm + 0.5);                                     // C truncation toward zero
    }
    return v;
}
OPV_HD inline int opv_quantise3(double soft, double scale, double inv) {
    const int v = opv_quantise3_unclamped(soft, scale, inv);
    return v < 0 ? 0 : (v > 7 ? 7 : v);
}

#ifdef __HIPCC__
// Device only (`lane` is a wavefront's). A lane's share of a payload = soft[(first + i) & mask], i < 2144: both code bits of trellis
// steps t = lane, lane + 64, ... (17 steps, the last for lanes < 48 only), through the address map. All 34 loads (from L2 / HBM)
// are requested before the first is used: a wave that waited for them one trellis step at a time spent 30 000 cycles here
// (17 round trips), more than in the trellis.
constexpr int kLaneSteps = (OPV_FBITS + 63) / 64;
__device__ inline void opv_gather_payload(const double* __restrict__ soft, uint32_t first, uint32_t mask, int lane, double (&sv)[2 * kLaneSteps]) {
#pragma unroll
    for (int k = 0; k < kLaneSteps; ++k) {
        const int t = lane + 64 * k;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const uint32_t a = opv_interleave_addr(2u * (uint32_t)(t < OPV_FBITS ? t : 0) + (uint32_t)h);
            sv[2 * k + h] = soft[(first + a) & mask];
        }
    }
}
#endif
