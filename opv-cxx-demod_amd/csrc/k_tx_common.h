// k_tx_common.h — the two bodies that the transmit kernels of one run (k_tx_modulate.hip) and of a bank of runs
// (k_tx_bank.hip) share: a frame's code bytes, and a symbol's 40 samples. One definition each; the kernels differ only in
// where a frame comes from, which symbol of which run a thread owns and where its samples go.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "opv_device.h"
#include "opv_frame_code.h"
#include "opv_tx_internal.h"

namespace {
static_assert(((OPV_SYNC_WORD >> 23) & 1u) == 0u, "symbol 0 of a run (first sync bit) is taken to be 0: it never enters the sign product");
static_assert(OPV_FSYMS % 2 == 0, "b_n toggles per symbol: a frame's first symbol always sees b_n = 1");
__constant__ OpvLfsrTable kTxLfsr = opv_make_lfsr();

// One workgroup of 256 threads, one frame: p = its 134 bytes; out[2168]: one code byte per on-air symbol (bit 0: the symbol's
// bit, bit 1: parity of the frame's bits in front of it); *par_out: parity of all 2168 bits of the frame
__device__ inline void tx_encode_frame(const uint8_t* __restrict__ p, uint8_t* __restrict__ out, uint8_t* __restrict__ par_out) {
    __shared__ uint8_t u[OPV_FBITS];                // encoder input bits in encoding order
    __shared__ uint8_t sym[OPV_FSYMS + 8];          // on-air bits: 24 sync + 2144 interleaved coded
    __shared__ uint32_t part[256];
    const int tid = threadIdx.x;
    if (tid < OPV_FB) {
        // byte 133 goes first, MSB first (opv-mod.cpp:186-196): input bit t = bit (7 - t % 8) of byte (133 - t / 8)
        const unsigned v = p[tid] ^ kTxLfsr.b[tid];
        const int t0 = 8 * (OPV_FB - 1 - tid);
#pragma unroll
        for (int b = 0; b < 8; ++b) u[t0 + b] = (uint8_t)((v >> (7 - b)) & 1u);
    }
    if (tid < OPV_SYNC_BITS) sym[tid] = (uint8_t)((OPV_SYNC_WORD >> (23 - tid)) & 1u);
    __syncthreads();
    for (int t = tid; t < OPV_FBITS; t += 256) {
        // reg = (in << 6) | sr, sr bit k = input bit t - 1 - k (zero before the frame: the encoder is reset per frame, :161)
        unsigned reg = (unsigned)u[t] << 6;
#pragma unroll
        for (int k = 0; k < 6; ++k)
            if (t - 1 - k >= 0) reg |= (unsigned)u[t - 1 - k] << k;
        const unsigned g1 = opv_code_g1(reg), g2 = opv_code_g2(reg);
#pragma unroll
        for (int h = 0; h < 2; ++h)                                                  // coded bit 2 t + h, order g1, g2
            sym[OPV_SYNC_BITS + opv_interleave_addr(2u * (uint32_t)t + (uint32_t)h)] = (uint8_t)(h ? g2 : g1);
    }
    __syncthreads();
    // exclusive parity prefix over the frame's 2168 bits: 9 consecutive symbols per thread, scan of the 256 partials
    constexpr int kPer = (OPV_FSYMS + 255) / 256;
    const int k0 = tid * kPer;
    uint32_t mine = 0;
    for (int k = k0; k < k0 + kPer && k < OPV_FSYMS; ++k) mine ^= sym[k];
    part[tid] = mine;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t v = tid >= off ? part[tid - off] : 0u;
        __syncthreads();
        part[tid] ^= v;
        __syncthreads();
    }
    uint32_t run = part[tid] ^ mine;                // exclusive prefix of this thread's first symbol
    for (int k = k0; k < k0 + kPer && k < OPV_FSYMS; ++k) {
        out[k] = (uint8_t)(sym[k] | (run << 1));
        run ^= sym[k];
    }
    if (tid == 255) *par_out = (uint8_t)part[255];
}

// tone / sign of a symbol that is not symbol 0 of its run: +/-1 tone 1 with that sign, +/-2 tone 2. c: its code byte;
// before: parity of the run's bits in front of its frame; sym: its index in the run
__device__ inline int tx_symbol_code(unsigned c, unsigned before, uint64_t sym) {
    // T(k) = prod_{0<j<k} d_j, d = -1 for a 1 bit (:232-239): its sign is the parity of the bits in front of the symbol
    const int T = ((before ^ (c >> 1)) & 1u) ? -1 : 1;
    if ((c & 1u) == 0u) return T;                                           // bit 0: d_s1 = T (:241-245)
    return 2 * ((sym & 1u) ? -T : T);                                       // bit 1: d_s2 = -/+T by b_n (:246-257); b_n = 0 on odd symbols
}

// The 40 samples of symbol `sym` of a run into mine[40] (packed int16 I | Q << 16). a: +/-1 tone 1 with that sign, +/-2 tone 2,
// 0 silent; (ph1, ph2): the NCOs at the symbol's start. ambiguous(i): sample i could truncate differently under the host's libm.
template <class Amb>
__device__ inline void tx_symbol_samples(int a, double ph1, double ph2, uint64_t sym, uint64_t flat_lo, uint64_t flat_hi,
                                         const uint8_t* __restrict__ flat_bits, int* mine, Amb ambiguous) {
    if (a == 0) {
        for (int i = 0; i < OPV_SPS; ++i) mine[i] = 0;
        return;
    }
    const bool tone1 = (a == 1 || a == -1);
    const double sgn = (a > 0) ? 1.0 : -1.0;
    for (int i = 0; i < OPV_SPS; ++i) {
        double sn, cs;
        sincos(tone1 ? ph1 : ph2, &sn, &cs);
        const double vi = 16383.0 * (sgn * sn), vq = 16383.0 * (sgn * cs);  // opv-mod.cpp:268-272
        int I = (int)vi, Q = (int)vq;                                         // truncation toward zero
        // a flat top (k_tx_modulate.hip's file comment): |sin| or |cos| = 1 - eps^2/2; whether libm's value IS 1.0 is a
        // function of the symbol index
        const bool top_i = fabs(vi) > 16382.5, top_q = fabs(vq) > 16382.5;
        if (top_i | top_q) {
            int mag = 16383;
            if (sym >= flat_hi) mag = 16382;
            else if (sym >= flat_lo) mag = ((flat_bits[sym - flat_lo] >> (tone1 ? 0 : 1)) & 1u) ? 16383 : 16382;
            if (top_i) I = vi < 0.0 ? -mag : mag;
            else Q = vq < 0.0 ? -mag : mag;
        }
        mine[i] = (I & 0xFFFF) | (Q << 16);
        // Could libm's value truncate differently? Only if v sits within the two libraries' ~1e-11
        // disagreement of a NON-ZERO integer without being exactly on it (|v| < 1 truncates to 0
        // from either side); the flat tops are decided above.
        const double ri = rint(vi), rq = rint(vq);
        if ((!top_i && ri != 0.0 && vi != ri && fabs(vi - ri) < 1e-9) || (!top_q && rq != 0.0 && vq != rq && fabs(vq - rq) < 1e-9)) ambiguous(i);
        advance(ph1, kInc1);
        advance(ph2, kInc2);
    }
}
}  // namespace
