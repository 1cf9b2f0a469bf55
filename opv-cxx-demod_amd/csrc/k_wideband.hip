// k_wideband.hip — k_wb_ddc: the wideband front door's DDC bank (include/opv_demod.h, opv_wb_*). One launch per push serves all K
// channels: mix each channel at +f_k down to 0 with a closed-form integer LO, filter with int16 taps, decimate by D, round, clamp,
// and store int16 IQ straight into each stream's reserved place in its device buffer. The arithmetic is integer-exact and
// independent of summation order (|acc| < 2^52: int64 here), so parity with the numpy model is `==`.
//
// Shape: workgroup (x, y) makes outputs [r0 + x * tile, + tile) of channels [y * kper, + kper). Its span of wide samples -
// tile * D new ones + the L - 1 in front - is fetched ONCE (16 B per lane where the source allows) into LDS and reused for every
// channel and tap. Per channel: every thread mixes its share of the span into a second LDS array (4 multiplies per sample, not
// per tap), then lane l accumulates output l over the L taps. Both arrays are laid out by decimation phase - local sample
// j = row * D + p lives at p * rowlen + row - so that lanes of neighbouring outputs (D samples apart) read neighbouring LDS words
// at every tap, whatever D is.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opv_wb_internal.h"

namespace {

// j / D for j < 4096 + 16 and 1 <= D <= 16 without a divide: m = ceil(2^16 / D) overshoots 2^16 / D by e / D with e = m D - 2^16 < D,
// so j m >> 16 is exact while j e < 2^16, and (4096 + 16) * 15 < 65536.
__device__ __forceinline__ uint32_t lds_slot(uint32_t j, uint32_t D, uint32_t m, uint32_t rowlen) {
    const uint32_t row = (j * m) >> 16;
    return (j - row * D) * rowlen + row;
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_wb_ddc(OpvWbArgs a) {
    __shared__ int raw[OPV_WB_SPAN];          // packed int16 I | Q << 16
    __shared__ int2 mixed[OPV_WB_SPAN];       // (mr, mi) of the channel in hand
    __shared__ int16_t lo[4096];
    const uint32_t tid = threadIdx.x;
    const uint32_t D = a.D, L = a.L, rowlen = a.rowlen, span = D * rowlen;
    const uint32_t recip = (65536u + D - 1u) / D;

    // the carry of the NEXT push: the last L - 1 samples of (carry, this push). It goes to the other buffer, so nobody's reads race it.
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        const uint64_t have = a.n_before + a.n_new;
        const uint32_t keep = have < (uint64_t)(L - 1) ? (uint32_t)have : L - 1;
        const uint32_t from = a.hist_len + a.n_new - keep;             // index into (hist_in, src) laid end to end
        for (uint32_t i = tid; i < keep; i += OPV_WB_THREADS) {
            const uint32_t ci = from + i;
            a.hist_out[i] = ci < a.hist_len ? a.hist_in[ci] : a.src[ci - a.hist_len];
        }
    }
    const uint64_t out0 = (uint64_t)blockIdx.x * a.tile;               // first output of this workgroup, within the push
    if (out0 >= a.n_out) return;
    const uint32_t cnt = a.n_out - out0 < a.tile ? (uint32_t)(a.n_out - out0) : a.tile;

    for (uint32_t i = tid; i < 4096; i += OPV_WB_THREADS) lo[i] = a.lo[i];

    // local sample j of the span is sample n = (r0 + out0) * D - lpad + j of the object, i.e. src[base_i + j]
    const int64_t base_i = (int64_t)((a.r0 + out0) * D) - (int64_t)a.lpad - (int64_t)a.n_before;
    // (1) what lies in front of this push (the carry, zeros before sample 0) and behind it (zeros: no output of this push reads them)
    for (uint32_t j = tid; j < span; j += OPV_WB_THREADS) {
        const int64_t i = base_i + (int64_t)j;
        if (i < 0) {
            const int64_t h = (int64_t)a.hist_len + i;
            raw[lds_slot(j, D, recip, rowlen)] = h >= 0 ? a.hist_in[h] : 0;
        } else if (i >= (int64_t)a.n_new) {
            raw[lds_slot(j, D, recip, rowlen)] = 0;
        }
    }
    // (2) the part inside this push, in 16-byte pieces of the source wherever a whole piece lies inside both the push and the span
    {
        const int64_t i_lo = base_i > 0 ? base_i : 0;
        const int64_t i_end = base_i + (int64_t)span < (int64_t)a.n_new ? base_i + (int64_t)span : (int64_t)a.n_new;
        if (i_end > i_lo) {
            const int64_t mis = (int64_t)(((uintptr_t)a.src >> 2) & 3u);   // src[4 q - mis] is 16-byte aligned
            const int64_t q_lo = (i_lo + mis) >> 2, q_hi = (i_end - 1 + mis) >> 2;
            for (int64_t q = q_lo + tid; q <= q_hi; q += OPV_WB_THREADS) {
                const int64_t i = 4 * q - mis;
                if (i >= i_lo && i + 4 <= i_end) {
                    const int4 v = *(const int4*)(a.src + i);
                    const uint32_t j = (uint32_t)(i - base_i);
                    raw[lds_slot(j, D, recip, rowlen)] = v.x;
                    raw[lds_slot(j + 1, D, recip, rowlen)] = v.y;
                    raw[lds_slot(j + 2, D, recip, rowlen)] = v.z;
                    raw[lds_slot(j + 3, D, recip, rowlen)] = v.w;
                } else {
                    for (int64_t e = i; e < i + 4; ++e)
                        if (e >= i_lo && e < i_end) raw[lds_slot((uint32_t)(e - base_i), D, recip, rowlen)] = a.src[e];
                }
            }
        }
    }
    __syncthreads();

    // phase of local sample j: phi = (uint32)((first_sample + n) * inc) - the low 32 bits only, so 32-bit arithmetic that wraps
    const uint32_t a_base = a.a0_lo + (uint32_t)(uint64_t)base_i;
    const uint32_t k_end = (blockIdx.y + 1) * a.kper < a.K ? (blockIdx.y + 1) * a.kper : a.K;
    const uint32_t u_lo = a.lpad - (L - 1);                             // tap t reads local sample lane * D + (lpad - t)
    const int64_t half = a.S ? (int64_t)1 << (a.S - 1) : 0;
    for (uint32_t k = blockIdx.y * a.kper; k < k_end; ++k) {
        const uint32_t inc = a.inc[k];
        for (uint32_t p = 0; p < D; ++p) {
            for (uint32_t row = tid; row < rowlen; row += OPV_WB_THREADS) {
                const uint32_t phi = (a_base + row * D + p) * inc;
                const uint32_t ix = phi >> 20;
                const int c = lo[ix], s = lo[(ix - 1024u) & 4095u];
                const int x = raw[p * rowlen + row];
                const int I = (int16_t)(x & 0xFFFF), Q = x >> 16;
                mixed[p * rowlen + row] = make_int2(I * c + Q * s, Q * c - I * s);
            }
        }
        __syncthreads();
        if (tid < cnt) {
            int64_t ar = 0, ai = 0;
            uint32_t p = u_lo % D, row = u_lo / D + tid;
            for (uint32_t t = L; t-- > 0;) {                            // u = lpad - t runs upwards: (p, row) step without a divide
                const int2 m = mixed[p * rowlen + row];
                const int64_t h = a.taps[t];
                ar += h * m.x;
                ai += h * m.y;
                if (++p == D) { p = 0; ++row; }
            }
            ar = (ar + half) >> a.S;                                    // floor((acc + 2^(S-1)) / 2^S): an arithmetic shift
            ai = (ai + half) >> a.S;
            ar = ar < -32768 ? -32768 : ar > 32767 ? 32767 : ar;
            ai = ai < -32768 ? -32768 : ai > 32767 ? 32767 : ai;
            a.dst[k][out0 + tid] = (int)(((uint32_t)ai << 16) | ((uint32_t)ar & 0xFFFFu));
        }
        __syncthreads();
    }
}
