// k_wideband_rational.hip — k_wbr_ddc: the DDC bank of the rational wideband front door (include/opv_demod.h, opv_wb_create_rational):
// the wide rate is 2 168 000 x M / U S/s. Per channel: mix at +f_k down to 0 with the closed-form integer LO of k_wb_ddc, then
// resample by U / M - output r reads the J wide samples n_r, n_r - 1, ... (n_r = floor(r M / U)) against row p_r = (r M) mod U of
// the phase-major tap table - round, clamp, and store int16 IQ into each stream's reserved place. Integer-exact and independent of
// summation order (|acc| < 2^52: int64), so parity with the numpy model is `==`.
//
// Shape, as k_wb_ddc: workgroup (x, y) makes outputs [x * tile, + tile) of this push for channels [y * kper, + kper). Its span of
// wide samples - rowlen - 1 in front (J - 1 of them carry weight, the rest meet the zero padding of a tap row), then up to
// floor(tile M / U) + 1 new ones - is fetched ONCE (16 B per lane where the source allows) into LDS; per channel every thread
// mixes its share of the span into a second LDS array, then lane l accumulates output l over its row of taps.
//
// LDS layout. Lanes of neighbouring outputs read samples floor((l + 1) M / U) - floor(l M / U) apart: M / U on average, anything
// from 1 to 32 and not an integer, so no layout by phase (k_wb_ddc's) makes them neighbours. The span stays in sample order and
// the mixed array is padded by one entry per 32: entry j lives at j + (j >> 5). An entry is 8 bytes (ds_read_b64: 64 banks of 4 B,
// 32 lanes per access). At a stride of s entries, s a power of two up to 32, 32 / s lanes share a block of 32 entries and the next
// block starts one entry (two banks) later: lane l sits at bank 2 (s l mod 32) + 2 (s l / 32), and those are 32 distinct even
// banks. Without the pad a stride of 32 puts all 32 lanes on one bank. The tap rows live in global memory (up to 2^20 entries):
// lane l walks its own row, 8 bytes at a time.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opv_wb_internal.h"

namespace {

constexpr uint32_t kMixedLen = OPV_WB_SPAN + OPV_WB_SPAN / 32;

__device__ __forceinline__ uint32_t mixed_slot(uint32_t j) { return j + (j >> 5); }

}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_wbr_ddc(OpvWbrArgs a) {
    __shared__ int raw[OPV_WB_SPAN];          // packed int16 I | Q << 16, in sample order
    __shared__ int2 mixed[kMixedLen];         // (mr, mi) of the channel in hand, padded (above)
    __shared__ int16_t lo[4096];
    const uint32_t tid = threadIdx.x;
    const uint32_t M = a.M, U = a.U, J = a.J, rowlen = a.rowlen;

    // the carry of the NEXT push: the last J - 1 samples of (carry, this push). It goes to the other buffer, so nobody's reads race it.
    if (blockIdx.x == 0 && blockIdx.y == 0) {
        const uint64_t have = a.n_before + a.n_new;
        const uint32_t keep = have < (uint64_t)(J - 1) ? (uint32_t)have : J - 1;
        const uint32_t from = a.hist_len + a.n_new - keep;             // index into (hist_in, src) laid end to end
        for (uint32_t i = tid; i < keep; i += OPV_WB_THREADS) {
            const uint32_t ci = from + i;
            a.hist_out[i] = ci < a.hist_len ? a.hist_in[ci] : a.src[ci - a.hist_len];
        }
    }
    const uint64_t out0 = (uint64_t)blockIdx.x * a.tile;               // first output of this workgroup, within the push
    if (out0 >= a.n_out) return;
    const uint32_t cnt = a.n_out - out0 < a.tile ? (uint32_t)(a.n_out - out0) : a.tile;

    // output out0 + l of the push: (p_r0 + (out0 + l) M) / U wide samples behind n_r0, remainder = its phase. 64 bits once per
    // workgroup for out0; per lane pbase + l M < 2^10 + 2^8 2^15 stays in 32.
    const uint64_t t0 = (uint64_t)a.p0 + out0 * M;
    const uint64_t q0 = t0 / U;
    const uint32_t pbase = (uint32_t)(t0 - q0 * U);
    const uint32_t front = rowlen - 1;
    const uint32_t span = front + (pbase + (cnt - 1) * M) / U + 1;     // <= rowlen + floor(tile M / U) <= OPV_WB_SPAN by the host's tile
    if (span > OPV_WB_SPAN) return;                                    // (a plan the host would not make: touch nothing)

    for (uint32_t i = tid; i < 4096; i += OPV_WB_THREADS) lo[i] = a.lo[i];

    // local sample j of the span is src[base_i + j]; the newest sample of output out0 + l is local sample front + dn_l
    const int64_t base_i = (int64_t)((uint64_t)a.nrel0 + q0) - (int64_t)front;
    // (1) what lies in front of this push (the carry, zeros before sample 0) and behind it (zeros: no output of this push reads them)
    for (uint32_t j = tid; j < span; j += OPV_WB_THREADS) {
        const int64_t i = base_i + (int64_t)j;
        if (i < 0) {
            const int64_t h = (int64_t)a.hist_len + i;
            raw[j] = h >= 0 ? a.hist_in[h] : 0;
        } else if (i >= (int64_t)a.n_new) {
            raw[j] = 0;
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
                    raw[j] = v.x;
                    raw[j + 1] = v.y;
                    raw[j + 2] = v.z;
                    raw[j + 3] = v.w;
                } else {
                    for (int64_t e = i; e < i + 4; ++e)
                        if (e >= i_lo && e < i_end) raw[(uint32_t)(e - base_i)] = a.src[e];
                }
            }
        }
    }
    __syncthreads();

    // phase of local sample j: phi = (uint32)((first_sample + n) * inc) - the low 32 bits only, so 32-bit arithmetic that wraps
    const uint32_t a_base = a.a0_lo + (uint32_t)(uint64_t)base_i;
    const uint32_t k_end = (blockIdx.y + 1) * a.kper < a.K ? (blockIdx.y + 1) * a.kper : a.K;
    const int64_t half = a.S ? (int64_t)1 << (a.S - 1) : 0;
    const uint32_t tl = pbase + (tid < cnt ? tid : 0u) * M;
    const uint32_t dn = tl / U;
    const uint32_t top = front + dn;                                    // tap j reads local sample top - j >= dn >= 0
    const int2* row = (const int2*)(a.tab + (size_t)(tl - dn * U) * rowlen);   // 4 taps per 8 bytes
    for (uint32_t k = blockIdx.y * a.kper; k < k_end; ++k) {
        const uint32_t inc = a.inc[k];
        for (uint32_t j = tid; j < span; j += OPV_WB_THREADS) {
            const uint32_t phi = (a_base + j) * inc;
            const uint32_t ix = phi >> 20;
            const int c = lo[ix], s = lo[(ix - 1024u) & 4095u];
            const int x = raw[j];
            const int I = (int16_t)(x & 0xFFFF), Q = x >> 16;
            mixed[mixed_slot(j)] = make_int2(I * c + Q * s, Q * c - I * s);
        }
        __syncthreads();
        if (tid < cnt) {
            int64_t ar = 0, ai = 0;
            for (uint32_t j = 0; j < rowlen; j += 4) {
                const int2 h4 = row[j >> 2];
                const int h[4] = {(int16_t)(h4.x & 0xFFFF), h4.x >> 16, (int16_t)(h4.y & 0xFFFF), h4.y >> 16};
#pragma unroll
                for (uint32_t e = 0; e < 4; ++e) {
                    const int2 m = mixed[mixed_slot(top - j - e)];
                    ar += (int64_t)h[e] * m.x;
                    ai += (int64_t)h[e] * m.y;
                }
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
