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

#include "k_wideband_common.h"
#include "opv_wb_internal.h"

namespace {

constexpr uint32_t kMixedLen = OPV_WB_SPAN + OPV_WB_SPAN / 32;

__device__ __forceinline__ uint32_t mixed_slot(uint32_t j) { return j + (j >> 5); }

// the kernel's body, once for both sources of the LO (k_wideband_common.h: WbLoFixed, WbLoTuned)
template <class Lo>
__device__ __forceinline__ void wbr_ddc(const OpvWbrArgs a, const typename Lo::Table* lo_table, uint32_t lo_base) {
    __shared__ int raw[OPV_WB_SPAN];          // packed int16 I | Q << 16, in sample order
    __shared__ int2 mixed[kMixedLen];         // (mr, mi) of the channel in hand, padded (above)
    __shared__ int16_t lo[4096];
    const uint32_t tid = threadIdx.x;
    const uint32_t M = a.M, U = a.U, J = a.J, rowlen = a.rowlen;

    wb_write_next_carry<OPV_WB_THREADS>(a.hist_out, a.hist_in, a.hist_len, a.src, a.n_new, a.n_before, J - 1, tid);
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

    wb_load_lo<OPV_WB_THREADS>(lo, a.lo, tid);

    // local sample j of the span is src[base_i + j]; the newest sample of output out0 + l is local sample front + dn_l
    const int64_t base_i = (int64_t)((uint64_t)a.nrel0 + q0) - (int64_t)front;
    wb_fetch_span<OPV_WB_THREADS>(raw, a.hist_in, a.hist_len, a.src, a.n_new, base_i, span, tid, [](uint32_t j) { return j; });
    __syncthreads();

    // phase of local sample j: Lo's for sample base_i + j of the push (WbLoFixed: phi = (uint32)((first_sample + n) * inc) - the
    // low 32 bits only, so 32-bit arithmetic that wraps)
    const uint32_t k_end = (blockIdx.y + 1) * a.kper < a.K ? (blockIdx.y + 1) * a.kper : a.K;
    const uint32_t tl = pbase + (tid < cnt ? tid : 0u) * M;
    const uint32_t dn = tl / U;
    const uint32_t top = front + dn;                                    // tap j reads local sample top - j >= dn >= 0
    const int16_t* tab = (const int16_t*)a.taps;                        // the rational door's image: the phase-major int16 table
    const int2* row = (const int2*)(tab + (size_t)(tl - dn * U) * rowlen);   // 4 taps per 8 bytes
    for (uint32_t k = blockIdx.y * a.kper; k < k_end; ++k) {
        const auto lo_of = Lo::channel(lo_table, lo_base, k, (uint32_t)(uint64_t)base_i);
        for (uint32_t j = tid; j < span; j += OPV_WB_THREADS) {
            int c, s;
            lo_of(lo, j, c, s);
            mixed[mixed_slot(j)] = wb_mix_down(raw[j], c, s);
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
            a.dst[k][out0 + tid] = wb_round_pack(ar, ai, a.S);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_wbr_ddc(OpvWbrArgs a) { wbr_ddc<WbLoFixed>(a, a.inc, a.a0_lo); }

// the same door behind an LO schedule (opv_wb_retune): sched[K] is this push's table, its origin kWbSchedBack samples in front of src[0]
extern "C" __global__ __launch_bounds__(256) void k_wbr_ddc_tuned(OpvWbrArgs a, const OpvWbDevSched* sched) { wbr_ddc<WbLoTuned>(a, sched, kWbSchedBack); }
