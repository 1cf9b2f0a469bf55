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

#include "k_wideband_common.h"
#include "opv_wb_internal.h"

namespace {

// j / D for j < 4096 + 16 and 1 <= D <= 16 without a divide: m = ceil(2^16 / D) overshoots 2^16 / D by e / D with e = m D - 2^16 < D,
// so j m >> 16 is exact while j e < 2^16, and (4096 + 16) * 15 < 65536.
__device__ __forceinline__ uint32_t lds_slot(uint32_t j, uint32_t D, uint32_t m, uint32_t rowlen) {
    const uint32_t row = (j * m) >> 16;
    return (j - row * D) * rowlen + row;
}

// the kernel's body, once for both sources of the LO (k_wideband_common.h: WbLoFixed, WbLoTuned)
template <class Lo>
__device__ __forceinline__ void wb_ddc(const OpvWbArgs a, const typename Lo::Table* lo_table, uint32_t lo_base) {
    __shared__ int raw[OPV_WB_SPAN];          // packed int16 I | Q << 16
    __shared__ int2 mixed[OPV_WB_SPAN];       // (mr, mi) of the channel in hand
    __shared__ int16_t lo[4096];
    const uint32_t tid = threadIdx.x;
    const uint32_t D = a.D, L = a.L, rowlen = a.rowlen, span = D * rowlen;
    const uint32_t recip = (65536u + D - 1u) / D;

    wb_write_next_carry<OPV_WB_THREADS>(a.hist_out, a.hist_in, a.hist_len, a.src, a.n_new, a.n_before, L - 1, tid);
    const uint64_t out0 = (uint64_t)blockIdx.x * a.tile;               // first output of this workgroup, within the push
    if (out0 >= a.n_out) return;
    const uint32_t cnt = a.n_out - out0 < a.tile ? (uint32_t)(a.n_out - out0) : a.tile;

    wb_load_lo<OPV_WB_THREADS>(lo, a.lo, tid);

    // local sample j of the span is sample n = (r0 + out0) * D - lpad + j of the object, i.e. src[base_i + j]
    const int64_t base_i = (int64_t)((a.r0 + out0) * D) - (int64_t)a.lpad - (int64_t)a.n_before;
    wb_fetch_span<OPV_WB_THREADS>(raw, a.hist_in, a.hist_len, a.src, a.n_new, base_i, span, tid, [=](uint32_t j) { return lds_slot(j, D, recip, rowlen); });
    __syncthreads();

    // phase of local sample j: Lo's for sample base_i + j of the push (WbLoFixed: phi = (uint32)((first_sample + n) * inc) - the
    // low 32 bits only, so 32-bit arithmetic that wraps)
    const uint32_t k_end = (blockIdx.y + 1) * a.kper < a.K ? (blockIdx.y + 1) * a.kper : a.K;
    const int* taps = (const int*)a.taps;                               // the integer door's image: h[L] widened to int32
    const uint32_t u_lo = a.lpad - (L - 1);                             // tap t reads local sample lane * D + (lpad - t)
    for (uint32_t k = blockIdx.y * a.kper; k < k_end; ++k) {
        const auto lo_of = Lo::channel(lo_table, lo_base, k, (uint32_t)(uint64_t)base_i);
        for (uint32_t p = 0; p < D; ++p) {
            for (uint32_t row = tid; row < rowlen; row += OPV_WB_THREADS) {
                int c, s;
                lo_of(lo, row * D + p, c, s);
                mixed[p * rowlen + row] = wb_mix_down(raw[p * rowlen + row], c, s);
            }
        }
        __syncthreads();
        if (tid < cnt) {
            int64_t ar = 0, ai = 0;
            uint32_t p = u_lo % D, row = u_lo / D + tid;
            for (uint32_t t = L; t-- > 0;) {                            // u = lpad - t runs upwards: (p, row) step without a divide
                const int2 m = mixed[p * rowlen + row];
                const int64_t h = taps[t];
                ar += h * m.x;
                ai += h * m.y;
                if (++p == D) { p = 0; ++row; }
            }
            a.dst[k][out0 + tid] = wb_round_pack(ar, ai, a.S);
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_wb_ddc(OpvWbArgs a) { wb_ddc<WbLoFixed>(a, a.inc, a.a0_lo); }

// the same door behind an LO schedule (opv_wb_retune): sched[K] is this push's table, its origin kWbSchedBack samples in front of src[0]
extern "C" __global__ __launch_bounds__(256) void k_wb_ddc_tuned(OpvWbArgs a, const OpvWbDevSched* sched) { wb_ddc<WbLoTuned>(a, sched, kWbSchedBack); }
