// k_wideband_tx.hip — k_wbtx_duc: the wideband transmit bank's up-converters (include/opv_demod.h, opv_wbtx_*), the mirror image of
// k_wb_ddc. One launch per push serves all K channels: zero-stuff each channel by U, filter with int16 taps, mix it up to +f_k with
// the DDC's closed-form integer LO, sum the channels, round, clamp and store one wide capture. The arithmetic is integer-exact and
// independent of summation order (|y| < 2^31 per channel: int32 over the taps; |sum| < 2^55: int64 over the channels), so parity with
// the numpy model is `==`.
//
// Shape: a workgroup owns 256 consecutive wide outputs, one per thread, and loops over all K channels itself: a thread keeps its
// output's (wr, wi) in int64 registers, so there is no sum across workgroups and no atomic. Wide sample n = q U + p reads taps
// p, p + U, ... against inputs q, q - 1, ...: consecutive lanes are consecutive p of the same q, so the input read is an LDS broadcast and
// the tap read is unit-stride (the taps stand in LDS as they are, padded with zeros to a whole number of phases: every thread runs
// the J taps of the longest phase and no lane branches). Per channel the workgroup's span of inputs - 256 / U new ones and the J - 1
// in front, from the carry, from this push, or zeros for an absent channel - goes into LDS once; two span buffers taken in turn
// leave one barrier per channel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_wideband_common.h"
#include "opv_wbtx_internal.h"

extern "C" __global__ __launch_bounds__(256) void k_wbtx_duc(OpvWbtxArgs a) {
    __shared__ int xs[2][OPV_WBTX_SPAN];      // packed int16 I | Q << 16
    __shared__ int16_t tp[OPV_WBTX_TAPS];
    __shared__ int16_t lo[4096];
    const uint32_t tid = threadIdx.x;
    const uint32_t U = a.U, H = a.H, J = a.J;

    wbtx_write_next_carry<OPV_WBTX_THREADS>(a.hist_out, a.hist_in, H, a.in, a.n_in, a.K, tid);
    const uint32_t n0 = blockIdx.x * OPV_WBTX_THREADS;                    // first wide output of this workgroup, within the push
    if (n0 >= a.n_out) return;

    wb_load_lo<OPV_WBTX_THREADS>(lo, a.lo, tid);
    for (uint32_t i = tid; i < J * U; i += OPV_WBTX_THREADS) tp[i] = i < a.L ? a.taps[i] : (int16_t)0;

    const uint32_t n_last = n0 + OPV_WBTX_THREADS - 1 < a.n_out ? n0 + OPV_WBTX_THREADS - 1 : a.n_out - 1;
    const uint32_t n = n0 + tid < a.n_out ? n0 + tid : n_last;           // (threads past the end redo the last output and store nothing)
    const uint32_t q_lo = n0 / U, q_last = n_last / U, q = n / U, p = n - q * U;
    // local sample i of the span is input sample q_lo - (J - 1) + i of this push: negative ones lie in the carry
    const uint32_t span = q_last - q_lo + J;
    const int64_t m0 = (int64_t)q_lo - (int64_t)(J - 1);
    const uint32_t xq = q - q_lo + J - 1;                                 // where x[q] stands; tap j reads xq - j >= 0
    const uint32_t a_lo = a.a0_lo + n;                                    // phi = (uint32)((first_sample + n) * inc): the low 32 bits only
    int64_t wr = 0, wi = 0;
    for (uint32_t k = 0; k < a.K; ++k) {
        int* x = xs[k & 1];
        const int* src = a.in[k];
        const int* old = a.hist_in + (size_t)k * H;
        for (uint32_t i = tid; i < span; i += OPV_WBTX_THREADS) {
            const int64_t m = m0 + (int64_t)i;                            // -H <= -(J - 1) <= m <= q_last < n_in
            x[i] = m < 0 ? old[(int64_t)H + m] : src ? src[m] : 0;
        }
        __syncthreads();                                                  // (also: tp and lo, before the first channel)
        int yr = 0, yi = 0;
        for (uint32_t j = 0; j < J; ++j) {
            const int v = x[xq - j];
            const int h = tp[p + j * U];
            yr += h * (int)(int16_t)(v & 0xFFFF);
            yi += h * (v >> 16);
        }
        int c, s;
        wb_lo_at(lo, a_lo * a.inc[k], c, s);
        wb_mix_up(wr, wi, yr, yi, c, s);
        // (no second barrier: the next channel fills the other span buffer, which was last read before the barrier above)
    }
    if (n0 + tid < a.n_out) a.out[n0 + tid] = wb_round_pack(wr, wi, a.S);
}
