// k_wideband_tx_rational.hip — k_wbtxr_duc: the up-converters of the rational wideband transmit bank (include/opv_demod.h,
// opv_wbtx_create_rational), the mirror image of k_wbr_ddc: the wide rate is 2 168 000 x M / U S/s. One launch per push serves all K
// channels: zero-stuff each channel by M, filter with int16 taps, keep every U-th sample - wide sample n reads the J inputs q_n,
// q_n - 1, ... (q_n = floor(n U / M)) against row p_n = (n U) mod M of the phase-major tap table - mix it up to +f_k with the DDC's
// closed-form integer LO, sum the channels, round, clamp and store one wide capture. Integer-exact and independent of summation
// order (|y| < 2^31 per channel: int32 over the taps; |sum| < 2^55: int64 over the channels), so parity with the numpy model is `==`.
//
// Shape, as k_wbtx_duc: a workgroup owns 256 consecutive wide outputs of the push, one per thread, and loops over all K channels
// itself: a thread keeps its output's (wr, wi) in int64 registers, so there is no sum across workgroups and no atomic. A thread's
// phase, and with it its row of taps, is the same for all K channels: the rows are read from the global table ONCE per workgroup
// into LDS, j-major with two int16 per dword (tile[j / 2][tid]: lanes at unit stride on every read; a thread-major row of 64 taps
// would put 64 lanes on two banks). Per channel the workgroup's span of inputs - floor(255 U / M) + 1 new ones at most and the
// taps' reach in front, from the carry, from this push, or zeros for an absent channel - goes into LDS once (neighbouring lanes
// read the same or the adjacent input: a broadcast); a thread fetches the next channel's share of the span into registers while it
// runs the taps of this one, and two span buffers taken in turn leave one barrier per channel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_wideband_common.h"
#include "opv_wbtx_internal.h"

// the kernel's body, once for both sources of the LO: k_wideband_tx_rational_body.inc
extern "C" __global__ __launch_bounds__(256) void k_wbtxr_duc(OpvWbtxrArgs a) {
#define WB_LO_OF(k, first) WbLoFixed::channel(a.inc, a.a0_lo, k, first)
#include "k_wideband_tx_rational_body.inc"
#undef WB_LO_OF
}

// the same bank behind an LO schedule (opv_wbtx_retune): sched[K] is this push's table, its origin the push's first wide sample; a.inc is not read
extern "C" __global__ __launch_bounds__(256) void k_wbtxr_duc_tuned(OpvWbtxrArgs a, const OpvWbDevSched* sched) {
#define WB_LO_OF(k, first) WbLoTuned::channel(sched, 0u, k, first)
#include "k_wideband_tx_rational_body.inc"
#undef WB_LO_OF
}
