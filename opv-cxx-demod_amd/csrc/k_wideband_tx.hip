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

// the kernel's body, once for both sources of the LO: k_wideband_tx_body.inc
extern "C" __global__ __launch_bounds__(256) void k_wbtx_duc(OpvWbtxArgs a) {
#define WB_LO_OF(k, first) WbLoFixed::channel(a.inc, a.a0_lo, k, first)
#include "k_wideband_tx_body.inc"
#undef WB_LO_OF
}

// the same bank behind an LO schedule (opv_wbtx_retune): sched[K] is this push's table, its origin the push's first wide sample; a.inc is not read
extern "C" __global__ __launch_bounds__(256) void k_wbtx_duc_tuned(OpvWbtxArgs a, const OpvWbDevSched* sched) {
#define WB_LO_OF(k, first) WbLoTuned::channel(sched, 0u, k, first)
#include "k_wideband_tx_body.inc"
#undef WB_LO_OF
}
