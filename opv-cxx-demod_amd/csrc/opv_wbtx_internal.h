// opv_wbtx_internal.h — what the host half of the wideband transmit bank (opv_wideband_tx.hip) hands to its kernel (k_wideband_tx.hip).
// The door to the context is the receive bank's (opv_wb_internal.h); the rules of both are opv_wb_rules.h.
#ifndef OPV_WBTX_INTERNAL_H
#define OPV_WBTX_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

// What both up-converter kernels are handed, by value, filled once by opv_wbtx_push. This push holds input samples [N, N + n_in)
// of every channel and writes n_out wide samples.
struct OpvWbtxHead {
    const int* const* in;    // in[K]: n_in packed (I | Q << 16) samples per channel in device memory, or null for an absent channel (zeros)
    const int* hist_in;      // [K][H]: the H input samples in front of this push, zeros where the channel had none yet
    int* hist_out;           // the other carry buffer: the last H samples of (hist_in, this push), channel k by workgroup k % gridDim.x
    const int16_t* lo;       // T[4096]
    const int16_t* taps;     // the taps as the kind's kernel reads them: h[L] (k_wbtx_duc), or the phase-major table [M][rowlen],
                             // tab[p * rowlen + j] = taps[p + j M], zeros from L on (k_wbtxr_duc)
    const uint32_t* inc;     // inc[K]
    int* out;                // n_out packed wide samples
    uint32_t a0_lo;          // low 32 bits of first_sample + the push's first wide sample: all the closed-form phase needs
    uint32_t n_in, n_out;
    uint32_t K, S;
    uint32_t H;              // input samples carried per channel
};

// Arguments of k_wbtx_duc (k_wideband_tx.hip). Input sample m of a channel (0 = its first sample ever pushed) feeds wide samples
// [m U, (m + 1) U) of the object; this push writes wide samples [N U, (N + n_in) U). H = ceil((L - 1) / U).
struct OpvWbtxArgs : OpvWbtxHead {
    uint32_t U, L;
    uint32_t J;              // floor((L - 1) / U) + 1: taps of the longest phase (p = 0)
};
constexpr uint32_t OPV_WBTX_THREADS = 256;                                  // = wide outputs per workgroup, one per thread
constexpr uint32_t OPV_WBTX_SPAN = OPV_WBTX_THREADS + 1024;                 // input samples a workgroup holds per channel: <= 256 / U + 1 new ones + J - 1 <= 1023 in front
constexpr uint32_t OPV_WBTX_TAPS = 1024 + 16;                               // J U <= L - 1 + U entries, zeros from L on

extern "C" __global__ void k_wbtx_duc(OpvWbtxArgs a);
struct OpvWbDevSched;        // opv_wb_rules.h: one channel's LO schedule as the kernels of one push read it
extern "C" __global__ void k_wbtx_duc_tuned(OpvWbtxArgs a, const OpvWbDevSched* sched);  // the same behind an LO schedule; a.inc is not read

// Arguments of k_wbtxr_duc (k_wideband_tx_rational.hip: the object made by opv_wbtx_create_rational). The wide rate is
// 2 168 000 x M / U: output i of this push is wide sample W(N) + i of the object; with t = p0 + i U it reads input floor(t / M) of
// this push and the ones in front of it against row t mod M of the phase-major tap table (opv_wb_rules.h). H = J - 1,
// n_out = W(N + n_in) - W(N).
struct OpvWbtxrArgs : OpvWbtxHead {
    uint32_t M, U;
    uint32_t J2;             // ceil(J / 2): tap pairs per phase (2 J2 <= rowlen)
    uint32_t rowlen;         // J rounded up to a multiple of 4
    uint32_t p0;             // phase of the push's first output: W(N) U - N M
};
constexpr uint32_t OPV_WBTXR_THREADS = 256;                                 // = wide outputs per workgroup, one per thread (= kWbtxrTile)
constexpr uint32_t OPV_WBTXR_MAXJ = 64;                                     // (= kWbtxrMaxJ)
constexpr uint32_t OPV_WBTXR_SPAN = OPV_WBTXR_THREADS + OPV_WBTXR_MAXJ;     // input samples a workgroup holds per channel: <= floor(255 U / M) + 1 new ones + 2 J2 - 1 <= 63 in front

extern "C" __global__ void k_wbtxr_duc(OpvWbtxrArgs a);
extern "C" __global__ void k_wbtxr_duc_tuned(OpvWbtxrArgs a, const OpvWbDevSched* sched);

#endif
