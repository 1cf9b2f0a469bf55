// opv_tx_internal.h — pieces of the host transmit chain (opv_tx.cpp) reused by the device
// modulator in opv_tx_device.hip / k_tx_modulate.hip. Not part of the public ABI.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "opv_frame_code.h"

// ---- the modulator's numbers, host and device (opv-mod.cpp:36-43, :259-260) and the NCO's step: a rounded add, then the wrap (:274-279)
constexpr double kPi = 3.14159265358979323846;
constexpr double kTwoPi = 2.0 * kPi;
constexpr double kFs = 2168000.0;
constexpr double kDev = 54200.0 / 4.0;
constexpr double kInc1 = kTwoPi * (-kDev) / kFs, kInc2 = kTwoPi * (+kDev) / kFs;   // phase per sample of tone 1 / tone 2
OPV_HD inline void advance(double& ph, double inc) {
    ph += inc;
    while (ph > kPi) ph -= kTwoPi;
    while (ph < -kPi) ph += kTwoPi;
}
// The same step without loops, for a phase that is in [-pi, pi] before it: tone 1 only ever falls (kInc1 < 0: it can pass -pi, never
// pi) and tone 2 only ever rises, and |inc| < pi, so of the two loops above one never runs and the other at most once - the same
// adds on the same values, the wrapped one chosen by a select (k_txb_phases replays 128 x 40 of these in a row per thread, and a
// lone wave pays for every instruction of them)
static_assert(kInc1 > -kPi && kInc1 < 0.0 && kInc2 < kPi && kInc2 > 0.0, "advance_tone1 / advance_tone2: one wrap per step at most, each to its side");
OPV_HD inline void advance_tone1(double& ph) {
    const double t = ph + kInc1, up = t + kTwoPi;
    ph = t < -kPi ? up : t;
}
OPV_HD inline void advance_tone2(double& ph) {
    const double t = ph + kInc2, down = t - kTwoPi;
    ph = t > kPi ? down : t;
}

// per-symbol tone/sign code of a whole opv-mod run: +/-1 tone 1, +/-2 tone 2, 0 silent
void opv_tx_symbol_codes(const uint8_t* frames134, size_t n_frames, int8_t* amp);
// NCO phases (ph1, ph2) at the start of n_symbols consecutive symbols, continuing from *ph1/*ph2
void opv_tx_symbol_phases(size_t first_symbol, size_t n_symbols, double* ph1_io, double* ph2_io, double* out2);
// one sample exactly as the reference computes it (libm), i samples into a symbol
void opv_tx_sample_exact(double ph1_sym, double ph2_sym, int a, int i, int16_t* I, int16_t* Q);

// ---- device transmit chain (k_tx_modulate.hip) ------------------------------------------------------------------
#define OPV_TX_CKPT_SYMS 128      // an NCO checkpoint every 128 symbols (5120 samples)
#define OPV_TX_CKPT_FRAMES 4096   // frames the build-time table covers (longer runs continue on the host, once per process)
// the embedded table (opv_tx_ckpt.cpp): n_entries pairs (ph1, ph2), entry j = state at symbol j * OPV_TX_CKPT_SYMS
const double* opv_tx_checkpoints(size_t* n_entries);
// entries [first, first + count) of the checkpoint sequence into out2 (2 doubles each): from the embedded table, beyond it
// from a process-wide extension that continues the recurrence on the host (thread-safe, computed once)
void opv_tx_checkpoint_range(size_t first, size_t count, double* out2);
