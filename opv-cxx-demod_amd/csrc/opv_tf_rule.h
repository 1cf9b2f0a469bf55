// opv_tf_rule.h — the per-call proof that the timing loop's clamp cannot act, one definition for the kernel that relies on it
// (k_frontend.hip: msk_frontend_body picks one of two symbol nests per demodulate() call) and for the host (tests/tf_rule_probe.cpp,
// tests/test_tf_clamp_rule_host.py). Plain C++17 for g++ and for hipcc, host and device alike; no other header of the project.
//
// The reference's timing loop (ref :118, :283-284): tf = clamp(tf + beta * ted, -0.1, +0.1), beta = 1e-5, once per symbol.
//   * ted = (el - ee) / (el + ee + 1e-10) with el, ee >= 0: |el - ee| < el + ee + 1e-10, so |ted| <= 1 up to the rounding of one
//     subtraction, two additions and the division. The rule bounds it by 2 and so needs no last-place reasoning.
//   * A symbol advances pos by 40 + adj, adj = alpha * ted + tf, |adj| <= 0.005 * 2 + 0.1 < 1: more than 39 samples per symbol, so
//     a call over n samples has at most n / 39 + 2 symbols (integer division; the + 2 covers the first symbol and the floor).
// Hence after any symbol of the call |tf| <= |tf at its start| + 2 * beta * (n / 39 + 2), and where that stays below 0.1 the clamp
// returns its argument unchanged on every symbol: fmin(fmax(x, -0.1), 0.1) == x, bit for bit, for every non-NaN x inside the
// bounds (and for +/-0.1 themselves). The roundings of the n / 39 + 2 additions (half an ulp of 0.1 each, 1.6e-14 in a -s call) are
// covered many times over by the factor 2: what a call can really add is beta * (1 + a few ulps) per symbol, so the rule keeps
// beta * (n / 39 + 2) >= 2e-5 in hand. A NaN fails the comparison and is left to the nest that keeps the clamp. A -s call (86 720 samples) passes with
// |tf| < 0.0555; a batch-mode call over a capture of 195 000 samples or more never does, whatever its tf.
#pragma once
#include <math.h>
#include <stdint.h>

#ifndef OPV_HD
#ifdef __HIPCC__
#define OPV_HD __host__ __device__
#else
#define OPV_HD
#endif
#endif

constexpr double kOpvTfBeta = 0.00001;    // ref :118
constexpr double kOpvTfMax = 0.1;         // ref :284

OPV_HD inline bool opv_tf_clamp_cannot_act(double tf, uint64_t n_samples_of_call) {
    const double symbols = (double)(n_samples_of_call / 39u + 2u);   // exact: below 2^53 for every n
    return fabs(tf) + 2.0 * kOpvTfBeta * symbols < kOpvTfMax;        // false for a NaN
}
