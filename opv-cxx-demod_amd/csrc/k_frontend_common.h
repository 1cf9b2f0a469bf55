// k_frontend_common.h — what the three stream-to-wave mappings of the MSK front-end share word for word (k_frontend.hip:
// one stream per wave, k_frontend_x4.hip: four, k_frontend_x16.hip: sixteen): constants of the reference, bit-level helpers,
// the carry of the on-time sums, and the signed-zero rule for std::arg on digital silence. Device-only; everything has
// internal linkage, because every .hip file is compiled to a code object of its own (tools/align_vop3.py depends on that).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "opv_device.h"

namespace {

constexpr double kPi = 3.14159265358979323846;  // ref :43
constexpr double kTwoPi = 2.0 * kPi;            // ref :44
constexpr double kFs = 2168000.0;               // ref :40
constexpr double kSymRate = 2168000.0 / 40.0;   // ref :41
constexpr double kDeltaPerHz = kTwoPi / kFs;    // d = 2 pi fo / Fs (ref :210-211, :305-306)

typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) unsigned char gbyte;

__device__ inline int dlo(double v) { return __double2loint(v); }
__device__ inline int dhi(double v) { return __double2hiint(v); }
__device__ inline double mkd(int hi, int lo) { return __hiloint2double(hi, lo); }

__device__ inline double clampd(double v, double lo, double hi) { return fmin(fmax(v, lo), hi); }

// four sums over a DPP row or quad in lockstep (CTRL: the rotation or permutation of one step): a DPP read needs two wait
// states behind the VALU write of its source, and one sum's steps are a dependent chain (hipcc pads every step with
// s_nop 1) - the other three sums' instructions fill the slots
template <int CTRL>
__device__ inline void dpp_add4(double& a, double& b, double& c, double& d) {
    const int al = __builtin_amdgcn_mov_dpp(dlo(a), CTRL, 0xF, 0xF, true), ah = __builtin_amdgcn_mov_dpp(dhi(a), CTRL, 0xF, 0xF, true);
    const int bl = __builtin_amdgcn_mov_dpp(dlo(b), CTRL, 0xF, 0xF, true), bh = __builtin_amdgcn_mov_dpp(dhi(b), CTRL, 0xF, 0xF, true);
    const int cl = __builtin_amdgcn_mov_dpp(dlo(c), CTRL, 0xF, 0xF, true), ch = __builtin_amdgcn_mov_dpp(dhi(c), CTRL, 0xF, 0xF, true);
    const int dl = __builtin_amdgcn_mov_dpp(dlo(d), CTRL, 0xF, 0xF, true), dh = __builtin_amdgcn_mov_dpp(dhi(d), CTRL, 0xF, 0xF, true);
    __builtin_amdgcn_sched_barrier(0);
    a += mkd(ah, al); b += mkd(bh, bl); c += mkd(ch, cl); d += mkd(dh, dl);
    __builtin_amdgcn_sched_barrier(0);
}

// exp(j x), |x| <= 0.284, for the several-streams-per-wave mappings: a near-minimax pair of degree 4 in u = x^2 each (ten
// coefficients, abs error 1e-19 / 1.3e-18). NOT k_frontend.hip's expj_small: that one is an asm block with a cubic for
// the sine, a measured choice of the one-wave kernel (see there).
__device__ inline void expj_small10(double x, double& xs, double& xc) {
    const double u = x * x;
    double p = fma(-0x1.add325df5e3b5p-26, u, 0x1.71de256e9bdffp-19);
    double r = fma(-0x1.276f06eab6283p-22, u, 0x1.a019dfaa26924p-16);
    p = fma(p, u, -0x1.a01a019da51d6p-13);
    r = fma(r, u, -0x1.6c16c16818f3fp-10);
    p = fma(p, u, 0x1.1111111110f73p-7);
    r = fma(r, u, 0x1.5555555555014p-5);
    p = fma(p, u, -0x1.5555555555555p-3);
    r = fma(r, u, -0x1.0000000000000p-1);
    xc = fma(r, u, 1.0);
    xs = fma(x * u, p, x);
}

struct PrevSums {
    double a, b, c, d;  // on-time P1..P4
    double x40c, x40s;  // X[40] = exp(j 40 d) of that symbol
};

// Digital silence on either side of the phase detector (rare, uniform over the lanes of a stream, kept out of line).
// The reference's product dom * conj(prev) (ref :299) is then an exact zero whose SIGNS decide
// std::arg: atan2(+0,-0) = pi, everything else +/-0 (IEEE). Working the signs through its
// complex multiply:
//   dom == (+0,+0), prev != 0 : pi iff Re(prev) < 0 and Im(prev) < 0
//   prev == (+0,+0), dom != 0 : pi iff Re(dom)  < 0 and Im(dom)  < 0
//   both zero                  : 0
// where dom/prev are the reference's correlations, i.e. ours times the absolute LO phasor it
// carries: c_t(k) = S_t(k) conj(E_t(k)), prev_t = P_t conj(E_t(k)), P_t = S_t(k-1) (-/+ j) X40(k-1),
// E_t(k) = exp(j(-/+ k pi/2 + (80 pi/Fs) sum_{j<k} fo_j)), rebuilt here from the running sum of fo
// (fo_sum: over the symbols BEFORE this one; ksym: their number). Checked on 598 gap edges by
// tests/test_gpu_parity.py::test_many_silence_gaps_signed_zero_rule.
//
// The one input class that is NOT reproducible is counted here (`ties`, reported as
// opv_stream_state.edge_ties): a window with exactly ONE non-zero tap, i.e. the first symbol a burst
// touches or the last one it leaves. Both tone energies are then |s|^2 in exact arithmetic (P1 P2 ==
// P3 P4, soft = 4 (P3 P4 - P1 P2) = 0) and the reference's e1 > e2 (ref :272/:291) is decided by the
// rounding of its own cos^2 + sin^2 at the accumulated LO phase, which no mapping carries. Such a
// symbol always has digital silence on one side, so it passes through this routine either as `cur`
// (leading edge: prev is zero) or as `prv` (trailing edge: dom is zero) - no cost on the symbol path.
__device__ inline bool tone_tie(double p1, double p2, double p3, double p4) {
    const double x = p1 * p2, y = p3 * p4;
    return (p1 != 0.0 || p2 != 0.0 || p3 != 0.0 || p4 != 0.0) && fabs(y - x) <= 1e-12 * (fabs(x) + fabs(y));
}
// Returns {pd, 1.0 if such a tie was seen else 0.0} (by value: no stack slot on the caller's side). Of ksym only ksym & 3
// is read. Its type is the caller's own (the one-wave kernel counts symbols in 64 bits, the other two pass a 32-bit sum):
// each code object holds one instance, and a fixed width re-allocated registers in the callers' symbol loops (32 bits:
// k_msk_frontend_rb_wg4 276 -> 274 VGPRs; 64 bits: a move more per call site of the row and quad kernels).
template <typename Count>
__device__ __noinline__ double2 silence_pd(double dr, double di, PrevSums prv, bool dom1, double fo_sum, Count ksym,
                                           double c1, double c2, double c3, double c4) {
    const double pr = dom1 ? prv.a + prv.b : prv.a - prv.b, pi = dom1 ? prv.c - prv.d : prv.c + prv.d;
    const bool dom_zero = (dr == 0.0 && di == 0.0), prev_zero = (pr == 0.0 && pi == 0.0);
    if (dom_zero == prev_zero) return make_double2(0.0, 0.0);
    const double tie = (prev_zero ? tone_tie(c1, c2, c3, c4) : tone_tie(prv.a, prv.b, prv.c, prv.d)) ? 1.0 : 0.0;
    double th = (80.0 * kPi / kFs) * fo_sum;
    th -= kTwoPi * rint(th / kTwoPi);
    double sn, cs;
    sincos(th, &sn, &cs);
    // multiply by (-/+ j)^k : tone 1 rotates by -pi/2 per symbol, tone 2 by +pi/2
    const unsigned q = (unsigned)((dom1 ? (4u - (unsigned)(ksym & 3u)) : (unsigned)(ksym & 3u)) & 3u);
    double er2 = cs, ei2 = sn;
    if (q == 1u) { er2 = -sn; ei2 = cs; }
    else if (q == 2u) { er2 = -cs; ei2 = -sn; }
    else if (q == 3u) { er2 = sn; ei2 = -cs; }
    double vr = dr, vi = di;
    if (dom_zero) {                                 // P = S_prev * (-/+ j) * X40_prev
        const double jr = dom1 ? pi : -pi, ji = dom1 ? -pr : pr;
        vr = jr * prv.x40c - ji * prv.x40s;
        vi = jr * prv.x40s + ji * prv.x40c;
    }
    const double qr = vr * er2 + vi * ei2;          // v * conj(E)
    const double qi = vi * er2 - vr * ei2;
    return make_double2((qr < 0.0 && qi < 0.0) ? kPi : 0.0, tie);
}

}  // namespace
