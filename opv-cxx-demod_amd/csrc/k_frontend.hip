// k_frontend.hip — MSK front-end: dual-tone correlator bank + early-late-gate timing loop +
// AFC, one wavefront (64 lanes) per IQ stream, serial over symbols, parallel inside a symbol.
//
// Replaces MSKDemodulatorAFC::demodulate (+interp) (reference src/opv-demod.cpp:206-329,
// :122-128) and the streaming chunker / batch driver of main() (:1012-1113 / :1132-1173).
//
// -------------------------------------------------------------------------------------------
// Algorithm restatement (what is computed per symbol, ref line in brackets)
//   samples:   L(p) = s[floor p](1-f) + s[floor p + 1] f                      [:122-128]
//   on-time:   c_t = sum_{i<40} L(pos+i)      conj(lo_t[i])                   [:236,:243-244]
//   early:     e_t = sum_{i<40} L(pos+i-10)   conj(lo_t[i])  (s[0] if <0)     [:237,:245-246]
//   late:      l_t = sum_{i<40} L(pos+i+10)   conj(lo_t[i])                   [:238,:247-248]
//   lo_t[i] = exp(j(ph_t + i inc_t)), inc_t = 2pi(-/+13550 + fo)/Fs, ph_t += 40 inc_t [:240-251]
//   soft = |c_2|^2 - |c_1|^2                                                  [:264-268]
//   ted on the dominant tone, 2nd-order loop on pos                           [:271-286,:313]
//   AFC: fo += alpha * arg(c_dom conj(c_dom_prev)) * 54200/2pi, not on the first
//        symbol of a demodulate() call                                        [:289-306]
//
// MI355X mapping
//   * Lane j (0..59) owns ONE interpolated sample  Lam_j = L(pos + j - 10). The three gates
//     are the same 60 values under three shifts: early uses lanes 0..39, on-time 10..49, late
//     20..59, so the 120 interpolations of the reference become 60, one per lane. (Row-broadcast body: 15 samples per
//     row of 16 lanes, lane 16 r + n <-> sample 15 r + n; a row's last lane carries no weight.)
//   * The LO is factored  lo_t[i] = E_t * T_t[i] * X[i],  E_t = exp(j ph_t) (a rotation that
//     every use below is invariant to, so it is never formed and no phase is tracked),
//     T_t[i] = exp(-/+ j 2pi i/160) a per-lane CONSTANT (13550*40 = Fs/4), and
//     X[m] = exp(j m d), d = 2pi fo/Fs, |m d| <= 0.29 rad: a short polynomial pair per lane
//     instead of two libm sincos per sample. T_2 = conj(T_1), so both tones share four real
//     products per gate:  P1=sum Zr a, P2=sum Zi b, P3=sum Zi a, P4=sum Zr b with
//     Z = Lam conj(X):  C_1 = (P1+P2, P3-P4), C_2 = (P1-P2, P3+P4).
//   * |.|^2 of early/late is invariant to the gate's constant rotation; for the AFC the
//     previous on-time correlation is advanced by the LO rotation of one symbol,
//     P_t = S_t * (-/+ j) * X[40]  (T_t[40] = -/+ j exactly), so that
//     arg(c(k) conj(c(k-1))) = arg(S(k) conj(P(k-1))).
//   * Sums over the wave, current body (`symbol_r`, kernels k_msk_frontend_rb / _rb_wg4): the DP-ALU DPP form
//     v_fmac_f64_dpp acc, src0 row_newbcast:n, src1 lets a row of 16 lanes form 16 differently weighted sums of its
//     samples; with 15 samples per row, 2 x 15 FMACs give ALL window sums of the symbol (on-time / early / late
//     correlations of both tones + the on-time sums P1..P4) as row partials in lane t = lane & 15, one all-reduce over
//     the four rows (two independent v_mfma_f64_4x4x4_4b_f64 with 0/1 row selectors and an add: the fp64 matrix pipe contracts over
//     lane bits 4-5, which is exactly the row index; bit for bit the two permlane swaps it replaced) completes them, v_mov_b64_dpp row_newbcast hands out what the loop filters need, the energies and
//     the dominant-tone select (shift and select in one v_cndmask_b32_dpp per word) are lane-parallel. The four-symbol loop
//     holds 133.75 instructions per symbol on the fp64 ring (135.75 in a call that keeps the timing clamp), 141.75 / 143.75 on the
//     int16 ring, 142.75 / 144.75 with four waves per workgroup (scripts/experiments/trip_census.py on the device assembly).
//     The scalar loop filters run redundantly on all lanes (wave-uniform, no divergence).
//   * A LONE wave on a SIMD issues one instruction of ANY kind (VALU, SALU, LDS, s_nop, branch)
//     every ~4.7 cycles and gains nothing from independent chains (scripts/microbench): the
//     symbol rate is set by the instruction COUNT of the loop body. Hence: no per-symbol
//     bookkeeping (chunk end and tile events are tested once per batch of symbols that provably
//     need neither), stateless power-of-two ring addressing, sign choices folded into FMA
//     multipliers and bit-field inserts, one shared reciprocal for the two divides, symbols
//     processed in pairs with alternating "previous" registers, the first symbol of a call (no
//     AFC) as its own instantiation, hazard slots of swaps / DPP reads filled with useful work.
//     Between two batches of whole four-symbol trips the wave goes from the trip loop straight to the
//     bookkeeping and back (fp64 ring: 35 instructions, 2 taken branches, the flag read's latency
//     partly covered by scalar work; the remainder path - pairs, a last symbol, settle, copy, a
//     second tap fetch, the `while` test - stood at ~82 and 6-7 and now serves only the first and
//     last symbols of a call and a batch the soft ring cuts short).
//   * int16 IQ is staged HBM -> LDS in 2048-sample tiles (8 KiB) with direct-to-LDS 16-byte
//     loads (global_load_lds_dwordx4, 1 KiB per wave instruction), two tile slots forming a
//     4096-sample ring (slot = sample index & 4095) plus a 4-sample guard that mirrors the head
//     of the even tile for a lane's second interpolation tap; the next tile is requested one
//     whole tile (~51 symbols) before its first use. Lanes read their taps straight from the
//     int16 ring (ds_read2_b32) and widen in registers. While a stream can have a CU to itself
//     (no more streams than CUs) the launch has a second, helper wave that widens the IQ into an
//     fp64 ring instead, and the symbol body reads its interpolation operands ready-made
//     (f64_ring_helper: 8 instructions per symbol fewer; round 8 measured 687 against 750 cycles per symbol, round 10 - this body - 663, round 13 - the batch boundary below - 652.5, profiles/r13_bench_ab.txt; then 631.6, profiles/symbol_slots_bench_ab.txt; with the cross-row sums on the matrix pipe and two soft values per store 621.7, profiles/rowsum_mfma_step0.txt).
//   * fp64 everywhere: the 1e-5 soft contract does not need it, bit-exact quantiser/sync
//     decisions on noisy input do. No MFMA for the correlations: the per-symbol
//     contraction is 3x4x60 with a serial dependence between symbols (the matrix pipe only adds the four row partials).
//
// Roofline: HBM-bound on paper (4 B/sample in, 8 B/symbol out => 4.2 B/sample) but actually
// issue-bound by the per-symbol feedback recurrence; see DESIGN.md and profiles/.
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

#include "k_frontend_common.h"
#include "opv_tf_rule.h"

namespace {

constexpr uint32_t kTile = OPV_TILE_SAMPLES;    // 2048 samples
constexpr uint32_t kRing = 2 * kTile;           // 4096 samples, two tile slots, slot = index & 4095
constexpr uint32_t kRingBytes = kRing * 4;      // 16384
constexpr uint32_t kGuardBytes = 16;            // mirror of the even slot's first 16 B
constexpr uint32_t kBack = 11;                  // lowest tap is floor(pos) - 10, one spare
constexpr uint32_t kAhead = 56;                 // highest tap is floor(pos) + 54, one spare
static_assert((kRing & (kRing - 1)) == 0, "ring must be a power of two");

// LDS map (bytes): WPB x (ring | guard), then ONE atan table shared by the workgroup's waves:
//   1025 rows x 4 doubles (opv_atan_table_q3r.inc: pi/4 + atan(q) around q = k/512, a cubic in q itself, 4e-14 rad:
//   opv_atan2.h says why that is plenty) = 32 800 B -> 49 200 B for one wave, 98 400 B for four
constexpr uint32_t kTabOff = kRingBytes + kGuardBytes;   // 16400
static_assert(kTabOff % 16 == 0, "16-byte LDS alignment");
constexpr uint32_t kAtanQBytes = 1025 * 32;
constexpr uintptr_t kRbLdsBase = 16;                // k_msk_frontend_rb: LDS bytes [0, 16) unused (see the kernel)
static_assert(kRbLdsBase + kTabOff + kAtanQBytes == OPV_RB_LDS_I16, "launch size of the int16-ring shape");

// The fp64 ring (k_msk_frontend_rb launched with 128 threads, one stream per CU): wave 1 is a helper that reads the int16 IQ
// once and writes each sample n as {x_r[n], x_i[n], x_r[n+1] - x_r[n], x_i[n+1] - x_i[n]} in fp64 (32 B, all exact), so that
// the stream's wave reads its interpolation operands with two ds_read_b128 instead of unpacking and widening int16 taps.
// LDS: atan table | ring | {low, ready, done} (table and ring offsets fit the 16-bit offset field of ds_read). `low` (wave 0): lowest sample it still needs; `ready` (wave 1): samples below
// it are written; `done` (wave 0): the helper may leave. Hand-over per batch of symbols, not per symbol; every wait bounded.
constexpr uint32_t kF64Ring = 2048;                  // samples, slot = index & 2047
constexpr uint32_t kF64RingBytes = kF64Ring * 32;    // 65 536
constexpr uint32_t kF64Chunk = 256;                  // samples the helper converts per publication (4 per lane)
constexpr uint32_t kF64TabOff = 0;
constexpr uint32_t kF64RingOff = kAtanQBytes;       // 32 800
constexpr uint32_t kF64FlagOff = kF64RingOff + kF64RingBytes;
constexpr uint32_t kF64WaitSpins = 1u << 22;         // wave 0 waiting for the helper: ~0.1 s of s_sleep 1, never reached
constexpr uint32_t kHelperSpins = 1u << 22;          // helper waiting for a free slot: ~1 s of s_sleep 8 without progress
static_assert(kRbLdsBase + kF64FlagOff + 16 == OPV_RB_LDS_F64, "launch size of the fp64-ring shape");
static_assert(kF64Ring % kF64Chunk == 0 && (kF64Ring & (kF64Ring - 1)) == 0, "chunks tile the power-of-two ring");

// LDS is addressed through address-space-3 pointers throughout, so that offsets from the constant base of k_msk_frontend_rb's
// dynamic allocation fold into the ds_read / ds_write offset fields
typedef double d2v __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) unsigned char lbyte;
typedef __attribute__((address_space(3))) int lint;
typedef __attribute__((address_space(3))) double ldouble;
typedef __attribute__((address_space(3))) d2v ld2v;
typedef __attribute__((address_space(1), aligned(8))) d2v gd2v8;   // two soft values in one store: 8-byte aligned, 0 or 8 mod 16
// a symbol's place in its loop trip; `paired`: the trip of four, whose symbols log their soft values two per 16-byte store
template <uint32_t K, bool PAIRED> struct SlotTag { static constexpr uint32_t value = K; static constexpr bool paired = PAIRED; };

// v_mov_b64_dpp row_newbcast:N - lane N of every row of 16 to all lanes of that row (the one DPP control 64-bit operations
// take). Through the builtin, so that hipcc sees the DPP hazards and schedules around them; every lane is written, `old`
// only names the register: pass a dead value (a zero or an undefined one would cost a move or an s_nop).
template <int N>
__device__ inline double row_bcast(double old, double v) { return __builtin_amdgcn_update_dpp(old, v, 0x150 + N, 0xF, 0xF, false); }
__device__ inline uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
// wave-uniform floating compare -> scalar branch (the operands are identical in every lane)
__device__ inline bool uni_lt(double a, double b) { return __builtin_amdgcn_fcmp(a, b, 4 /*FCMP_OLT*/) != 0ull; }
__device__ inline bool uni_eq(double a, double b) { return __builtin_amdgcn_fcmp(a, b, 1 /*FCMP_OEQ*/) != 0ull; }

// instantiations of the per-symbol body (see `symbol` in the kernel)
struct TagFirst { static constexpr bool first = true, wide = true, tf_free = false; };     // first symbol of a demodulate() call
struct TagSecond { static constexpr bool first = false, wide = true, tf_free = false; };   // second symbol under an out-of-range -o
struct TagSteady { static constexpr bool first = false, wide = false, tf_free = false; };  // everything else ...
struct TagSteadyFree { static constexpr bool first = false, wide = false, tf_free = true; };   // ... in a call whose timing clamp cannot act (opv_tf_clamp_cannot_act)

// X = exp(j x), x = kfs * fo, |x| <= 0.284 (fo within the AFC clamp of +/-2000 Hz, |kf| <= 49):
//   sin x = x + x u q(u),  cos x = 1 + u r(u),  u = x^2,
// q a near-minimax cubic, r of degree 4 on u <= 0.0823 (mpmath chebyfit; in fp64 arithmetic sin to 2.2e-16 = one ulp over
// the whole range, cos to 1.3e-18 before rounding). Round 2 carried a degree-4 q as well (1e-19): one FMA per symbol for
// digits below the rounding of the products that follow. A cubic r (8e-15 at |x| = 0.287, lane 63's sample with fo at its
// clamp) was measured too - 9 cycles per symbol faster still - and is NOT used: on the 6 dB / -2 kHz fixture it moved the
// integer printed by one `raw=%.0f` tracker line (tests/test_gpu_parity.py::test_noisy_configs_vs_reference_fixtures).
// One asm block: the constants stay in registers as written and hipcc's hazard recogniser does
// not pad between the dependent FMAs. (k_frontend_common.h: expj_small10 is the other mappings' plain ten-coefficient pair.)
struct SinCosK {
    double s0, s1, s2, s3;      // q(u) low -> high (cubic)
    double c0, c1, c2, c3, c4;  // r(u) low -> high (degree 4)
};
#define OPV_EXPJ_ASM \
    "v_mul_f64 %[x], %[kfs], %[fo]\n\t" \
    "v_mul_f64 %[u], %[x], %[x]\n\t" \
    "v_fma_f64 %[r], %[c4], %[u], %[c3]\n\t" \
    "v_fma_f64 %[p], %[s3], %[u], %[s2]\n\t" \
    "v_fma_f64 %[r], %[r], %[u], %[c2]\n\t" \
    "v_fma_f64 %[p], %[p], %[u], %[s1]\n\t" \
    "v_fma_f64 %[r], %[r], %[u], %[c1]\n\t" \
    "v_fma_f64 %[p], %[p], %[u], %[s0]\n\t" \
    "v_fma_f64 %[r], %[r], %[u], %[c0]\n\t" \
    "v_mul_f64 %[t], %[x], %[u]\n\t" \
    "v_fma_f64 %[xc], %[r], %[u], 1.0\n\t" \
    "v_fma_f64 %[xs], %[t], %[p], %[x]"
__device__ inline void expj_small(double kfs, double fo, const SinCosK& k, double& xs, double& xc) {
    double x, u, p, r, t;
    asm(OPV_EXPJ_ASM
        : [x] "=&v"(x), [u] "=&v"(u), [p] "=&v"(p), [r] "=&v"(r), [t] "=&v"(t), [xs] "=&v"(xs), [xc] "=&v"(xc)
        : [kfs] "v"(kfs), [fo] "v"(fo), [s0] "v"(k.s0), [s1] "v"(k.s1), [s2] "v"(k.s2), [s3] "v"(k.s3),
          [c0] "v"(k.c0), [c1] "v"(k.c1), [c2] "v"(k.c2), [c3] "v"(k.c3), [c4] "v"(k.c4));
}
// The steady-state form: the AFC clamp of the previous symbol's update (ref :302-303) and the LO factor of this symbol in ONE
// block, so that no padding stands between the clamp and the first product (hipcc pads an fp64 instruction behind an asm block).
__device__ inline void expj_small_clamped(double kfs, double fo_raw, double fo_lo, double fo_hi, const SinCosK& k, double& fo,
                                          double& xs, double& xc) {
    double x, u, p, r, t;
    asm("v_max_f64 %[fo], %[raw], %[lo]\n\t"
        "v_min_f64 %[fo], %[fo], %[hi]\n\t" OPV_EXPJ_ASM
        : [fo] "=&v"(fo), [x] "=&v"(x), [u] "=&v"(u), [p] "=&v"(p), [r] "=&v"(r), [t] "=&v"(t), [xs] "=&v"(xs), [xc] "=&v"(xc)
        : [raw] "v"(fo_raw), [lo] "v"(fo_lo), [hi] "v"(fo_hi), [kfs] "v"(kfs), [s0] "v"(k.s0), [s1] "v"(k.s1), [s2] "v"(k.s2), [s3] "v"(k.s3),
          [c0] "v"(k.c0), [c1] "v"(k.c1), [c2] "v"(k.c2), [c3] "v"(k.c3), [c4] "v"(k.c4));
}
#undef OPV_EXPJ_ASM

}  // namespace

#include "opv_atan2.h"  // kOpvAtanTabQ3R (constant-memory image of the angle table) + the host statement of the routine

// WPB = wavefronts (= streams) per workgroup. One wave per workgroup is the natural shape, but the dispatcher
// places single-wave workgroups without regard to SIMDs: with 1024 of them on the chip's 1024 SIMDs, 88 SIMDs
// received two waves and 88 none (census from this kernel's own HW_ID tap, profiles/r02_placement_1024_streams.txt),
// and the doubled-up waves - this kernel keeps a SIMD's fp64 pipe 80 % busy on its own - took 1.74x as long and set
// the kernel's duration. A 256-thread workgroup's four waves always land on the four SIMDs of one CU, so from 513
// streams on the shim launches four streams per workgroup (k_msk_frontend_wg4). Waves of a workgroup share nothing
// but the atan table.
// (A two-waves-per-stream mapping and the round-1 symbol body were measured against this one - 6 % and 25 % slower -
// and removed in round 6: NOTEBOOK.md has the measurements, git the code.)
typedef __attribute__((address_space(3))) volatile uint32_t lds_flag;
__device__ inline lds_flag* f64_flags(lbyte* lds_all) {
    return reinterpret_cast<lds_flag*>(lds_all + kF64FlagOff);
}

// Wave 1 of the fp64-ring shape: converts chunks of kF64Chunk samples ahead of the stream's wave, from the first tile the
// int16 path would stage (origin - kBack) up to past the last sample the stream's wave can request. Nothing at or past
// n_avail is read from memory: such samples (and the difference of the last one) are zeros, which no kept result uses
// (the highest tap of a symbol is sample origin + N - 1). Writes no OpvStream field.
__device__ void f64_ring_helper(const OpvStream& st, lbyte* lds_all) {
    const uint32_t lane = threadIdx.x & 63u;
    lds_flag* const fl = f64_flags(lds_all);
    const uint32_t n_avail = uni((uint32_t)st.n_avail), origin = uni((uint32_t)st.origin);
    const int* const iq = reinterpret_cast<const int*>(st.iq);   // one int = one int16 IQ pair
    uint32_t fill = ((origin >= kBack ? origin - kBack : 0u) / kF64Chunk) * kF64Chunk;
    const uint32_t fill_end = n_avail + kAhead + 2u;          // the stream's wave never waits for more (housekeeping)
    uint32_t spins = 0;
    while ((int)(fill - fill_end) < 0) {
        if (fl[2] != 0u) return;                               // the stream's wave has finished
        if ((int)(fl[0] + kF64Ring - fill - kF64Chunk) < 0) {  // the chunk's slots are still in use
            if (++spins > kHelperSpins) return;                // (the stream's wave times out on `ready` and says so)
            __builtin_amdgcn_s_sleep(8);
            continue;
        }
        spins = 0;
        // Lane l converts samples fill + l + 64 k: consecutive lanes write consecutive 32-byte entries, so the eight lanes
        // one ds_write_b128 group serves cover all 32 banks twice (2-way; four samples in a row per lane put a group's eight
        // lanes 128 B apart on the same four banks, 8-way, in bursts the stream's wave's tap reads queued behind). Sample n
        // and its successor as two dword loads, coalesced across the wave.
        constexpr uint32_t kPerLane = kF64Chunk / 64u;
        const uint32_t n0 = fill + lane;
        int w[kPerLane], wn[kPerLane];
        if (fill + kF64Chunk < n_avail) {                      // (wave-uniform) the chunk and the sample behind it exist
#pragma unroll
            for (uint32_t k = 0; k < kPerLane; ++k) { w[k] = iq[n0 + 64u * k]; wn[k] = iq[n0 + 64u * k + 1u]; }
        } else {
#pragma unroll
            for (uint32_t k = 0; k < kPerLane; ++k) {
                const uint32_t n = n0 + 64u * k;
                w[k] = n < n_avail ? iq[n] : 0;
                wn[k] = n + 1u < n_avail ? iq[n + 1u] : 0;
            }
        }
#pragma unroll
        for (uint32_t k = 0; k < kPerLane; ++k) {
            const int xr = (int)(short)(w[k] & 0xFFFF), xi = w[k] >> 16;
            const int yr = (int)(short)(wn[k] & 0xFFFF) - xr, yi = (wn[k] >> 16) - xi;
            ld2v* e = reinterpret_cast<ld2v*>(lds_all + kF64RingOff + (((n0 + 64u * k) & (kF64Ring - 1u)) << 5));
            e[0] = d2v{(double)xr, (double)xi};
            e[1] = d2v{(double)yr, (double)yi};
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // the entries before `ready`
        fill += kF64Chunk;
        if (lane == 0u) fl[1] = fill;
    }
}

template <int WPB, bool F64 = false>
__device__ __forceinline__ void msk_frontend_body(OpvStream* __restrict__ streams, OpvGlobalCfg cfg, int n_streams,
                                                  lbyte* lds_all) {
    const int lane = threadIdx.x & 63;
    const int wave = WPB == 1 ? 0 : __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (a constant 0 lets the ring base fold into the tap address)
    const int sidx = (int)blockIdx.x * WPB + wave;
    const uint64_t dbg_t0 = __builtin_amdgcn_s_memtime(), dbg_r0 = __builtin_amdgcn_s_memrealtime();

    lbyte* const lds = lds_all + (F64 ? kF64RingOff : wave * kTabOff);   // this wave's ring + guard (F64: the fp64 ring)
    const lbyte* ringb = lds;
    const ldouble* atab = reinterpret_cast<const ldouble*>(lds_all + (F64 ? kF64TabOff : WPB * kTabOff));   // filled by the kernel wrapper, barrier included
    if (sidx >= n_streams) return;       // a last, partly filled workgroup
    OpvStream& st = streams[sidx];

    // ---- per-lane constants -------------------------------------------------------------
    // rows of 15 samples (lane 16 r + n <-> sample 15 r + n, n < 15), so that the 60 samples take 15 broadcast steps per
    // row instead of 16. A row's last lane carries no weight - no row_newbcast:0..14 reads its Z - and is given sample 50
    // (kf = 40): its LO factor IS X[40], which the next symbol's phase detector needs in every lane, one row_newbcast:15
    // away in each row (its taps, floor(pos) + 40 and + 41, lie inside what kAhead guarantees in both rings)
    const int jsamp = (lane & 15) == 15 ? 50 : lane - (lane >> 4);
    const double kf = (double)(jsamp - 10);
    const double kfs = kf * kDeltaPerHz;
    // T_1[i] = exp(-j 2 pi i / 160) = (a, b) = (cos(pi i/80), -sin(pi i/80)); zero outside a gate's window.
    // Output t = lane & 15 of every row is one of the symbol's window sums, and wr[n] / wi[n] are the weights of
    // Re / Im Z of the row's n-th sample in it (see `symbol_r`). Correlations C_1 = sum Z conj(T_1[i]) = (sum Zr a + Zi b,
    // sum Zi a - Zr b), C_2 = sum Z T_1[i] = (sum Zr a - Zi b, sum Zi a + Zr b); Re in t, Im in t + 8:
    //   t = 0, 1   on-time correlation of tone 1 / tone 2 (S_1, S_2)                          (window j in [10, 50), i = j - 10)
    //   t = 2..5   early / late correlation of tone 1, then of tone 2 (E_1, L_1, E_2, L_2)    (early: j in [0, 40), i = j;
    //                                                                                           late: j in [20, 60), i = j - 20)
    //   t = 6, 7, 14, 15   the on-time sums P1 = sum Zr a, P2 = sum Zi b, P3 = sum Zi a, P4 = sum Zr b
    //              (S_1 = (P1 + P2, P3 - P4), S_2 = (P1 - P2, P3 + P4): what the phase detector and the carry use)
    double wr[15], wi[15];
    {
        const int row = lane >> 4, t = lane & 15, u = t & 7;
        const bool is_p = u >= 6, imag = t >= 8;
        const int gate = (u < 2 || is_p) ? 1 : ((u & 1) ? 2 : 0);  // 0 early, 1 on-time, 2 late (u = 2: E_1, 3: L_1, 4: E_2, 5: L_2)
        const bool tone2 = is_p ? false : (u < 2 ? u == 1 : u >= 4);
#pragma unroll
        for (int n = 0; n < 15; ++n) {
            const int i = 15 * row + n - 10 * gate;
            double sn, cs;
            sincospi((double)i / 80.0, &sn, &cs);
            const bool in = i >= 0 && i < 40;
            const double a = in ? cs : 0.0, b = in ? -sn : 0.0;
            double r_, i_;
            if (is_p) { r_ = (t == 6) ? a : (t == 15 ? b : 0.0); i_ = (t == 7) ? b : (t == 14 ? a : 0.0); }   // P1, P4 | P2, P3
            else if (!imag) { r_ = a; i_ = tone2 ? -b : b; }      // Re C_1 / C_2
            else { r_ = tone2 ? b : -b; i_ = a; }                 // Im C_1 / C_2
            wr[n] = r_; wi[n] = i_;
            asm volatile("" : "+v"(wr[n]), "+v"(wi[n]));
        }
    }
    SinCosK sck;
    sck.s0 = -0x1.5555555555412p-3; sck.s1 = 0x1.1111110f26395p-7; sck.s2 = -0x1.a019e48059d90p-13; sck.s3 = 0x1.7150a543fadc5p-19;
    sck.c0 = -0x1.0000000000000p-1; sck.c1 = 0x1.5555555555014p-5; sck.c2 = -0x1.6c16c16818f3fp-10;
    sck.c3 = 0x1.a019dfaa26924p-16; sck.c4 = -0x1.276f06eab6283p-22;
    // Loop constants parked in VGPRs: one wave per SIMD has registers to spare, while hipcc
    // otherwise keeps re-forming 64-bit literals in SGPR pairs inside the loop.
    double kc_tfmax = 0.1, kc_beta = 0.00001, kc_alpha = 0.005, kc_fomax = 2000.0, kc_eps = 1e-10;
    double kc_tiny = 1e-100, kc_m1 = -1.0;
    asm volatile("" : "+v"(kc_tiny), "+v"(kc_m1));
    double kc_halfpi = 1.57079632679489661923, kc_32 = 32.0, kc_m1_32 = -1.0 / 32.0, kc_gain = st.afc_alpha * (kSymRate / kTwoPi);
    // rows per unit of the angle table, its inverse, 1.5 * 2^52 + the row offset (the 1025 rows of opv_atan2_q3r)
    [[maybe_unused]] double kc_64 = 512.0, kc_m1_64 = -1.0 / 512.0, kc_magic = 6755399441055744.0 + 512.0;
    asm volatile("" : "+v"(kc_64), "+v"(kc_m1_64), "+v"(kc_magic));
    asm volatile("" : "+v"(kc_tfmax), "+v"(kc_beta), "+v"(kc_alpha), "+v"(kc_fomax), "+v"(kc_eps));
    asm volatile("" : "+v"(kc_halfpi), "+v"(kc_32), "+v"(kc_m1_32), "+v"(kc_gain));
    const double kc_nfomax = __builtin_canonicalize(-kc_fomax), kc_ntfmax = __builtin_canonicalize(-kc_tfmax);
    kc_fomax = __builtin_canonicalize(kc_fomax);
    kc_tfmax = __builtin_canonicalize(kc_tfmax);
    double sx = 1.0, nsg = 1.0;          // +/-1.0 rebuilt per symbol by rewriting the high word only
    asm volatile("" : "+v"(sx), "+v"(nsg));
    // Selectors of the cross-row sums (symbol_r): v_mfma_f64_4x4x4_4b_f64 takes A's contraction index k from lane bits 4-5, B's k
    // from lane bits 4-5 and its column and block from lane bits 0-3, and writes D's row to lane bits 4-5, column and block to
    // lane bits 0-3 (scripts/microbench/mfma_rows.hip, part 1). With A = sel[k] in every row and B = v, every lane 16 i + t
    // receives sum_k sel[k] * v[16 k + t]: selE picks rows 0 and 2, selO rows 1 and 3.
    // The bits are those of the swap tree (r0 + r2) + (r1 + r3): each MFMA adds two products 1.0 * r, which are exact, and two
    // exact zeros onto +0, so whatever the order inside the instruction, and with or without rounding between its steps, it
    // returns fl(r0 + r2) resp. fl(r1 + r3), and one v_add_f64 adds the two. A row partial is never -0 (both accumulators
    // start at +0 and a sum of products that cancels is +0), so a zero sum is +0 on both paths; with int16 input the partials
    // are finite and their non-zero values far from denormal (the smallest is about 1e-18), so 0 * r is a zero and never a NaN.
    double selE = ((lane >> 4) & 1) ? 0.0 : 1.0, selO = ((lane >> 4) & 1) ? 1.0 : 0.0;
    asm volatile("" : "+v"(selE), "+v"(selO));

    // ---- carry ---------------------------------------------------------------------------
    double fo = st.freq_offset, tf = st.timing_freq, mu = st.mu;
    PrevSums qp{st.p1r, st.p1i, st.p2r, st.p2i, st.x40c, st.x40s}, qq{0, 0, 0, 0, 1, 0};    // previous on-time P1..P4 (S_1 = (a+b, c-d), S_2 = (a-b, c+d))
    double fo_sum = st.fo_sum;
    uint32_t origin = uni((uint32_t)st.origin);
    const uint32_t n_avail = uni((uint32_t)st.n_avail);
    uint64_t n_soft = st.n_soft, total_samples = st.total_samples;
    uint32_t n_chunks = uni(st.n_chunks);
    int tail_done = (int)uni((uint32_t)st.tail_done);
    const int eof = (int)uni((uint32_t)st.eof);
    int overflow = (int)uni((uint32_t)st.overflow), stalled = 0;
    uint32_t edge_ties = uni(st.edge_ties);
    uint32_t calls_free = 0, calls_guarded = 0;   // demodulate() calls of this launch by the nest they took (opv_tap_frontend_calls)
    const uint64_t cap_soft = st.cap_soft;
    if (cap_soft > (1ull << 28)) overflow = 1;  // byte offsets into the soft ring are kept in 32 bits
    // oldest soft symbol the tracker may still read: its 24-symbol window, or the payload / next
    // sync check hanging off the current anchor
    uint64_t soft_keep = st.trk_next >= 24 ? st.trk_next - 24 : 0;
    if (st.trk_state != 0 && st.trk_anchor < soft_keep) soft_keep = st.trk_anchor;
    const uint32_t soft_bmask = (uint32_t)(cap_soft * 8u - 1u) & ~7u;
    // (in SGPRs, the store's base operand: hipcc reads the fp64-ring shape's context with vector loads)
    gbyte* const soft_base = (gbyte*)(((uint64_t)uni((uint32_t)((uint64_t)st.soft >> 32)) << 32) | uni((uint32_t)(uint64_t)st.soft));
    const gbyte* iq_bytes = (const gbyte*)st.iq;
    const uint64_t n_bytes = (uint64_t)n_avail * 4u;

    // ---- tile staging (wave-uniform state) ----------------------------------------------
    // Direct-to-LDS 16-byte load (global_load_lds_dwordx4): lane l moves 16 B from its own global
    // address to LDS byte (m0 + 16 l). Issued through inline asm on purpose: hipcc's waitcnt pass
    // would otherwise drain vmcnt(0) before EVERY later LDS read it cannot disambiguate from the
    // DMA destination. Completion is awaited explicitly with s_waitcnt vmcnt(0) one tile later
    // (see the tile events below).
    auto glds16 = [&](const gbyte* gsrc, uint32_t lds_byte) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(gsrc), "s"(uni(lds_byte))
                     : "memory");
    };
    const uint32_t lds_base = uni((uint32_t)(uintptr_t)lds);
    auto issue_tile = [&](uint32_t t) {
        // tile t -> slot t&1: 8 wave instructions; an even tile's first 16 B are mirrored into the
        // guard behind the ring. The capture's last, incomplete 16 bytes (n_avail not a multiple
        // of 4 samples) are copied sample by sample: nothing past n_avail is ever read.
        const uint64_t base = (uint64_t)t * OPV_TILE_BYTES;
        const uint32_t slot = (t & 1u) * OPV_TILE_BYTES;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const uint32_t in_tile = (uint32_t)r * 1024u + (uint32_t)lane * 16u;
            const uint64_t off = base + in_tile;
            if (off + 16u <= n_bytes) glds16(iq_bytes + off, lds_base + slot + (uint32_t)r * 1024u);
            else if (off < n_bytes) {
                for (uint32_t j = 0; off + 4u * j < n_bytes; ++j)
                    *reinterpret_cast<lint*>(lds + slot + in_tile + 4u * j) = *reinterpret_cast<const __attribute__((address_space(1))) int*>(iq_bytes + off + 4u * j);
            }
        }
        if ((t & 1u) == 0u && lane == 0) {
            if (base + 16u <= n_bytes) glds16(iq_bytes + base, lds_base + kRingBytes);
            else
                for (uint32_t j = 0; base + 4u * j < n_bytes && j < 4u; ++j)
                    *reinterpret_cast<lint*>(lds + kRingBytes + 4u * j) = *reinterpret_cast<const __attribute__((address_space(1))) int*>(iq_bytes + base + 4u * j);
        }
    };
    // lowest sample any lane can touch at the first symbol of this launch
    uint32_t t_lo = (origin >= kBack ? origin - kBack : 0u) / kTile;
    if constexpr (!F64) {
        issue_tile(t_lo);
        issue_tile(t_lo + 1u);
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): both tiles (and the guard) landed
    }
    bool evt_issue = true;               // next tile event: request tile t_lo+2 (else: wait for the newest)
    uint32_t next_evt = (t_lo + 1u) * kTile + kBack;
    // fp64 ring: wait until the helper has written every sample below `need` (bounded: a hand-over that times out ends
    // the stream's launch with overflow = 2, which opv_process reports)
    [[maybe_unused]] lds_flag* const fl = f64_flags(lds_all);
    [[maybe_unused]] auto f64_wait = [&](uint32_t need) {
        uint32_t r = uni(fl[1]);
        for (uint32_t spins = 0; (int)(r - need) < 0;) {
            if (overflow != 0 || ++spins > kF64WaitSpins) { overflow = 2; break; }
            __builtin_amdgcn_s_sleep(1);
            r = uni(fl[1]);
        }
        return r;
    };

    for (;;) {
        // ---- which demodulate() call comes next (ref :1026 / :1088 / :1173) ----------------
        const uint32_t remaining = n_avail - origin;
        uint32_t N;
        bool last = false;
        if (cfg.streaming) {
            if (remaining >= OPV_CHUNK) N = OPV_CHUNK;
            else if (eof && !tail_done && remaining > 0) { N = remaining; last = true; }
            else { if (eof) tail_done = 1; break; }
        } else {
            if (!eof || tail_done) break;
            N = n_avail;
            last = true;
        }
        // worst case one symbol per 38 samples: postpone the call rather than overrun soft symbols the tracker
        // still needs (back-pressure: it is retried next round, once frames have been popped)
        if (overflow) break;
        if ((n_soft - soft_keep) + (uint64_t)(N / 38u + 2u) > cap_soft) { stalled = 1; break; }

        const double Nd = (double)N;
        double pos = mu;                                   // ref :217
        const uint32_t soft_off0 = ((uint32_t)n_soft * 8u) & soft_bmask;  // ring byte offset of this call's first symbol
        // The offset of the next symbol to be logged, unwrapped: inside a batch of symbols the soft ring does not wrap
        // (housekeeping), so that a symbol's store is soft_v + a constant and only the batch boundary applies the ring mask.
        // soft_off: wave-uniform, advanced once per batch; soft_v: the store's address operand, one add per loop trip.
        uint32_t soft_off = soft_off0;
        uint32_t soft_v = soft_off0;
        asm volatile("" : "+v"(soft_v));
        auto soft_advance = [&](uint32_t nsym) {           // behind a batch of nsym symbols
            soft_off = (soft_off + 8u * nsym) & soft_bmask;
            soft_v = soft_off;
            asm volatile("" : "+v"(soft_v));
        };
        const uint32_t ring_c = (origin << 5) & (kF64RingBytes - 1u);   // fp64 ring: byte offset of the call's sample 0
        double fo_raw = fo;                                // the AFC's update before its clamp (symbol_r)

        // Tile bookkeeping for the symbol at `at` (wave-uniform, rare). Returns how many FOLLOWING
        // symbols need neither it nor the end-of-call test: pos advances by at most 42 samples per
        // symbol (|adj| <= 2, ref :285-286). `adv`: NoAdvance, or the symbols of the batch just finished (the fast boundary):
        // their soft_advance is done here, in the shadow of the flag read. A lost helper (overflow set by f64_wait) returns 0:
        // `ready` is then short of gb + kAhead + 2, so lim1 below is negative.
        using NoAdvance = std::integral_constant<uint32_t, 0>;
        auto housekeeping = [&](double at, auto adv) {
            // (the conversion on the VALU, ONE transfer to an SGPR; everything below is scalar arithmetic on it. Left alone,
            // hipcc moves both words of `at` to SGPRs, converts from there and moves the result back a third time.)
            uint32_t bv = (uint32_t)at;
            asm("" : "+v"(bv));
            const uint32_t b = uni(bv);
            const uint32_t gb = origin + b;                // global index of floor(pos)
            [[maybe_unused]] uint32_t ready_v = 0;
            if constexpr (F64) {
                // release the slots below the lowest tap, then take what the helper has written so far (it keeps
                // about a ring ahead, so the wait below only ever happens at the launch's first symbol)
                if (lane == 0) fl[0] = gb >= kBack ? gb - kBack : 0u;
                ready_v = fl[1];
                __builtin_amdgcn_sched_barrier(0);         // the scalar work below covers part of the read's latency
            }
            if constexpr (std::is_same_v<decltype(adv), uint32_t>) soft_advance(adv);
            int lim2 = (int)N - 52 - (int)b;
            // ... and while the soft ring does not wrap: soft_off is masked, so at least one symbol fits behind it
            uint32_t by_ring = ((soft_bmask + 8u - soft_off) >> 3) - 1u;
            if constexpr (F64) {
                asm volatile("" : "+s"(lim2), "+s"(by_ring));   // (formed here, not behind the wait where they are used)
                __builtin_amdgcn_sched_barrier(0);
                uint32_t ready = uni(ready_v);
                if (__builtin_expect((int)(ready - gb) < (int)(kAhead + 2u), 0)) ready = f64_wait(gb + kAhead + 2u);
                asm volatile("" ::: "memory");             // no tap read is hoisted above `ready`
                next_evt = ready - kAhead;                 // taps of a symbol at gb' < next_evt lie below `ready`
            }
            while (!F64 && gb >= next_evt) {
                if (evt_issue) {
                    // the lowest tap has left tile t_lo for good: refill its slot with tile
                    // t_lo+2 (asynchronous; first needed a whole tile = ~51 symbols from now)
                    issue_tile(t_lo + 2u);
                    ++t_lo;
                    evt_issue = false;
                    next_evt = (t_lo + 1u) * kTile - kAhead;
                } else {
                    __builtin_amdgcn_s_waitcnt(0x0F70);    // vmcnt(0): requested a tile ago, no stall
                    evt_issue = true;
                    next_evt = (t_lo + 1u) * kTile + kBack;
                }
            }
            // j more symbols are safe iff gb + 42 j + 1 < next_evt and b + 1 + 42 j + 50 <= N
            const int lim1 = (int)(next_evt - gb) - 2;
            int lim = lim1 < lim2 ? lim1 : lim2;
            if (lim < 0) lim = 0;
            const uint32_t by_samples = ((uint32_t)lim * 1560u) >> 16;     // <= floor(lim / 42), lim < 2^17
            return by_samples < by_ring ? by_samples : by_ring;
        };

        // One interpolated sample per lane (ref :122-128, :232-238): the two int16 IQ words around
        // pos + kf. Issued for symbol k+1 as soon as pos(k+1) exists.
        int w0 = 0, w1 = 0;
        [[maybe_unused]] d2v x0{0.0, 0.0}, dx{0.0, 0.0};   // F64: (x_r, x_i)[idx] and the difference to idx + 1
        double f = 0.0;
        uint32_t tap_byte = 0;
        auto fetch_addr = [&](double at, bool clamp0) {
            double p = at + kf;
            if (clamp0) p = fmax(p, 0.0);                  // early gate before the chunk: s[0] (ref :237)
            const int idx = (int)p;
            f = __builtin_amdgcn_fract(p);                 // p - idx, p >= 0
            // fp64 ring: exactly 2^16 bytes, so (32 idx + ring_c) mod 2^16 is one 16-bit multiply-add. tap_byte is written by
            // nothing else in this shape and starts as 0: its high half is 0 whether the instruction clears or keeps it.
            if constexpr (F64) asm("v_mad_legacy_u16 %0, %1, 32, %2" : "+v"(tap_byte) : "v"(idx), "s"(ring_c));
            else tap_byte = (((uint32_t)idx + origin) << 2) & (kRingBytes - 4u);
        };
        auto fetch_read = [&]() {
            if constexpr (F64) {
                const ld2v* tap = reinterpret_cast<const ld2v*>(ringb + tap_byte);
                x0 = tap[0];
                dx = tap[1];
            } else {
                const lint* tap = reinterpret_cast<const lint*>(ringb + tap_byte);
                w0 = tap[0];
                w1 = tap[1];
            }
        };
        auto fetch = [&](double at, bool clamp0) {
            fetch_addr(at, clamp0);
            fetch_read();
        };

        // One symbol, with the ROW-BROADCAST reduction. gfx950's DP-ALU DPP form
        //   v_fmac_f64_dpp acc, src0 row_newbcast:n, src1      acc[l] += src0[row(l), lane n] * src1[l]
        // lets the 16 lanes of a row form 16 differently weighted sums of the row's samples, one broadcast step per
        // sample and component: 2 x 15 full-rate FMACs produce ALL twelve window sums of the symbol (on-time P1..P4, early
        // and late correlations of BOTH tones) as row partials in lanes t = lane & 15, with no product instructions, no
        // dominant-tone dependence and no v_readlane. One all-reduce over the four rows (two v_mfma_f64_4x4x4 that each sum
        // two rows, and an add) completes them; v_mov_b64_dpp row_newbcast hands the numbers the loop filters need to
        // every lane (one instruction per double instead of two v_readlane + the SGPR-operand restrictions), and the four
        // early / late energies are formed lane-parallel (square, row_ror:8, add: Re at t, Im at t + 8), the dominant
        // tone's pair selected lane-parallel (row_shl:2), before two of them are handed out. The phase detector's angle
        // comes without the octant fix-up (opv_atan2.h: opv_atan2_q3r, 1025-row table of pi/4 + atan, cubics in the argument itself; round 2: 257 rows, degree 5).
        // Scheduling notes: hipcc counts an asm block as no wait state and pads behind one, so neighbouring pieces are ONE block
        // (the AFC clamp with the LO factor, the thirty FMACs with the sum and the all-reduce, the tone compare with the P3 / P4
        // hand-outs and the selects), and the wait states DPP reads / MFMAs need behind a VALU write are filled with
        // useful instructions where there are any: three s_nop per symbol remain (two behind the MFMA pair, nothing
        // independent is cheap there; one behind the select block). (scripts/microbench/dpp64.hip has the instruction costs.)
        [[maybe_unused]] double soft_held = 0.0;               // the soft value of a trip's slot 0 / 2 until slot 1 / 3 stores the pair
        auto symbol_r = [&](auto tag, auto slot, PrevSums& cur, const PrevSums& prv) {
            constexpr bool kFirst = decltype(tag)::first;
            constexpr bool kWide = decltype(tag)::wide;
            constexpr uint32_t kSlot = decltype(slot)::value;          // the symbol's place in its loop trip: logged at soft_v + 8 kSlot
            // The LO factor FIRST: it needs fo only, and its twelve instructions are the cover the tap read of the previous
            // symbol's tail still lacked (round 3: without that read the kernel ran 34 cycles per symbol faster, i.e. ~26 of
            // its latency were exposed when the unpack below came first)
            double xs, xc;
            if constexpr (kWide) {
                if (__builtin_expect(uni_lt(2000.0, fabs(fo)), 0)) sincos(kfs * fo, &xs, &xc);
                else expj_small(kfs, fo, sck, xs, xc);
            } else {
                expj_small_clamped(kfs, fo_raw, kc_nfomax, kc_fomax, sck, fo, xs, xc);   // fo: the previous symbol's update, clamped here
            }
            __builtin_amdgcn_sched_barrier(0);
            double lr, li;
            if constexpr (F64) {                                            // the same operands, widened by the helper
                lr = fma(f, dx.x, x0.x);
                li = fma(f, dx.y, x0.y);
            } else {
                const int s0r = (int)(short)(w0 & 0xFFFF), s0i = w0 >> 16;      // ref :1023
                const int d_r = (int)(short)(w1 & 0xFFFF) - s0r, d_i = (w1 >> 16) - s0i;
                lr = fma(f, (double)d_r, (double)s0r);                          // ref :122-128
                li = fma(f, (double)d_i, (double)s0i);
            }
            const double zr = fma(lr, xc, li * xs);                         // Z = Lam * conj(X)
            const double zi = fma(li, xc, -(lr * xs));
            __builtin_amdgcn_sched_barrier(0);

            // ---- 1. the twelve window sums: row partials by broadcast-FMAC into two accumulators (the two moves are
            // the wait states a DPP read needs behind the VALU write of Z)
            double acc0, acc1, v, t;
#define OPV_RB(N) "v_fmac_f64_dpp %[a0], %[zr], %[r" #N "] row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t" \
                  "v_fmac_f64_dpp %[a1], %[zi], %[i" #N "] row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t"
            // One block with the all-reduce over the four rows behind the thirty FMACs: the sum of the two accumulators, then two
            // independent v_mfma_f64_4x4x4 with the row selectors (at `selE`: why the bits are the swap tree's (r0 + r2) + (r1 + r3))
            // and one add. The X[40] hand-over (the spare lane 15 of every row carries sample 50: two DPP moves, equal in every
            // lane) stands IN FRONT of the pair, as the two wait states an MFMA needs behind the VALU write of its operand: behind
            // the pair, in the six wait states its result needs, the same two moves cost 20 cycles (mfma_rows.hip; in the loop 13
            // cycles per symbol slower than the swaps). Those six are s_nop 3 + s_nop 1 and not one s_nop 5: a lone 4-byte
            // instruction flips the parity of the eleven 8-byte instructions behind it, which tools/align_vop3.py has nothing
            // to widen against (11 cycles per symbol, profiles/rowsum_mfma_step0.txt).
            asm("v_mov_b64 %[a0], 0\n\tv_mov_b64 %[a1], 0\n\t" OPV_RB(0) OPV_RB(1) OPV_RB(2) OPV_RB(3) OPV_RB(4) OPV_RB(5) OPV_RB(6) OPV_RB(7)
                OPV_RB(8) OPV_RB(9) OPV_RB(10) OPV_RB(11) OPV_RB(12) OPV_RB(13) OPV_RB(14)
                "v_add_f64 %[t], %[a0], %[a1]\n\t"
                "v_mov_b64_dpp %[x40c], %[xc] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b64_dpp %[x40s], %[xs] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                "v_mfma_f64_4x4x4_4b_f64 %[a0], %[selE], %[t], 0\n\t"
                "v_mfma_f64_4x4x4_4b_f64 %[a1], %[selO], %[t], 0\n\t"
                "s_nop 3\n\ts_nop 1\n\t"
                "v_add_f64 %[v], %[a0], %[a1]"
                : [a0] "=&v"(acc0), [a1] "=&v"(acc1), [v] "=&v"(v), [t] "=&v"(t), [x40c] "=&v"(cur.x40c), [x40s] "=&v"(cur.x40s)
                : [zr] "v"(zr), [zi] "v"(zi), [r0] "v"(wr[0]), [i0] "v"(wi[0]), [r1] "v"(wr[1]), [i1] "v"(wi[1]), [r2] "v"(wr[2]), [i2] "v"(wi[2]),
                  [r3] "v"(wr[3]), [i3] "v"(wi[3]), [r4] "v"(wr[4]), [i4] "v"(wi[4]), [r5] "v"(wr[5]), [i5] "v"(wi[5]),
                  [r6] "v"(wr[6]), [i6] "v"(wi[6]), [r7] "v"(wr[7]), [i7] "v"(wi[7]),
                  [r8] "v"(wr[8]), [i8] "v"(wi[8]), [r9] "v"(wr[9]), [i9] "v"(wi[9]), [r10] "v"(wr[10]), [i10] "v"(wi[10]),
                  [r11] "v"(wr[11]), [i11] "v"(wi[11]), [r12] "v"(wr[12]), [i12] "v"(wi[12]), [r13] "v"(wr[13]), [i13] "v"(wi[13]),
                  [r14] "v"(wr[14]), [i14] "v"(wi[14]), [xc] "v"(xc), [xs] "v"(xs), [selE] "v"(selE), [selO] "v"(selO));
#undef OPV_RB
            __builtin_amdgcn_sched_barrier(0);
            double fo_sum_next = fo_sum + fo;                       // sum of the fo every symbol USED
            asm volatile("" : "+v"(fo_sum_next));
            const double sq = v * v;
            __builtin_amdgcn_sched_barrier(0);
            // energies, lane-parallel (Re at t, Im at t + 8): t = 0..5 -> |S_1|^2, |S_2|^2 (on-time), |E_1|^2, |L_1|^2, |E_2|^2, |L_2|^2
            const double shv = mkd(__builtin_amdgcn_mov_dpp(dhi(v), 0x128, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(dlo(v), 0x128, 0xF, 0xF, true));
            const double en = fma(shv, shv, sq);
            __builtin_amdgcn_sched_barrier(0);
            // on-time sums P1, P2 to every lane (`old` operands: dead temporaries of the stages above; the two moves are en's
            // wait states before the DPP reads below); P3, P4 follow further down
            const double P1o = row_bcast<6>(zr, v), P2o = row_bcast<7>(zi, v);
            __builtin_amdgcn_sched_barrier(0);
            // soft value = |S_2|^2 - |S_1|^2 (ref :264-268): the difference of the two energies like the reference, each from its
            // own correlation. (Where the reference's tones tie exactly - a real or imaginary Z - so do these: the two
            // correlations' accumulation chains are mirror images.) Two instructions: |S_2|^2 handed out by one DPP move, then
            // soft += |S_1|^2 * -1.0 by one v_fmac_f64_dpp whose first source is the row's lane 0 (the first instruction of the
            // block below). The product with -1.0 is exact and the sum is rounded once: en2 - en1 bit for bit, a tie gives +0.
            double soft = row_bcast<1>(acc1, en);
            __builtin_amdgcn_sched_barrier(0);
            // The dominant tone's early / late pair moves to t = 2, 3, then one hand-out each; tone 1 iff e1 > e2 (ref :272 / :291;
            // a tie gives +0: tone 2). Shift and select are ONE instruction per word: v_cndmask_b32_dpp takes its first source
            // through row_shl:2 (tone 2's pair, two lanes up) and keeps the lane's own word where vcc is set. The hand-outs of
            // P3, P4 stand between the compare and the selects (the two wait states a DPP instruction is given behind a write
            // it depends on); en was written seven instructions earlier.
            double P3o, P4o;
            int sel_lo, sel_hi;
            asm(
                "v_fmac_f64_dpp %[soft], %[en], %[m1] row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
                "v_cmp_gt_f64 vcc, 0, %[soft]\n\t"
                "v_mov_b64_dpp %[p3], %[v] row_newbcast:14 row_mask:0xf bank_mask:0xf\n\t"
                "v_mov_b64_dpp %[p4], %[v] row_newbcast:15 row_mask:0xf bank_mask:0xf\n\t"
                "v_cndmask_b32_dpp %[sl], %[el], %[el], vcc row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1\n\t"
                "v_cndmask_b32_dpp %[sh], %[eh], %[eh], vcc row_shl:2 row_mask:0xf bank_mask:0xf bound_ctrl:1"
                : [p3] "=&v"(P3o), [p4] "=&v"(P4o), [sl] "=&v"(sel_lo), [sh] "=&v"(sel_hi), [soft] "+v"(soft)
                : [v] "v"(v), [en] "v"(en), [m1] "v"(kc_m1), [el] "v"(dlo(en)), [eh] "v"(dhi(en))
                : "vcc");
            const double seln = mkd(sel_hi, sel_lo);
            __builtin_amdgcn_sched_barrier(0);
            // sg = +1 for tone 1, -1 for tone 2 (the sign insert is the 32-bit instruction hipcc wants behind an asm block)
            nsg = mkd((dhi(soft) & (int)0x80000000) | (dhi(nsg) & 0x7fffffff), dlo(nsg));
            asm volatile("" : "+v"(nsg));                           // (updated in place: no copy of the low word)
            const double sg = -nsg;
            __builtin_amdgcn_sched_barrier(0);

            [[maybe_unused]] double pd = 0.0, cx = 0, cy = 0, sum = 1.0, dif = 0, dm_ = 1.0, ee, el;
            [[maybe_unused]] uint64_t zmask = 0;
            if constexpr (!kFirst) {
                // hand-outs of the two energies, HERE: they are the wait state between the sign insert above and the first fma
                // that reads nsg (an s_nop otherwise), and the pad hipcc puts behind the select block (soft is one of its
                // outputs, the sign insert reads it) and that insert are the two wait states their own DPP reads of seln need
                ee = row_bcast<2>(sq, seln); el = row_bcast<3>(shv, seln);
                __builtin_amdgcn_sched_barrier(0);
                // phase detector operands: dom * conj(prev) (ref :299), prev advanced by one symbol's LO rotation
                // (header: P_t = S_t (-/+ j) X[40]); sg picks the dominant tone's combination of the shared sums
                const double dr = fma(sg, P2o, P1o), di = fma(-sg, P4o, P3o);
                const double prs = fma(sg, prv.a, prv.b), pis = fma(sg, prv.c, -prv.d);
                const double ar = fma(dr, prs, di * pis), ai = fma(di, prs, -(dr * pis));
                cy = fma(ar, prv.x40c, ai * prv.x40s);              // Im z
                cx = fma(ar, prv.x40s, -(ai * prv.x40c));           // Re z
                __builtin_amdgcn_sched_barrier(0);
                // cx < 0: pi - pd, as a +/-1 multiplier and a 0/pi offset built from the sign bit
                sx = mkd((dhi(cx) & (int)0x80000000) | (dhi(sx) & 0x7fffffff), dlo(sx));
                asm volatile("" : "+v"(sx));
                sum = fabs(cx) + fabs(cy); dif = fabs(cy) - fabs(cx);
                // the divisor's guard against digital silence: sum + 1e-100 IS sum unless sum is 0 (a non-zero sum of
                // products of window sums is far above 1e-84), and an add needs no canonicalised operand where fmax does
                dm_ = sum + kc_tiny;
                // One wave per workgroup (WPB == 1): the silence test's compare HERE, its branch 35 instructions later - a v_cmp
                // whose mask a scalar branch reads in the next instruction costs a lone wave a VALU -> SALU round trip (798 ->
                // 774 cycles per symbol on clean 60-frame streams, 779 -> 774 on the bench workload). The mask is left to hipcc
                // as a plain value: the compare lands here (the sched_barriers keep it in this stretch), writes vcc, and the
                // branch is one s_cbranch_vccnz - nothing between the two touches vcc (the tone select stands in front), and
                // if that ever changes hipcc copies the mask and scripts/experiments/trip_census.py shows the copy. (Pinned
                // through an opaque SGPR pair it cost an s_cmp per symbol: 8.2 cycles.) Four waves per workgroup keep the
                // adjacent pair: with the CU's other three SIMDs busy the early form measured 850 cycles per symbol against
                // 804 (1024 streams).
                if constexpr (WPB == 1) zmask = __builtin_amdgcn_fcmp(sum, 0.0, 1 /*FCMP_OEQ*/);
            } else {
                ee = row_bcast<2>(sq, seln); el = row_bcast<3>(shv, seln);
            }
            const double den = el + ee + kc_eps;                    // ted = num/den (ref :275/:279)

            // ---- 3. divides (one reciprocal for both), timing loop, AFC --------------------------------
            double ted, h = 0;
            [[maybe_unused]] d2v c01{0, 0}, c23{0, 0};
            if constexpr (kFirst) {
                double y = __builtin_amdgcn_rcp(den);
                const double num = el - ee;
                y = fma(fma(-den, y, 1.0), y, y);
                y = fma(fma(-den, y, 1.0), y, y);
                ted = num * y;
                ted = fma(fma(-den, ted, num), y, ted);
            } else {
                const double dm = dm_;                              // max(|cx| + |cy|, 1e-100); digital silence: 0/1e-100 = 0, fixed up below
                const double tt = den * dm;
                double y = __builtin_amdgcn_rcp(tt);
                const double num = el - ee;                         // (fills the wait state behind the reciprocal)
                // ONE Newton step: v_rcp_f64 is good to 2^-24.4, one step to 2^-48.7, and both quotients below get their
                // own residual step - the same error profile as with two (scripts/microbench/rcp_accuracy.hip)
                y = fma(fma(-tt, y, 1.0), y, y);
                const double iden = y * dm, idm = y * den;
                // q = (|cy| - |cx|) / (|cy| + |cx|) in [-1, 1], good to 2^-48 without a residual step: 3.5e-15 rad on the
                // angle, i.e. 3e-14 Hz x afc_alpha / 0.001 on fo - nothing rounds on it the way pos does on ted
                const double ratio = dif * idm;
                // nearest expansion point k/128, k = -128..128, by the 1.5 * 2^52 trick: the sum's low word IS the row index
                // k + 128, and subtracting the constant gives k as a double - no v_rndne, no v_cvt
                const double kt = fma(ratio, kc_64, kc_magic);
                h = ratio;                                          // (the rows' cubics are written in the argument itself)
                const lbyte* rowb = reinterpret_cast<const lbyte*>(atab) + ((unsigned)dlo(kt) << 5);
                const ld2v* trow = reinterpret_cast<const ld2v*>(rowb);
                c23 = trow[1]; c01 = trow[0];
                ted = num * iden;
                ted = fma(fma(-den, ted, num), iden, ted);
            }
            __builtin_amdgcn_sched_barrier(0);
            // beta (ref :118,:283-284). Without the clamp where the call's proof holds (opv_tf_rule.h: opv_tf_clamp_cannot_act):
            // fmin(fmax(x, -0.1), 0.1) returns every non-NaN x inside the bounds unchanged, so the bits are the same.
            if constexpr (decltype(tag)::tf_free) tf = fma(kc_beta, ted, tf);
            else tf = clampd(fma(kc_beta, ted, tf), kc_ntfmax, kc_tfmax);
            const double adj = fma(kc_alpha, ted, tf);                // alpha (ref :117,:285); the +/-2 clamp (:286) cannot act
            pos += 40.0 + adj;                                        // ref :313
            fetch_addr(pos, false);
            __builtin_amdgcn_sched_barrier(0);
            fetch_read();                                             // next symbol's taps requested as soon as their address exists
            __builtin_amdgcn_sched_barrier(0);
            if constexpr (decltype(slot)::paired) {
                if constexpr ((kSlot & 1u) == 0u) soft_held = soft;
                else *(gd2v8*)(soft_base + soft_v + 16u * (kSlot / 2u)) = d2v{soft_held, soft};
            } else
            *(gdouble*)(soft_base + soft_v + 8u * kSlot) = soft;      // (the slot's 8 kSlot is the store's immediate offset)
            // (a trip of four: slots 0 and 2 hold their value - a register, no instruction - and slots 1 and 3 store both as one
            // global_store_dwordx4 at soft_v + 16 (kSlot / 2). A batch of whole trips does not wrap the soft ring, so the pair is
            // contiguous; every trip is run whole, so nothing is held at any way out of the loop; the silence block of slot 1
            // reads and writes other registers. In the loop 3.7 cycles per symbol, profiles/rowsum_mfma_step0.txt.)
            if constexpr (!kFirst) {
                const double pd_off = fma(-sx, kc_halfpi, kc_halfpi);
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (F64) __builtin_amdgcn_s_waitcnt(0xC27F);   // lgkmcnt(2): the table row landed (the two tap reads may be in flight)
                else __builtin_amdgcn_s_waitcnt(0xC17F);            // lgkmcnt(1): the table row landed (only the tap read may be in flight)
                __builtin_amdgcn_sched_barrier(0);
                pd = fma(c23.y, h, c23.x);                          // the row's cubic in q: pi/4 + atan(q) to 4e-14 rad
                pd = fma(pd, h, c01.y);
                pd = fma(pd, h, c01.x);
                pd = fma(sx, pd, pd_off);
                pd = mkd((dhi(pd) & 0x7fffffff) | (dhi(cy) & (int)0x80000000), dlo(pd));  // sign of cy
                if (__builtin_expect(WPB == 1 ? zmask != 0ull : uni_eq(sum, 0.0), 0)) {   // digital silence on either side
                    const double dr = fma(sg, P2o, P1o), di = fma(-sg, P4o, P3o);
                    const double2 sp = silence_pd(dr, di, prv, soft < 0.0, fo_sum, n_soft + (((soft_v + 8u * kSlot - soft_off0) & soft_bmask) >> 3),
                                                  P1o, P2o, P3o, P4o);
                    pd = sp.x;
                    edge_ties += uni((uint32_t)sp.y);
                }
                fo_raw = fma(kc_gain, pd, fo);                      // ref :300-303; clamped by the next symbol, or by fo_settle
            }
            fo_sum = fo_sum_next;
            cur.a = P1o; cur.b = P2o; cur.c = P3o; cur.d = P4o;     // prev <- this symbol's on-time correlations (ref :309-310)
        };

        // behind the last symbol of a batch: the AFC clamp its successor would have applied (idempotent: the successor applies it again)
        auto fo_settle = [&]() {
            asm("v_max_f64 %0, %1, %2\n\tv_min_f64 %0, %0, %3" : "=&v"(fo) : "v"(fo_raw), "v"(kc_nfomax), "v"(kc_fomax));
            fo_raw = fo;
        };
        using Slot0 = SlotTag<0, false>;
        using Slot1 = SlotTag<1, false>;
        using Trip0 = SlotTag<0, true>;
        using Trip1 = SlotTag<1, true>;
        using Trip2 = SlotTag<2, true>;
        using Trip3 = SlotTag<3, true>;
        auto sym = [&](auto tag, auto slot, PrevSums& cur, const PrevSums& prv) { symbol_r(tag, slot, cur, prv); };

        // The call's symbols, from the first one through the batch loop, in two instantiations chosen once per call (below):
        // `steady` is TagSteady, or TagSteadyFree where the timing clamp provably cannot act in this call. The first symbol and
        // the second one under an out-of-range -o keep the clamp in both.
        auto call_symbols = [&](auto steady) {
        if (uni_lt(pos + 40.0 + 10.0, Nd)) {               // ref :221
            (void)housekeeping(pos, NoAdvance{});
            fetch(pos, true);
            sym(TagFirst{}, Slot0{}, qp, qp);
            soft_advance(1u);
            if (__builtin_expect(uni_lt(2000.0, fabs(fo)), 0) && uni_lt(pos + 40.0 + 10.0, Nd)) {
                (void)housekeeping(pos, NoAdvance{});      // an out-of-range -o is still in force for one more symbol
                fetch(pos, false);
                sym(TagSecond{}, Slot0{}, qq, qp);
                fo_settle();
                soft_advance(1u);
                qp = qq;
            }
            // Batches: the end-of-call test and the tile events once, then as many symbols as are
            // provably clear of both. Every symbol fetches its successor's taps; behind a remainder
            // batch that fetch is speculative (LDS only, harmless) and is repeated after the
            // bookkeeping, behind a batch of whole trips it is known good and kept (below).
            while (uni_lt(pos + 40.0 + 10.0, Nd)) {        // ref :221
                uint32_t more = uni(housekeeping(pos, NoAdvance{}));   // symbols behind the one at pos that are clear of both tests
                if (F64 && overflow != 0) break;           // the helper was lost (f64_wait)
                fetch(pos, false);
                // The fast boundary: batches of whole four-symbol trips (a taken branch costs a lone wave 36 cycles,
                // scripts/microbench/dpp64.hip, empty loop), from housekeeping straight back to housekeeping.
                //  * After a whole trip the previous sums are in qp again: nothing is copied.
                //  * fo stays unsettled: fo_raw is carried, and the next symbol clamps it as it does inside a trip. Every way
                //    out of here settles it (the remainder path below ends in fo_settle; the overflow exit calls it).
                //  * The symbol behind the batch has index 4 quads <= more, so housekeeping's promise covers it: it exists
                //    (the `while` test is known true and is not evaluated), and its taps lie below `ready` / inside landed
                //    tiles and inside the call. The batch's last symbol has already read them and they are NOT read again.
                //    That read stays valid across the housekeeping that follows it: the new `low` is posted behind the read
                //    in program order and one wave's LDS operations execute in order, the taps (>= floor(pos) - 10) are at or
                //    above the new `low` as well, and the helper never writes a slot at or above `low`; on the int16 ring a
                //    tile request refills the slot of tile t_lo only once the lowest tap has left it.
                // (The s_nop in front of each nest put its trip loop's top at 8 mod 32: the same loop ran 5.6 cycles per symbol
                // slower at 16 mod 32. tools/align_vop3.py reports both addresses at every build and says how many to add when
                // code in front of here has moved one; the two nests carry their own counts. The fp64 ring only: with two waves per CU, 512 streams on the int16 ring,
                // a loop so placed measured 1.2 % slower than where hipcc happened to put it. NOTEBOOK.md, Round 13.)
                if constexpr (F64 && decltype(steady)::tf_free) asm volatile("; opv_symbol_loop_top\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0\n\ts_nop 0");
                else if constexpr (F64) asm volatile("; opv_symbol_loop_top\n\ts_nop 0\n\ts_nop 0");
                while (more >= 4u) {
                    for (uint32_t quads = more >> 2; quads != 0u; --quads) {
                        sym(steady, Trip0{}, qq, qp);
                        sym(steady, Trip1{}, qp, qq);
                        sym(steady, Trip2{}, qq, qp);
                        sym(steady, Trip3{}, qp, qq);
                        soft_v += 32u;
                    }
                    more = uni(housekeeping(pos, more & ~3u));   // (0 once the helper is lost)
                }
                if (F64 && overflow != 0) { fo_settle(); break; }
                // The remainder (more < 4: the first batches of a launch, the last symbols of a call, a batch the soft ring
                // cuts short): symbols in pairs so that the "previous" registers alternate, one last symbol, settle, copy.
                uint32_t pairs = more >> 1;
                const uint32_t batch = 2u * pairs + 1u;    // symbols of this batch: they fit in front of the soft ring's wrap
                for (; pairs != 0u; --pairs) {
                    sym(steady, Slot0{}, qq, qp);
                    sym(steady, Slot1{}, qp, qq);
                    soft_v += 16u;
                }
                sym(steady, Slot0{}, qq, qp);
                fo_settle();
                soft_advance(batch);
                qp = qq;
            }
        }
        };
        // Once per call, wave-uniform: can the timing clamp act on any symbol of it? (tf moves by kc_beta |ted| per symbol.)
        // Both nests compute the same bits wherever the rule holds; where it does not, the guarded nest is the reference's text.
        // tf cannot turn NaN inside a call (den >= 1e-10 and dm >= 1e-100 keep ted finite on int16 input), and a NaN handed in
        // fails the rule.
        const double tf_uni = mkd((int)uni((uint32_t)dhi(tf)), (int)uni((uint32_t)dlo(tf)));
        if (cfg.tf_guard == 0 && opv_tf_clamp_cannot_act(tf_uni, N)) { ++calls_free; call_symbols(TagSteadyFree{}); }
        else { ++calls_guarded; call_symbols(TagSteady{}); }

        // ---- end of this demodulate() call (ref :318-328, :1067-1076) ------------------------
        const uint32_t nsym_call = ((soft_off - soft_off0) & soft_bmask) >> 3;
        const uint32_t used = uni((uint32_t)pos);
        mu = pos - (double)used;
        const uint32_t leftover = N - used;
        if (lane == 0) {                                   // chunk log is a ring
            double* c = st.chunk_log + 5 * (size_t)(n_chunks % st.cap_chunks);
            c[0] = fo;
            c[1] = tf; c[2] = mu; c[3] = (double)leftover; c[4] = (double)nsym_call;
        }
        ++n_chunks;
        n_soft += nsym_call;
        total_samples += N;
        origin += (leftover > 0u && leftover < N) ? used : N;
        if (last) { tail_done = 1; break; }
    }

    if constexpr (F64) {
        if (lane == 0) fl[2] = 1u;                         // the helper may leave
    }
    if (lane == 0) {
        st.freq_offset = fo;
        st.p1r = qp.a; st.p1i = qp.b; st.p2r = qp.c; st.p2i = qp.d; st.x40c = qp.x40c; st.x40s = qp.x40s;
        st.fo_sum = fo_sum;
        st.edge_ties = edge_ties;
        st.timing_freq = tf; st.mu = mu;
        st.origin = origin; st.n_soft = n_soft; st.total_samples = total_samples;
        st.n_chunks = n_chunks; st.tail_done = tail_done; st.overflow = overflow;
        st.stalled = stalled;
        st.fe_calls_free += calls_free; st.fe_calls_guarded += calls_guarded;
        // where and at which clock this stream's wave ran (two scalar reads per launch; opv_tap_wave_info)
        unsigned hw, xcc;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
        st.dbg_hw_id = hw; st.dbg_xcc_id = xcc;
        st.dbg_cycles = __builtin_amdgcn_s_memtime() - dbg_t0;
        st.dbg_ticks = __builtin_amdgcn_s_memrealtime() - dbg_r0;
    }
}

// the front-end kernels: one wave per stream, one or four waves (streams) per workgroup
template <int NT>
__device__ __forceinline__ void load_atan_table_q(lbyte* lds_tab) {
    ldouble* atab = reinterpret_cast<ldouble*>(lds_tab);
    for (int i = threadIdx.x; i < 1025 * 4; i += NT) atab[i] = (&kOpvAtanTabQ3R[0][0])[i];
}
// k_msk_frontend_rb has two launch shapes (opv_process): 64 threads, OPV_RB_LDS_I16 bytes of dynamic LDS = the int16 ring;
// 128 threads, OPV_RB_LDS_F64 bytes = wave 0 on the fp64 ring that wave 1 fills (f64_ring_helper)
extern "C" __global__ __launch_bounds__(128) void k_msk_frontend_rb(OpvStream* __restrict__ streams, OpvGlobalCfg cfg,
                                                                     int n_streams) {
    // All of the kernel's LDS is dynamic and starts at LDS address 0 (it has no static LDS; opv_create checks that). Its map
    // starts at the constant kRbLdsBase, not at an extern array's symbol, so that ring and table offsets fold into the ds_read
    // offset fields as they did with a static array (and not at 0: no pointer of the kernel is a null pointer).
    lbyte* const lds_dyn = reinterpret_cast<lbyte*>(kRbLdsBase);
    if (blockDim.x == 128) {
        load_atan_table_q<128>(lds_dyn + kF64TabOff);
        if (threadIdx.x == 0) {   // (plain stores: the barrier orders them before every wave's first look at a flag; wave 0
                                  // posts `low` at its first batch, before it waits for `ready`)
            __attribute__((address_space(3))) uint32_t* const fl = reinterpret_cast<__attribute__((address_space(3))) uint32_t*>(lds_dyn + kF64FlagOff);
            fl[0] = 0u;                                       // low
            fl[1] = 0u;                                       // ready
            fl[2] = 0u;                                       // done
        }
        __syncthreads();
        if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) != 0) {   // (wave-uniform, and hipcc is told so)
            if ((int)blockIdx.x < n_streams) f64_ring_helper(streams[blockIdx.x], lds_dyn);
            return;
        }
        msk_frontend_body<1, true>(streams, cfg, n_streams, lds_dyn);
    } else {
        load_atan_table_q<64>(lds_dyn + kTabOff);
        __syncthreads();
        msk_frontend_body<1>(streams, cfg, n_streams, lds_dyn);
    }
}
extern "C" __global__ __launch_bounds__(256) void k_msk_frontend_rb_wg4(OpvStream* __restrict__ streams, OpvGlobalCfg cfg,
                                                                         int n_streams) {
    __shared__ __attribute__((aligned(16))) unsigned char lds_all[4 * kTabOff + kAtanQBytes];
    lbyte* const lds = (lbyte*)lds_all;
    load_atan_table_q<256>(lds + 4 * kTabOff);
    __syncthreads();
    msk_frontend_body<4>(streams, cfg, n_streams, lds);
}
