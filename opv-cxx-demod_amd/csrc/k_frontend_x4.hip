// k_frontend_x4.hip — MSK front-end for MANY streams: FOUR IQ streams per wavefront, one per DPP row
// (16 lanes), four interpolated samples per lane. Same arithmetic contract as k_frontend.hip
// (reference src/opv-demod.cpp:206-329 + the chunker :1012-1113 / :1132-1173); selected by the shim
// when a context carries enough streams to fill the chip without the one-wave-per-stream mapping
// (opv_set_frontend, or by stream count: opv_round_rules.h, frontend_kernel).
//
// Why: a symbol's loop filters, divides and atan2 are scalar work per STREAM. With one stream per
// wave they are executed on 64 lanes for one result (about 65 of that kernel's 161 instructions per
// symbol). Here a wave instruction advances four streams: the scalar tail is shared by four, the
// reductions stay inside a DPP row (4 rotations, no cross-row swaps), and the per-sample work grows only
// from one to four taps per lane. Rows reach their chunk ends, first symbols and refill points at different
// symbols, so the loop carries per-row call state under exec masks; symbols run in BATCHES that provably need none
// of it for any row (round 2: the same statements compiled without the tests), the rings are refilled in 256-sample
// blocks by the whole wave, the row sums run four in lockstep and finish with broadcast FMACs; together they took the
// per-wave-symbol count (rocprofv3 PMC, MI355X, 4096 streams) from 448 VALU + 87 SALU + 12 LDS/VMEM to 319 + 25 + 7 =
// 88 issued instructions per symbol and stream (one wave per stream: 161). Because a wave carries four streams the chip fills four times later, and a launch lasts as long as one wave
// needs for its four streams: 47 ms for 30 frames whether the context has 1025 or 4096 streams (four waves per
// workgroup = one per SIMD of a CU by construction, see msk_frontend_x4_body), 81 ms for 8192 (two waves per SIMD):
// front-end alone 228 GS/s at 4096 streams, 264 at 8192 (round 1: 87 / 130). The one-wave kernel runs 1024 streams at a
// time in 23 ms per 30 frames: faster while two such rounds hold every stream, slower beyond, which is where the shim switches
// (opv_round_rules.h: frontend_kernel; DESIGN.md §3.1, NOTEBOOK.md §3.1).
//
// Mapping (row r = lane / 16 serves stream 4*blockIdx.x + r, t = lane % 16):
//   * lane t owns the interpolated samples Lam_j = L(pos + j - 10), j = t + 16 q, q = 0..3 (j < 60); the
//     three gates are j in [0,40) / [10,50) / [20,60) as in k_frontend.hip, their LO constants T[i] zero
//     outside the window, so a lane accumulates its (up to) four taps per gate in registers;
//   * X[m] = exp(j m d) for m = t - 10 by the same polynomial, X[m+16 q] by three complex multiplies
//     with X[16];
//   * every stream-level quantity lives in VGPRs, replicated over the 16 lanes of its row (k_frontend_rows.h: RowStream);
//   * int16 IQ: a 1024-sample ring per row in LDS (+ 60-sample guard mirroring its head), refilled in
//     256-sample blocks (one direct-to-LDS 16 B/lane load of the WHOLE wave per row and block), requested
//     one refill point (four symbols) before their first use and awaited with one s_waitcnt vmcnt(0) there.
//
// Differences from the reference are of the same kind and size as k_frontend.hip's (shared
// interpolation fraction, factored LO, FMA, table atan2): soft symbols agree to ~1e-14 of their mean,
// every decision downstream is identical (tests/test_gpu_parity.py runs both mappings).
#include <type_traits>

#include "k_frontend_rows.h"

namespace {

constexpr uint32_t kRingSamples = 1024;
constexpr uint32_t kRingBytes = kRingSamples * 4;   // 4096
constexpr uint32_t kGuardBytes = 240;               // mirror of the ring's first 60 samples (a tap reaches 200 B past the ring; 240 keeps
                                                    // two 16-stream workgroups with their 12 KB angle table inside a CU's 160 KB)
constexpr uint32_t kRowBytes = kRingBytes + kGuardBytes;
constexpr uint32_t kBlock = 256;                    // samples per refill block (64 lanes x 16 B: the WHOLE wave loads for one row)
// Refill rule, applied every fourth symbol after the previous blocks have landed (g = floor(pos) of the row, hi = end of
// what its ring holds): a symbol reads samples g - 11 .. g + 55 and g grows by at most 42 per symbol, so the four symbols
// up to the next refill point need hi >= g + 182 NOW (invariant) and the ones after it hi >= g + 350 THEN. A block is
// requested while hi < g + 648: it lands by the next refill point, where hi + 256 >= (g + 168) + 182 again, and it
// overwrites samples below hi - 768 <= g - 120, which nothing reads any more. At most one block per row and refill point.
constexpr uint32_t kAheadMin = 648;
constexpr uint32_t kTabOff = 4 * kRowBytes;         // 17408
// LDS per workgroup: WPB x kTabOff + the atan table (257 x 48 B) = 29 680 B for one wave (five workgroups per CU), 81 712 B for four (two)
static_assert(kTabOff % 16 == 0, "16-byte LDS alignment");

// Four row sums in lockstep (dpp_add4, one rotation step per call). Two rotation steps leave the row's four partial sums in
// its lanes 0..3 (every lane l holds the one of l mod 4); the
// DP-ALU DPP forms finish the job in 16 instructions instead of the 24 of two more rotation steps: v_mov_b64_dpp
// row_newbcast:0 + three v_fmac_f64_dpp row_newbcast:n with a factor of 1.0 per value (k_frontend.hip: symbol_r,
// scripts/microbench/dpp64.hip). The four adds of the step before are the wait states the first DPP reads need.
__device__ inline void row_sum4(double& a, double& b, double& c, double& d, double one) {
    dpp_add4<0x128>(a, b, c, d);
    dpp_add4<0x124>(a, b, c, d);
    double ra, rb, rc, rd;
#define OPV_B4(N) "v_fmac_f64_dpp %0, %4, %8 row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t" \
                  "v_fmac_f64_dpp %1, %5, %8 row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t" \
                  "v_fmac_f64_dpp %2, %6, %8 row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t" \
                  "v_fmac_f64_dpp %3, %7, %8 row_newbcast:" #N " row_mask:0xf bank_mask:0xf\n\t"
    asm("v_mov_b64_dpp %0, %4 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b64_dpp %1, %5 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b64_dpp %2, %6 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
        "v_mov_b64_dpp %3, %7 row_newbcast:0 row_mask:0xf bank_mask:0xf\n\t"
        OPV_B4(1) OPV_B4(2) OPV_B4(3)
        : "=&v"(ra), "=&v"(rb), "=&v"(rc), "=&v"(rd) : "v"(a), "v"(b), "v"(c), "v"(d), "v"(one));
#undef OPV_B4
    a = ra; b = rb; c = rc; d = rd;
}
}  // namespace

// this translation unit's own image of the angle table (opv_atan2.h: kOpvAtanTabQ): every .hip file is compiled to a
// code object of its own (no relocatable device code), so that the front-end files can go through tools/align_vop3.py
__constant__ double kOpvAtanTabQx4[257][6] = {
#include "opv_atan_table_q.inc"
};

// WPB = wavefronts per workgroup (k_frontend.hip, msk_frontend_body: single-wave workgroups are placed without regard
// to SIMDs, four waves of one workgroup always land on the four SIMDs of a CU). Waves share only the atan table.
template <int WPB>
__device__ __forceinline__ void msk_frontend_x4_body(OpvStream* __restrict__ streams, OpvGlobalCfg cfg, int n_streams) {
    const int lane = threadIdx.x & 63, row = lane >> 4, t = lane & 15;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sidx = ((int)blockIdx.x * WPB + wave) * 4 + row;
    const bool have = sidx < n_streams;
    OpvStream& st = streams[have ? sidx : n_streams - 1];   // idle rows read a valid record and never write
    const uint64_t dbg_t0 = __builtin_amdgcn_s_memtime(), dbg_r0 = __builtin_amdgcn_s_memrealtime();

    __shared__ __attribute__((aligned(16))) unsigned char lds_all[WPB * kTabOff + 257 * 48];
    unsigned char* const lds = lds_all + wave * kTabOff;    // this wave's four rings
    double* atab = reinterpret_cast<double*>(lds_all + WPB * kTabOff);
    for (int i = threadIdx.x; i < 257 * 6; i += 64 * WPB) atab[i] = (&kOpvAtanTabQx4[0][0])[i];
    const unsigned char* ring = lds + (uint32_t)row * kRowBytes;
    const uint32_t lds_base = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;
    const uint32_t ring_lds = lds_base + (uint32_t)row * kRowBytes;

    // ---- per-lane constants: T_1[i] = (cos(pi i/80), -sin(pi i/80)) inside each gate's window ----
    double aE[4], bE[4], aO[4], bO[4], aL[4], bL[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int j = t + 16 * q;
        double sn, cs;
        aE[q] = bE[q] = aO[q] = bO[q] = aL[q] = bL[q] = 0.0;
        if (j < 40) { sincospi((double)j / 80.0, &sn, &cs); aE[q] = cs; bE[q] = -sn; }
        if (j >= 10 && j < 50) { sincospi((double)(j - 10) / 80.0, &sn, &cs); aO[q] = cs; bO[q] = -sn; }
        if (j >= 20 && j < 60) { sincospi((double)(j - 20) / 80.0, &sn, &cs); aL[q] = cs; bL[q] = -sn; }
    }
    const double kf0 = (double)(t - 10);
    const double kfs0 = kf0 * kDeltaPerHz;
    const double kgain = st.afc_alpha * (kSymRate / kTwoPi);
    double kc_one = 1.0;                                // the broadcast FMACs' second factor has to be a VGPR
    asm volatile("" : "+v"(kc_one));

    // ---- carry and call state (row-uniform, in VGPRs: k_frontend_rows.h) ------------------------------
    RowStream rs;
    rs.load(st, have);

    // ---- ring refill ------------------------------------------------------------------------------
    // hi: the row's ring holds absolute samples [hi - 1024, hi) (as far as the capture reaches); blocks of 256 samples,
    // 1 KB aligned in the capture, moved by ONE direct-to-LDS load of the whole wave (lane l writes LDS byte m0 + 16 l):
    // all 64 lanes load for one row at a time, from that row's capture (its pointer and cursor broadcast by v_readlane).
    // The ring head is mirrored into the guard by the row's own 16 lanes (64 samples).
    auto glds16 = [&](const gbyte* gsrc, uint32_t m0v) {
        unsigned keep;
        asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                     : "=&s"(keep)
                     : "v"(gsrc), "s"(m0v)
                     : "memory");
    };
    uint32_t hi;
    {
        const uint32_t g0 = rs.origin + (uint32_t)(int)rs.mu;
        hi = (g0 >= 11u ? g0 - 11u : 0u) & ~(kBlock - 1u);
    }
    auto issue_block = [&](uint32_t dst_off) {   // the calling lanes are the 16 lanes of ONE row
        const uint64_t off = (uint64_t)hi * 4u + (uint32_t)t * 16u;
        const uint32_t m0v = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ring_lds + dst_off - 256u * (uint32_t)row));
        if (off + 16u <= rs.n_bytes) glds16(rs.iq_bytes + off, m0v);
        else if (off < rs.n_bytes) {   // the capture's last, incomplete 16 bytes: nothing past n_avail is read
            for (uint32_t j = 0; off + 4u * j < rs.n_bytes; ++j)
                *reinterpret_cast<int*>(lds + (uint32_t)row * kRowBytes + dst_off + (uint32_t)t * 16u + 4u * j) =
                    *reinterpret_cast<const __attribute__((address_space(1))) int*>(rs.iq_bytes + off + 4u * j);
        }
    };
    auto issue_wide = [&](int r, uint32_t hi_r) {   // all 64 lanes; r is a constant after unrolling
        const uint32_t nb_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)rs.n_bytes, 16 * r);
        const uint32_t nb_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(rs.n_bytes >> 32), 16 * r);
        const uint64_t nb = ((uint64_t)nb_hi << 32) | nb_lo;
        const uint64_t pb = (uint64_t)(uintptr_t)rs.iq_bytes;
        const uint32_t p_lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pb, 16 * r);
        const uint32_t p_hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(pb >> 32), 16 * r);
        const gbyte* src = (const gbyte*)(uintptr_t)(((uint64_t)p_hi << 32) | p_lo);
        const uint32_t dst = (hi_r * 4u) & (kRingBytes - 1u);
        const uint64_t off = (uint64_t)hi_r * 4u + (uint32_t)lane * 16u;
        if (off + 16u <= nb) glds16(src + off, lds_base + (uint32_t)r * kRowBytes + dst);
        else if (off < nb) {   // the capture's last, incomplete 16 bytes: nothing past n_avail is read
            for (uint32_t j = 0; off + 4u * j < nb; ++j)
                *reinterpret_cast<int*>(lds + (uint32_t)r * kRowBytes + dst + (uint32_t)lane * 16u + 4u * j) =
                    *reinterpret_cast<const __attribute__((address_space(1))) int*>(src + off + 4u * j);
        }
    };
    auto refill = [&](bool wants, uint32_t g, int max_rounds) {
        for (int rep = 0; rep < max_rounds; ++rep) {
            const bool need = wants && hi < g + kAheadMin && (uint64_t)hi * 4u < rs.n_bytes;
            const uint64_t m = __ballot(need);
            if (m == 0ull) break;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if ((m >> (16 * r)) & 1ull) {      // wave-uniform
                    const uint32_t hi_r = (uint32_t)__builtin_amdgcn_readlane((int)hi, 16 * r);
                    issue_wide(r, hi_r);
                    if (((hi_r * 4u) & (kRingBytes - 1u)) == 0u) {   // ring head: mirror its first 64 samples into the guard
                        if (row == r && t < 15) issue_block(kRingBytes);   // 15 lanes x 16 B = the guard's 240 B
                    }
                }
            }
            if (need) hi += kBlock;
        }
    };
    // One symbol of every row that executes this (exec = the rows inside a demodulate() call whose next symbol exists).
    // Generic / fast: RowStream::finish_symbol. `slot`: which of a row's four soft-log lanes keeps this symbol's value.
    auto symbol_body = [&](auto generic_tag, uint32_t slot) {
        constexpr bool kGeneric = decltype(generic_tag)::value;
        // ---- taps (ref :122-128, :232-238) --------------------------------------------------
        const double pf = rs.pos + kf0;
        const double fl = floor(pf);
        const double f = pf - fl;
        const int i0 = (int)fl;
        const uint32_t byte0 = (((uint32_t)(i0 + (int)rs.origin)) << 2) & (kRingBytes - 1u);
        int w0[4], w1[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int* tap = reinterpret_cast<const int*>(ring + byte0 + 64u * (uint32_t)q);
            w0[q] = tap[0];
            w1[q] = tap[1];
        }
        __builtin_amdgcn_sched_barrier(0);                              // taps requested FIRST, the LO under their latency
        if (kGeneric && rs.first && pf < 0.0) {                           // early gate before the chunk: s[0] (ref :237)
            const int s0 = *reinterpret_cast<const int*>(ring + ((rs.origin << 2) & (kRingBytes - 1u)));
            w0[0] = s0;
            w1[0] = s0;
        }
        // ---- LO: X[m] for m = t - 10 + 16 q ---------------------------------------------------
        double xs[4], xc[4], s16, c16;
        expj_small10(kfs0 * rs.fo, xs[0], xc[0]);
        expj_small10((16.0 * kDeltaPerHz) * rs.fo, s16, c16);
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            xc[q] = fma(xc[q - 1], c16, -(xs[q - 1] * s16));
            xs[q] = fma(xc[q - 1], s16, xs[q - 1] * c16);
        }
        if (kGeneric && fabs(rs.fo) > 2000.0) {
            // -o takes any value (ref :1004-1005) and the AFC clamp (:303) first acts at the END of the
            // call's second symbol: outside the polynomial's range those symbols take the full-range routine
#pragma unroll
            for (int q = 0; q < 4; ++q) sincos((kfs0 + (16.0 * q) * kDeltaPerHz) * rs.fo, &xs[q], &xc[q]);
        }
        // X[40] = exp(j 40 d), needed by the NEXT symbol's phase detector: it is lane 2's fourth tap (m = 2 - 10 + 48),
        // handed to the row by v_mov_b64_dpp row_newbcast:2 (`old` operands: the two dead X[16] registers)
        const double x40c = __builtin_amdgcn_update_dpp(c16, xc[3], 0x152, 0xF, 0xF, false);
        const double x40s = __builtin_amdgcn_update_dpp(s16, xs[3], 0x152, 0xF, 0xF, false);
        // (the LO above does not depend on the taps: it stays between their LDS reads and their first use - left to
        // itself hipcc unpacks the taps first and waits for them)
        asm volatile("" : "+v"(xs[3]), "+v"(xc[3]));
        __builtin_amdgcn_sched_barrier(0);

        double o1 = 0, o2 = 0, o3 = 0, o4 = 0;             // on-time P1..P4 partials
        double eA = 0, eB = 0, eC = 0, eD = 0, lA = 0, lB = 0, lC = 0, lD = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s0r = (int)(short)(w0[q] & 0xFFFF), s0i = w0[q] >> 16;    // ref :1023
            const int d_r = (int)(short)(w1[q] & 0xFFFF) - s0r, d_i = (w1[q] >> 16) - s0i;
            const double lr = fma(f, (double)d_r, (double)s0r);
            const double li = fma(f, (double)d_i, (double)s0i);
            const double zr = fma(lr, xc[q], li * xs[q]);   // Z = Lam conj(X)
            const double zi = fma(li, xc[q], -(lr * xs[q]));
            o1 = fma(zr, aO[q], o1); o2 = fma(zi, bO[q], o2); o3 = fma(zi, aO[q], o3); o4 = fma(zr, bO[q], o4);
            if (q < 3) { eA = fma(zr, aE[q], eA); eB = fma(zi, aE[q], eB); eC = fma(zi, bE[q], eC); eD = fma(zr, bE[q], eD); }
            if (q > 0) { lA = fma(zr, aL[q], lA); lB = fma(zi, aL[q], lB); lC = fma(zi, bL[q], lC); lD = fma(zr, bL[q], lD); }
        }
        // ---- on-time gate: soft value, dominant tone (ref :264-272) --------------------------
        row_sum4(o1, o2, o3, o4, kc_one);
        const RowTone tn = RowStream::tone(o1, o2, o3, o4);
        const double sg = -tn.nsg;
        // ---- early / late gates of the dominant tone (ref :271-280) ---------------------------
        double Ere = fma(sg, eC, eA), Eim = fma(-sg, eD, eB), Lre = fma(sg, lC, lA), Lim = fma(-sg, lD, lB);
        row_sum4(Ere, Eim, Lre, Lim, kc_one);
        rs.finish_symbol<kGeneric>(o1, o2, o3, o4, tn.soft, sg, Ere, Eim, Lre, Lim, x40c, x40s, atab, kgain, (uint32_t)t == slot);
    };
    refill(!rs.done, rs.origin + (uint32_t)(int)rs.mu, 4);
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    __syncthreads();                     // atan table visible (single wave: LDS ordering only)

    for (uint32_t iter = 0;; ++iter) {
        if (!rs.in_call && !rs.done) rs.begin_call(cfg);
        if (__ballot(rs.in_call) == 0ull) break;

        // ---- batches: as many symbols as EVERY row inside a call can take (RowStream::quota), in groups of four (the
        // soft-log lanes and the refill points keep their rhythm); the per-symbol bookkeeping of the loop below - what makes
        // up a third of its instructions - is then paid once per batch.
        if ((iter & 3u) == 0u) {
            const int krow = rs.quota();
            int kmin = __builtin_amdgcn_readlane(krow, 0);
            { const int k1 = __builtin_amdgcn_readlane(krow, 16); kmin = k1 < kmin ? k1 : kmin; }
            { const int k2 = __builtin_amdgcn_readlane(krow, 32); kmin = k2 < kmin ? k2 : kmin; }
            { const int k3 = __builtin_amdgcn_readlane(krow, 48); kmin = k3 < kmin ? k3 : kmin; }
            for (uint32_t quads = (uint32_t)kmin >> 2; quads != 0u; --quads) {
                __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): blocks and stores issued 4 symbols ago
                rs.flush_soft();
                refill(rs.in_call, rs.origin + (uint32_t)(int)rs.pos, 4);
                if (rs.in_call) {
                    symbol_body(std::false_type{}, 0u);
                    symbol_body(std::false_type{}, 1u);
                    symbol_body(std::false_type{}, 2u);
                    symbol_body(std::false_type{}, 3u);
                }
                iter += 4u;
            }
        }

        if ((iter & 3u) == 0u) {
            __builtin_amdgcn_s_waitcnt(0x0F70);                    // vmcnt(0): blocks and stores issued 4 symbols ago
            rs.flush_soft();
            refill(rs.in_call, rs.origin + (uint32_t)(int)rs.pos, 4);
        }

        if (rs.in_call) {
            if (rs.has_symbol()) symbol_body(std::true_type{}, iter & 3u);
            else rs.end_call(t == 0);
        }
    }

    rs.flush_soft();
    if (have && t == 0) rs.store(st, dbg_t0, dbg_r0);
}

// sixteen streams per workgroup: one wave per SIMD of a CU by construction. (A one-wave workgroup shape of this body existed
// until round 6; it was reachable only by forcing this mapping beyond 8192 streams, where the automatic choice is sixteen per wave.)
extern "C" __global__ __launch_bounds__(256) void k_msk_frontend_x4_wg4(OpvStream* __restrict__ streams, OpvGlobalCfg cfg,
                                                                        int n_streams) {
    msk_frontend_x4_body<4>(streams, cfg, n_streams);
}
