// k_frontend_x16.hip — MSK front-end for VERY MANY streams: SIXTEEN IQ streams per wavefront, one per DPP quad
// (4 lanes), fifteen CONSECUTIVE interpolated samples per lane. Same arithmetic contract as k_frontend.hip /
// k_frontend_x4.hip (reference src/opv-demod.cpp:206-329 + the chunker :1012-1113 / :1132-1173); selected with
// opv_set_frontend(ctx, 16), and by opv_process itself from the stream count opv_round_rules.h names (frontend_kernel;
// bench.py's stream_sweep, front-end alone: 4096 x 15 frames 207 GS/s four-per-wave against 129 sixteen-per-wave - 256 waves
// leave three SIMDs in four idle -, 8192 x 7: 221 against 255, 16 384 x 3: 175 against 407; see the rule's comment).
//
// Why: the per-stream arithmetic of a symbol is ~1080 lane-FMAs, everything else - loop filters,
// divides, atan2, chunk bookkeeping - is scalar work per STREAM that a wave executes on all of its lanes. With four
// streams per wave (k_frontend_x4.hip) that tail is 247 of the 319 vector instructions of a wave-symbol, i.e. 88 issued
// instructions per symbol and stream; here it is shared by sixteen streams.
//
// Mapping (quad r = lane / 4 serves stream 16 * (wave index) + r, t = lane % 4):
//   * lane t owns the interpolated samples Lam_j = L(pos + j - 10), j = 15 t + q, q = 0..14: sixteen CONSECUTIVE int16 IQ
//     samples from the quad's ring give its fifteen linear interpolations (the reference's interp(), :122-128, with the shared
//     fraction of k_frontend.hip), so every sample is unpacked and widened once per lane instead of twice per tap;
//   * the LO X[m] = exp(j m d), m = j - 10, from a seed per lane (same polynomial as the other kernels) and fourteen complex
//     multiplies by X[1];
//   * ONE window coefficient set T'[j] = exp(-j pi (j - 10) / 80) for all three gates: the on-time gate (j in [10, 50)) is
//     then exactly the other kernels' convention (its four sums P1..P4 are the carry in OpvStream, shared with every other
//     mapping), the early gate (j in [0, 40)) and the late gate (j in [20, 60)) come out rotated by exp(j pi / 8) and
//     exp(-j pi / 8) - and only their NORMS are used (:271-280). A tap is therefore accumulated ONCE (four FMAs), into one of
//     three per-lane groups (q < 5, q < 10, q < 15); a gate is a 0/1-weighted sum of groups (the five segments [0,10) [10,20)
//     [20,40) [40,50) [50,60) of the sample axis meet lane boundaries at 15, 30, 45), reduced over the quad by two
//     quad_perm steps;
//   * every stream-level quantity lives in VGPRs, replicated over the 4 lanes of its quad (k_frontend_rows.h: RowStream);
//   * int16 IQ: a 256-sample ring per quad in LDS (+ a 16-sample guard mirroring its head). Every second symbol each
//     quad requests the 16-sample blocks (64 B: one 16-byte load per lane, all sixteen quads in ONE instruction) that the two
//     symbols AFTER the next refill point will need, holds them in registers, and writes them into its ring at that next
//     point: two symbols of latency budget, no scalar bookkeeping per block, the HBM stream of a quad stays sequential.
//
// Differences from the reference: as k_frontend_x4.hip states, and here one rotation-free re-association of the early /
// late sums.
#include <type_traits>

#include "k_frontend_rows.h"

namespace {

constexpr uint32_t kRingSamples = 256;
constexpr uint32_t kRingBytes = kRingSamples * 4;   // 1024
constexpr uint32_t kGuardBytes = 64;                // mirror of the ring's first 16 samples (a lane reads 16 consecutive samples)
constexpr uint32_t kRowBytes = kRingBytes + kGuardBytes;   // 1088
constexpr uint32_t kBlk = 16;                       // samples per block: 4 lanes x 16 B
constexpr int kBlocksPerPoint = 6;                  // blocks a quad may request per refill point (two symbols consume <= 84 samples)
// Refill rule (g = floor(pos) of the quad at a refill point, hi = end of what its ring holds or has requested): a symbol reads
// samples g - 11 .. g + 55 and g grows by 38..42 per symbol. Blocks requested at point k are written at point k + 1 (two symbols
// later, g' <= g + 84) and have to carry the two symbols after THAT: up to g' + 42 + 55 <= g + 181. So a quad requests blocks
// while hi < g + 182 (at most 6: it held hi >= g_prev + 182 >= g + 98 already). A written block [h, h + 16) with h < g + 198
// takes the ring slot of [h - 256, h - 240), below g - 42 <= g' - 11 - 31: nothing reads that any more.
constexpr uint32_t kAhead = 182;
constexpr uint32_t kTabOff = 16 * kRowBytes;        // 17408 B of rings per wave
static_assert(kTabOff % 16 == 0, "16-byte LDS alignment");

typedef int v4i __attribute__((ext_vector_type(4)));

// four quad sums in lockstep (quad_perm [1,0,3,2] then [2,3,0,1]): a DPP read needs two wait states behind the VALU write of
// its source - the other three sums' instructions fill the slots (k_frontend_common.h: dpp_add4)
__device__ inline void quad_sum4(double& a, double& b, double& c, double& d) {
    dpp_add4<0xB1>(a, b, c, d);
    dpp_add4<0x4E>(a, b, c, d);
}
__device__ inline double quad_bcast3(double v) {        // lane 3 of the quad -> every lane of it (quad_perm [3,3,3,3])
    return mkd(__builtin_amdgcn_mov_dpp(dhi(v), 0xFF, 0xF, 0xF, true), __builtin_amdgcn_mov_dpp(dlo(v), 0xFF, 0xF, 0xF, true));
}

}  // namespace

// this translation unit's own image of the angle table (opv_atan2.h: kOpvAtanTabQ; see k_frontend_x4.hip)
__constant__ double kOpvAtanTabQx16[257][6] = {
#include "opv_atan_table_q.inc"
};

// WPB = wavefronts per workgroup (four waves of one workgroup always land on the four SIMDs of a CU). Waves share only the
// atan table.
template <int WPB>
__device__ __forceinline__ void msk_frontend_x16_body(OpvStream* __restrict__ streams, OpvGlobalCfg cfg, int n_streams) {
    const int lane = threadIdx.x & 63, row = lane >> 2, t = lane & 3;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int sidx = ((int)blockIdx.x * WPB + wave) * 16 + row;
    const bool have = sidx < n_streams;
    OpvStream& st = streams[have ? sidx : n_streams - 1];   // idle quads read a valid record and never write
    const uint64_t dbg_t0 = __builtin_amdgcn_s_memtime(), dbg_r0 = __builtin_amdgcn_s_memrealtime();

    __shared__ __attribute__((aligned(16))) unsigned char lds_all[WPB * kTabOff + 257 * 48];
    unsigned char* const lds = lds_all + wave * kTabOff;    // this wave's sixteen rings
    double* atab = reinterpret_cast<double*>(lds_all + WPB * kTabOff);
    for (int i = threadIdx.x; i < 257 * 6; i += 64 * WPB) atab[i] = (&kOpvAtanTabQx16[0][0])[i];
    unsigned char* const ring = lds + (uint32_t)row * kRowBytes;

    // ---- per-lane constants: T'[j] = (cos, -sin)(pi (j - 10) / 80), j = 15 t + q --------------------------------
    double Tc[15], Ts[15];
#pragma unroll
    for (int q = 0; q < 15; ++q) {
        double sn, cs;
        sincospi((double)(15 * t + q - 10) / 80.0, &sn, &cs);
        Tc[q] = cs; Ts[q] = -sn;
    }
    // which of the lane's three tap groups (q < 5, < 10, < 15) lie inside each gate: E = j in [0,40), O = [10,50), L = [20,60)
    //   lane 0: j 0..14    lane 1: j 15..29    lane 2: j 30..44    lane 3: j 45..59
    const double wE0 = t <= 2 ? 1.0 : 0.0, wE1 = t <= 2 ? 1.0 : 0.0, wE2 = t <= 1 ? 1.0 : 0.0;
    const double wO0 = t >= 1 ? 1.0 : 0.0, wO1 = (t == 1 || t == 2) ? 1.0 : 0.0, wO2 = t <= 2 ? 1.0 : 0.0;
    const double wL0 = t >= 2 ? 1.0 : 0.0, wL1 = t >= 1 ? 1.0 : 0.0, wL2 = t >= 1 ? 1.0 : 0.0;
    const double kf0 = (double)(15 * t - 10);
    const double kfs0 = kf0 * kDeltaPerHz;
    const double kgain = st.afc_alpha * (kSymRate / kTwoPi);
    // ---- carry and call state (row-uniform, in VGPRs: k_frontend_rows.h) ------------------------------
    RowStream rs;
    rs.load(st, have);

    // ---- ring refill (see the rule at kAhead) --------------------------------------------------------------------
    // hi: the quad's ring holds (or has in flight) absolute samples [.., hi); blocks of 16 samples, 64 B aligned in the capture.
    uint32_t hi;
    {
        const uint32_t g0 = rs.origin + (uint32_t)(int)rs.mu;
        hi = (g0 >= 11u ? g0 - 11u : 0u) & ~(kBlk - 1u);
    }
    v4i blkv[kBlocksPerPoint];
    uint32_t blk_hi0 = 0, blk_n = 0;                      // the blocks in registers: samples [blk_hi0, blk_hi0 + 16 blk_n)
    auto load_block = [&](uint32_t h) -> v4i {           // this lane's 16 bytes of block [h, h + 16)
        const uint64_t off = (uint64_t)h * 4u + (uint32_t)t * 16u;
        v4i v = {0, 0, 0, 0};
        if (off + 16u <= rs.n_bytes) v = *reinterpret_cast<const __attribute__((address_space(1))) v4i*>(rs.iq_bytes + off);
        else if (off < rs.n_bytes) {                         // the capture's last, incomplete 16 bytes: nothing past n_avail is read
            int e[4] = {0, 0, 0, 0};
            for (uint32_t j = 0; j < 4u && off + 4u * j < rs.n_bytes; ++j)
                e[j] = *reinterpret_cast<const __attribute__((address_space(1))) int*>(rs.iq_bytes + off + 4u * j);
            v = v4i{e[0], e[1], e[2], e[3]};
        }
        return v;
    };
    auto store_block = [&](uint32_t h, v4i v) {
        const uint32_t o = ((h * 4u) & (kRingBytes - 1u)) + (uint32_t)t * 16u;
        *reinterpret_cast<v4i*>(ring + o) = v;
        if (o < kGuardBytes) *reinterpret_cast<v4i*>(ring + kRingBytes + o) = v;   // the ring's head is mirrored behind its end
    };
    auto write_held = [&]() {                             // the blocks requested at the previous refill point have landed
#pragma unroll
        for (int k = 0; k < kBlocksPerPoint; ++k)
            if ((uint32_t)k < blk_n) store_block(blk_hi0 + kBlk * (uint32_t)k, blkv[k]);
        blk_n = 0;
    };
    auto request = [&](bool wants, uint32_t g) {          // at most kBlocksPerPoint blocks towards hi >= g + kAhead
        blk_hi0 = hi;
        uint32_t n = 0;
        if (wants && hi < g + kAhead && (uint64_t)hi * 4u < rs.n_bytes) {
            n = (g + kAhead - hi + kBlk - 1u) / kBlk;
            if (n > (uint32_t)kBlocksPerPoint) n = (uint32_t)kBlocksPerPoint;
        }
#pragma unroll
        for (int k = 0; k < kBlocksPerPoint; ++k)
            if ((uint32_t)k < n) blkv[k] = load_block(hi + kBlk * (uint32_t)k);
        blk_n = n;
        hi += kBlk * n;
    };
    // One symbol of every quad that executes this (exec = the quads inside a demodulate() call whose next symbol exists).
    // Generic / fast: RowStream::finish_symbol. `slot`: which of a quad's four lanes keeps this symbol's soft value.
    auto symbol_body = [&](auto generic_tag, uint32_t slot) {
        constexpr bool kGeneric = decltype(generic_tag)::value;
        // ---- taps (ref :122-128, :232-238): sixteen consecutive samples -> fifteen interpolations ---------------
        const double pf = rs.pos + kf0;
        const double fl = floor(pf);
        const double f = pf - fl;
        const int i0 = (int)fl;
        const uint32_t byte0 = (((uint32_t)(i0 + (int)rs.origin)) << 2) & (kRingBytes - 1u);
        int w[16];
        {
            const int* tap = reinterpret_cast<const int*>(ring + byte0);
#pragma unroll
            for (int q = 0; q < 16; ++q) w[q] = tap[q];
        }
        __builtin_amdgcn_sched_barrier(0);                              // taps requested FIRST, the LO seed under their latency
        // ---- LO: X[m] for m = 15 t - 10 + q: seed and step ---------------------------------------------------------
        double xs, xc, s1, c1;
        expj_small10(kfs0 * rs.fo, xs, xc);
        expj_small10(kDeltaPerHz * rs.fo, s1, c1);
        if (kGeneric && fabs(rs.fo) > 2000.0) {
            // -o takes any value (ref :1004-1005) and the AFC clamp (:303) first acts at the END of the
            // call's second symbol: outside the polynomial's range those symbols take the full-range routine
            sincos(kfs0 * rs.fo, &xs, &xc);
            sincos(kDeltaPerHz * rs.fo, &s1, &c1);
        }
        __builtin_amdgcn_sched_barrier(0);
        const int s0_first = (kGeneric && rs.first) ? *reinterpret_cast<const int*>(ring + ((rs.origin << 2) & (kRingBytes - 1u))) : 0;

        double g0A = 0, g0B = 0, g0C = 0, g0D = 0, g1A = 0, g1B = 0, g1C = 0, g1D = 0, g2A = 0, g2B = 0, g2C = 0, g2D = 0;
        double x40c_l = 0.0, x40s_l = 0.0;
        double pr = (double)(int)(short)(w[0] & 0xFFFF), pi_ = (double)(w[0] >> 16);   // ref :1023
        asm("" : "+v"(pr), "+v"(pi_));
#pragma unroll
        for (int q = 0; q < 15; ++q) {
            double nr = (double)(int)(short)(w[q + 1] & 0xFFFF), ni = (double)(w[q + 1] >> 16);
            asm("" : "+v"(nr), "+v"(ni));                          // (opaque: hipcc otherwise subtracts the int16 values and widens the difference too - 60 conversions instead of 32)
            double lr = fma(f, nr - pr, pr);                       // (differences of int16 values are exact in fp64)
            double li = fma(f, ni - pi_, pi_);
            if (kGeneric && rs.first && pf + (double)q < 0.0) {        // early gate before the chunk: s[0] (ref :237)
                lr = (double)(int)(short)(s0_first & 0xFFFF);
                li = (double)(s0_first >> 16);
            }
            pr = nr; pi_ = ni;
            if (q == 5) { x40c_l = xc; x40s_l = xs; }               // X[40] is lane 3's sixth tap (m = 45 - 10 + 5)
            const double zr = fma(lr, xc, li * xs);                 // Z = Lam conj(X)
            const double zi = fma(li, xc, -(lr * xs));
            if (q < 5) { g0A = fma(zr, Tc[q], g0A); g0B = fma(zi, Ts[q], g0B); g0C = fma(zi, Tc[q], g0C); g0D = fma(zr, Ts[q], g0D); }
            else if (q < 10) { g1A = fma(zr, Tc[q], g1A); g1B = fma(zi, Ts[q], g1B); g1C = fma(zi, Tc[q], g1C); g1D = fma(zr, Ts[q], g1D); }
            else { g2A = fma(zr, Tc[q], g2A); g2B = fma(zi, Ts[q], g2B); g2C = fma(zi, Tc[q], g2C); g2D = fma(zr, Ts[q], g2D); }
            if (q < 14) {                                           // X[m + 1] = X[m] X[1]
                const double nc = fma(xc, c1, -(xs * s1));
                xs = fma(xc, s1, xs * c1);
                xc = nc;
            }
        }
        // X[40] = exp(j 40 d), needed by the NEXT symbol's phase detector
        const double x40c = quad_bcast3(x40c_l), x40s = quad_bcast3(x40s_l);
        // ---- on-time gate: soft value, dominant tone (ref :264-272) --------------------------
        double o1 = fma(wO2, g2A, fma(wO1, g1A, wO0 * g0A)), o2 = fma(wO2, g2B, fma(wO1, g1B, wO0 * g0B));
        double o3 = fma(wO2, g2C, fma(wO1, g1C, wO0 * g0C)), o4 = fma(wO2, g2D, fma(wO1, g1D, wO0 * g0D));
        quad_sum4(o1, o2, o3, o4);
        const RowTone tn = RowStream::tone(o1, o2, o3, o4);
        const double sg = -tn.nsg;
        // ---- early / late gates of the dominant tone (ref :271-280): rotated by a constant, only their norms are used ----
        const double r0 = fma(sg, g0B, g0A), i0_ = fma(-sg, g0D, g0C);
        const double r1 = fma(sg, g1B, g1A), i1_ = fma(-sg, g1D, g1C);
        const double r2 = fma(sg, g2B, g2A), i2_ = fma(-sg, g2D, g2C);
        double Ere = fma(wE2, r2, fma(wE1, r1, wE0 * r0)), Eim = fma(wE2, i2_, fma(wE1, i1_, wE0 * i0_));
        double Lre = fma(wL2, r2, fma(wL1, r1, wL0 * r0)), Lim = fma(wL2, i2_, fma(wL1, i1_, wL0 * i0_));
        quad_sum4(Ere, Eim, Lre, Lim);
        rs.finish_symbol<kGeneric>(o1, o2, o3, o4, tn.soft, sg, Ere, Eim, Lre, Lim, x40c, x40s, atab, kgain, (uint32_t)t == slot);
    };
    // ---- initial fill: everything the first two symbols can read, synchronously ---------------------------------
    {
        const uint32_t g = rs.origin + (uint32_t)(int)rs.mu;
        for (int rep = 0; rep < 3; ++rep) {                // (198 samples = 13 blocks at most)
            request(!rs.done, g);
            __builtin_amdgcn_s_waitcnt(0x0F70);            // vmcnt(0)
            write_held();
        }
    }
    __syncthreads();                     // atan table visible (single wave: LDS ordering only)

    // a refill point: the blocks requested two symbols ago go into the ring, the next ones are requested, the held soft
    // symbols leave (every second point: four symbols)
    auto refill_point = [&](bool flush) {
        __builtin_amdgcn_s_waitcnt(0x0F70);                // vmcnt(0): blocks and stores issued two symbols ago
        write_held();
        if (flush) rs.flush_soft();
        request(rs.in_call, rs.origin + (uint32_t)(int)rs.pos);
    };

    for (uint32_t iter = 0;; ++iter) {
        if (!rs.in_call && !rs.done) rs.begin_call(cfg);
        if (__ballot(rs.in_call) == 0ull) break;

        // ---- batches: as many symbols as EVERY quad inside a call can take (RowStream::quota), in groups of four (the
        // soft-log lanes and the refill points keep their rhythm)
        if ((iter & 3u) == 0u) {
            int krow = rs.quota();
#pragma unroll
            for (int off = 32; off >= 4; off >>= 1) { const int o = __shfl_xor(krow, off, 64); krow = o < krow ? o : krow; }
            const int kmin = __builtin_amdgcn_readfirstlane(krow);
            for (uint32_t quads = (uint32_t)kmin >> 2; quads != 0u; --quads) {
                refill_point(true);
                if (rs.in_call) { symbol_body(std::false_type{}, 0u); symbol_body(std::false_type{}, 1u); }
                refill_point(false);
                if (rs.in_call) { symbol_body(std::false_type{}, 2u); symbol_body(std::false_type{}, 3u); }
                iter += 4u;
            }
        }

        if ((iter & 1u) == 0u) refill_point((iter & 3u) == 0u);

        if (rs.in_call) {
            if (rs.has_symbol()) symbol_body(std::true_type{}, iter & 3u);
            else rs.end_call(t == 0);
        }
    }

    rs.flush_soft();
    if (have && t == 0) rs.store(st, dbg_t0, dbg_r0);
}

extern "C" __global__ __launch_bounds__(64) void k_msk_frontend_x16(OpvStream* __restrict__ streams, OpvGlobalCfg cfg,
                                                                     int n_streams) {
    msk_frontend_x16_body<1>(streams, cfg, n_streams);
}
// sixty-four streams per workgroup: one wave per SIMD of a CU by construction
extern "C" __global__ __launch_bounds__(256) void k_msk_frontend_x16_wg4(OpvStream* __restrict__ streams, OpvGlobalCfg cfg,
                                                                         int n_streams) {
    msk_frontend_x16_body<4>(streams, cfg, n_streams);
}
// 128 streams per workgroup: two waves per SIMD of a CU (8 x 17 KB of rings + one 12 KB angle table = 148 KB: one workgroup
// per CU; two of the four-wave kind miss the CU's 160 KB by 96 bytes)
extern "C" __global__ __launch_bounds__(512) void k_msk_frontend_x16_wg8(OpvStream* __restrict__ streams, OpvGlobalCfg cfg,
                                                                         int n_streams) {
    msk_frontend_x16_body<8>(streams, cfg, n_streams);
}
