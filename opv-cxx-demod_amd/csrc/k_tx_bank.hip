// k_tx_bank.hip — one round of a transmit bank (include/opv_demod.h, opv_txb_*): many independent modulators, a few frames
// each, ONE set of launches for all of them. The frame code and the sample synthesis are k_tx_modulate.hip's (k_tx_common.h);
// what is new is that a workgroup finds out whose work it does. A round is a table of entries (OpvTxbEntry: stream, frames,
// output, the entry's first symbol AS AN INDEX INTO ITS STREAM'S RUN), and each kernel's grid is the entries' shares back to back:
//
//   k_txb_encode    one workgroup per frame of the round -> code bytes + the frame's parity (tx_encode_frame)
//   k_txb_scan      one wave per entry: exclusive parity scan over the entry's frames, seeded with the stream's carried sign
//                   parity; leaves the new parity in the bank's device state, where the next round's scan reads it
//   k_txb_phases    one thread per (entry, 128-symbol checkpoint interval it touches): the NCOs are a function of the symbol's
//                   index in the run alone, so a stream far into its run starts from checkpoint index / 128 and replays at most
//                   128 x 40 additions per symbol it needs - the same IEEE adds and wraps as k_tx_expand_phases. A frame is
//                   16 x 128 + 120 symbols, so entries start and end mid-interval. The phases live in the ROUND's scratch
//                   (16 B per symbol of the round), never in a table of the run.
//   k_txb_modulate  64 symbols per workgroup through LDS to 16-byte-per-lane stores (tx_symbol_samples); an entry's last
//                   workgroup is partial (2168 = 33 x 64 + 56) and frame boundaries fall inside workgroups. Flat tops are decided
//                   by the symbol's index in the run, like every run's (k_tx_modulate.hip's file comment).
//
// Ambiguous samples go into one list of self-contained entries (OpvTxbAmb) that the host re-evaluates without the frames.
// Roofline: HBM write, 4 B/sample; per symbol of the round 1 + 16 B of scratch written and read back.
#include "k_tx_common.h"
#include "opv_txb_rules.h"

namespace {
// the entry that owns item `key` of a grid laid out entry after entry: the last one whose first item is <= key (m >= 1)
__device__ inline uint32_t txb_owner(const OpvTxbEntry* __restrict__ ents, uint32_t m, uint32_t key, uint32_t OpvTxbEntry::*first) {
    uint32_t lo = 0, hi = m;                        // ents[lo].*first <= key < ents[hi].*first (hi = m: past the end)
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ents[mid].*first <= key) lo = mid; else hi = mid;
    }
    return lo;
}
}  // namespace

// codes: [round frames * 2168], frame_par: [round frames] (as k_tx_encode's, over the round's frames)
extern "C" __global__ __launch_bounds__(256) void k_txb_encode(const OpvTxbEntry* __restrict__ ents, uint32_t m, uint32_t n_frames,
                                                                uint8_t* __restrict__ codes, uint8_t* __restrict__ frame_par) {
    const uint32_t f = blockIdx.x;
    if (f >= n_frames) return;
    const OpvTxbEntry& e = ents[txb_owner(ents, m, f, &OpvTxbEntry::first_frame)];
    tx_encode_frame(e.frames + (size_t)(f - e.first_frame) * OPV_FB, codes + (size_t)f * OPV_FSYMS, frame_par + f);
}

// in place, per entry: frame_par[f] <- parity of the stream's bits in front of frame f (carried parity + the entry's frames
// before f); parity[stream] <- the parity behind the entry's last frame. Four entries (waves) per workgroup.
extern "C" __global__ __launch_bounds__(256) void k_txb_scan(const OpvTxbEntry* __restrict__ ents, uint32_t m,
                                                              uint8_t* __restrict__ frame_par, uint8_t* __restrict__ parity) {
    const uint32_t i = blockIdx.x * 4u + threadIdx.x / 64u, lane = threadIdx.x & 63u;
    if (i >= m) return;                             // (whole waves)
    const OpvTxbEntry e = ents[i];
    uint32_t carry = parity[e.stream] & 1u;
    for (uint32_t base = 0; base < e.n_frames; base += 64u) {
        const uint32_t k = base + lane;
        const uint32_t own = k < e.n_frames ? (frame_par[e.first_frame + k] & 1u) : 0u;
        const uint64_t ones = __ballot(own != 0u);
        if (k < e.n_frames) frame_par[e.first_frame + k] = (uint8_t)((carry ^ (uint32_t)__popcll(ones & ((1ull << lane) - 1ull))) & 1u);
        carry ^= (uint32_t)__popcll(ones) & 1u;
    }
    if (lane == 0) parity[e.stream] = (uint8_t)carry;
}

// ckpt: (ph1, ph2) at symbol j * OPV_TX_CKPT_SYMS of a run; phases: [round symbols] (ph1, ph2) at every symbol start
extern "C" __global__ __launch_bounds__(64) void k_txb_phases(const OpvTxbEntry* __restrict__ ents, uint32_t m, uint32_t n_ivl,
                                                               const double2* __restrict__ ckpt, double2* __restrict__ phases) {
    const uint32_t t = blockIdx.x * 64u + threadIdx.x;
    if (t >= n_ivl) return;
    const OpvTxbEntry e = ents[txb_owner(ents, m, t, &OpvTxbEntry::first_ivl)];
    const uint64_t s_lo = e.first_symbol, s_hi = s_lo + (uint64_t)e.n_frames * OPV_FSYMS;
    const uint64_t j = s_lo / OPV_TX_CKPT_SYMS + (t - e.first_ivl);
    double2 p = ckpt[j];
    double2* out = phases + (size_t)e.first_frame * OPV_FSYMS;
    uint64_t s = j * OPV_TX_CKPT_SYMS;
    for (uint32_t k = 0; k < OPV_TX_CKPT_SYMS && s < s_hi; ++k, ++s) {
        if (s >= s_lo) out[s - s_lo] = p;
        for (int i = 0; i < OPV_SPS; ++i) { advance_tone1(p.x); advance_tone2(p.y); }   // (a checkpoint is a wrapped phase)
    }
}

// codes / frame_pre / phases: the round's scratch as the three kernels above left it; amb_*: the round's list
extern "C" __global__ __launch_bounds__(64) void k_txb_modulate(const OpvTxbEntry* __restrict__ ents, uint32_t m,
                                                                 const uint8_t* __restrict__ codes, const uint8_t* __restrict__ frame_pre,
                                                                 const double2* __restrict__ phases, uint32_t* __restrict__ amb_count,
                                                                 OpvTxbAmb* __restrict__ amb_list, uint32_t amb_cap, uint64_t flat_lo,
                                                                 uint64_t flat_hi, const uint8_t* __restrict__ flat_bits) {
    __shared__ __attribute__((aligned(16))) int stage[kTxbBlockSyms * OPV_SPS];
    const OpvTxbEntry e = ents[txb_owner(ents, m, blockIdx.x, &OpvTxbEntry::first_block)];
    const uint32_t nsym = e.n_frames * (uint32_t)OPV_FSYMS;                 // (a run is at most 65536 frames: 1.4e8 symbols)
    const uint32_t ls0 = (blockIdx.x - e.first_block) * kTxbBlockSyms, ls = ls0 + threadIdx.x;   // the entry's symbols
    const uint64_t sym = e.first_symbol + ls;                               // the run's
    int a = 0;                                      // +/-1: tone 1 with that sign, +/-2: tone 2, 0: silent
    double ph1 = 0.0, ph2 = 0.0;
    if (ls < nsym && sym != 0) {                    // (symbol 0 of a run: T = 0 right after the modulator's reset, :221-226 - silent)
        const size_t r = (size_t)e.first_frame * OPV_FSYMS + ls;
        a = tx_symbol_code(codes[r], frame_pre[e.first_frame + ls / OPV_FSYMS], sym);
        const double2 p = phases[r];
        ph1 = p.x; ph2 = p.y;
    }
    tx_symbol_samples(a, ph1, ph2, sym, flat_lo, flat_hi, flat_bits, stage + threadIdx.x * OPV_SPS, [&](int i) {
        const uint32_t k = atomicAdd(amb_count, 1u);
        if (k < amb_cap) amb_list[k] = OpvTxbAmb{(uint64_t)(uintptr_t)(e.out + (size_t)ls * OPV_SPS + i), sym, i, a};
    });
    __syncthreads();
    // 64 symbols x 40 samples = 2560 dwords = 10 x (64 lanes x 16 B); the entry's last workgroup stops at its last sample
    const uint64_t base = (uint64_t)ls0 * OPV_SPS, total = (uint64_t)nsym * OPV_SPS;
    const int4* s4 = reinterpret_cast<const int4*>(stage);
    int4* o4 = reinterpret_cast<int4*>(e.out + base);
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const int q = r * 64 + threadIdx.x;
        if (base + 4u * q + 3u < total) o4[q] = s4[q];
    }
}
