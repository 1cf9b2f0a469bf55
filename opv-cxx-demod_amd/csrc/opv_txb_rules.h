// opv_txb_rules.h — the rules of a transmit bank's round, once each, in plain C++ (no HIP header: with opv_txb_rules.cpp it
// compiles with the host compiler like opv_stream_rules.cpp, and runs under sanitizers without a GPU): what a round refuses,
// the geometry of its launches, and the host's evaluation of one ambiguous sample.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/opv_demod.h"
#include "opv_frame_code.h"

constexpr uint32_t kTxbBlockSyms = 64;                                                        // symbols per workgroup of k_txb_modulate
constexpr uint32_t kTxbFrameBlocks = (OPV_FRAME_SYMBOLS + kTxbBlockSyms - 1) / kTxbBlockSyms; // 34: 33 full + one of 56 symbols
constexpr uint64_t kTxbFrameSamples = (uint64_t)OPV_FRAME_SYMBOLS * OPV_SAMPLES_PER_SYMBOL;   // 86720
constexpr uint64_t kTxbMaxRunSymbols = (uint64_t)OPV_TXB_MAX_RUN_FRAMES * OPV_FRAME_SYMBOLS;
constexpr uint64_t kTxbMaxRoundFrames = 0x7FFFFFFFull / kTxbFrameBlocks;                      // the modulate grid stays below 2^31

// nullptr if `s` is a state a modulator can be in, else why not (every refusal is OPV_EINVAL)
const char* txb_state_refusal(const opv_txb_state& s);

// opv_txb_plan_round (include/opv_demod.h) without the error text's destination: OPV_OK, or the refusal's code with *why set
int txb_plan_round(int n_streams, const opv_txb_state* states, int count, const int* streams, const size_t* n_frames,
                   const uintptr_t* out_addr, uint32_t* first_block, uint64_t* first_symbol, const char** why);

// opv_tap_txb_patch: the NCOs at `symbol` from checkpoint symbol / 128, replayed; then the sample as the reference computes it
void txb_patch_sample(uint64_t symbol, int sample, int code, int16_t out_iq[2]);

// One entry of the device's list of ambiguous samples (k_tx_bank.hip), self-contained: the host re-evaluates it without the
// frames (opv_tap_txb_patch's arguments + where the sample lives)
struct OpvTxbAmb {
    uint64_t addr;      // device address of the sample's int16 pair
    uint64_t symbol;    // index of its symbol in its stream's run
    int32_t sample;     // 0..39 within the symbol
    int32_t code;       // +/-1 tone 1 with that sign, +/-2 tone 2
};

// One entry of a round as the kernels see it (entries of 0 frames are left out). The round's frames are numbered entry after
// entry: frame first_frame + k of the round's scratch (code bytes, parities, symbol-start phases) is the entry's frame k.
struct OpvTxbEntry {
    const uint8_t* frames;   // device-visible: n_frames x 134 bytes
    int* out;                // device: n_frames x 86720 packed samples
    uint64_t first_symbol;   // of the entry, as an index into its stream's run
    uint32_t n_frames;
    uint32_t first_frame;    // among the round's frames
    uint32_t first_block;    // workgroup of k_txb_modulate (txb_plan_round)
    uint32_t first_ivl;      // thread of k_txb_phases: one per 128-symbol checkpoint interval the entry touches
    uint32_t stream;         // slot of the bank: where the carried sign parity lives
    uint32_t pad;
};
// checkpoint intervals that n_symbols symbols from first_symbol on touch (n_symbols > 0)
inline uint64_t txb_intervals(uint64_t first_symbol, uint64_t n_symbols, uint32_t ckpt_syms) {
    return (first_symbol + n_symbols - 1) / ckpt_syms - first_symbol / ckpt_syms + 1;
}
