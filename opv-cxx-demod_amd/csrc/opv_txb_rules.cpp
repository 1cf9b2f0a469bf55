// opv_txb_rules.cpp — see opv_txb_rules.h. Plain C++: no HIP, no device.
#include "opv_txb_rules.h"

#include <algorithm>
#include <utility>
#include <vector>

#include "opv_tx_internal.h"

const char* txb_state_refusal(const opv_txb_state& s) {
    if (s.sign_parity != 0 && s.sign_parity != 1) return "opv_txb: sign_parity outside {0, 1}";
    if (s.reserved != 0) return "opv_txb: reserved must be 0";
    if (s.symbols > kTxbMaxRunSymbols) return "opv_txb: symbols beyond OPV_TXB_MAX_RUN_FRAMES frames";
    return nullptr;
}

int txb_plan_round(int n_streams, const opv_txb_state* states, int count, const int* streams, const size_t* n_frames,
                   const uintptr_t* out_addr, uint32_t* first_block, uint64_t* first_symbol, const char** why) {
    auto refuse = [&](int code, const char* text) { *why = text; return code; };
    if (!states || !first_block || !first_symbol) return refuse(OPV_EINVAL, "opv_txb_round: null pointer");
    if (n_streams < 1 || n_streams > OPV_TXB_MAX_STREAMS) return refuse(OPV_EINVAL, "opv_txb_round: n_streams outside 1..OPV_TXB_MAX_STREAMS");
    if (count < 0) return refuse(OPV_EINVAL, "opv_txb_round: count < 0");
    if (count > 0 && (!streams || !n_frames || !out_addr)) return refuse(OPV_EINVAL, "opv_txb_round: null pointer");
    // ---- what is wrong with the call (OPV_EINVAL), over all entries, before what is wrong with a run's length
    std::vector<char> seen((size_t)n_streams, 0);
    std::vector<std::pair<uintptr_t, uintptr_t>> spans;                    // [first byte, one past the last) of every non-empty output
    uint64_t round_frames = 0;
    for (int i = 0; i < count; ++i) {
        const int s = streams[i];
        if (s < 0 || s >= n_streams) return refuse(OPV_EINVAL, "opv_txb_round: stream index out of range");
        if (seen[s]) return refuse(OPV_EINVAL, "opv_txb_round: a stream is named twice");
        seen[s] = 1;
        if (const char* bad = txb_state_refusal(states[s])) return refuse(OPV_EINVAL, bad);
        if (n_frames[i] == 0) continue;                                    // (changes nothing: its output is not looked at)
        if (out_addr[i] == 0) return refuse(OPV_EINVAL, "opv_txb_round: null output pointer");
        if (out_addr[i] & 15u) return refuse(OPV_EINVAL, "opv_txb_round: device IQ pointer must be 16-byte aligned");
        if (n_frames[i] > kTxbMaxRoundFrames || (round_frames += n_frames[i]) > kTxbMaxRoundFrames)
            return refuse(OPV_EINVAL, "opv_txb_round: too many frames for one round");
        const uint64_t bytes = (uint64_t)n_frames[i] * kTxbFrameSamples * 4u;
        if (bytes > UINTPTR_MAX - out_addr[i]) return refuse(OPV_EINVAL, "opv_txb_round: output wraps the address space");
        spans.emplace_back(out_addr[i], out_addr[i] + (uintptr_t)bytes);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t k = 1; k < spans.size(); ++k)
        if (spans[k].first < spans[k - 1].second) return refuse(OPV_EINVAL, "opv_txb_round: outputs of two entries overlap");
    for (int i = 0; i < count; ++i) {
        const opv_txb_state& st = states[streams[i]];
        if ((uint64_t)n_frames[i] * OPV_FRAME_SYMBOLS > kTxbMaxRunSymbols - st.symbols)     // (both sides checked above: no wrap)
            return refuse(OPV_ECAPACITY, "opv_txb_round: a stream's run would pass OPV_TXB_MAX_RUN_FRAMES (reset it)");
    }
    // ---- the geometry: 34 workgroups of 64 symbols per frame and entry, entries back to back in the grid
    uint32_t block = 0;
    for (int i = 0; i < count; ++i) {
        first_block[i] = block;
        first_symbol[i] = states[streams[i]].symbols;
        const uint64_t syms = (uint64_t)n_frames[i] * OPV_FRAME_SYMBOLS;
        block += (uint32_t)((syms + kTxbBlockSyms - 1) / kTxbBlockSyms);
    }
    first_block[count] = block;
    return OPV_OK;
}

void txb_patch_sample(uint64_t symbol, int sample, int code, int16_t out_iq[2]) {
    const size_t ck = (size_t)(symbol / OPV_TX_CKPT_SYMS), in = (size_t)(symbol % OPV_TX_CKPT_SYMS);
    double p[2];
    opv_tx_checkpoint_range(ck, 1, p);
    std::vector<double> ph(2 * (in + 1));
    opv_tx_symbol_phases(0, in + 1, &p[0], &p[1], ph.data());
    opv_tx_sample_exact(ph[2 * in], ph[2 * in + 1], code, sample, &out_iq[0], &out_iq[1]);
}
