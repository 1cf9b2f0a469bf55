// tune_rules_probe.cpp - TEST INFRASTRUCTURE (tests/san_tune/Makefile): the LO schedule's rules of csrc/opv_wb_rules.cpp driven by a
// program of its own, so that they run under ASan + UBSan without Python and without a device. It checks by itself what needs no
// model - a segment's phase against 128-bit arithmetic, every refusal and that it changes nothing, pruning, and the per-push device
// table against the absolute formula on every local index - exits 1 on the first miss, and prints the phases and segments of a
// fixed walk for tests/test_wideband_tune_host.py to hold to tests/wideband_tune_model.py.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "opv_wb_rules.h"

namespace {

int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            std::printf("MISS %s:%d %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

uint64_t phase128(const opv_wb_seg& s, uint64_t a) {
    const unsigned __int128 d = (uint64_t)(a - s.start);
    const unsigned __int128 tri = d ? d * (d - 1) / 2 : 0;              // < 2^127
    return (uint64_t)(s.phase + (uint64_t)d * s.inc + (uint64_t)s.ramp * (uint64_t)tri);
}

uint64_t rng_state = 0x9E3779B97F4A7C15ull;
uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

bool same(const std::vector<opv_wb_seg>& a, const std::vector<opv_wb_seg>& b) {
    return a.size() == b.size() && (a.empty() || !std::memcmp(a.data(), b.data(), a.size() * sizeof(opv_wb_seg)));
}

// what the device computes from a table entry for local index j (k_wideband_common.h, WbLoTuned), with at most two segments in
// reach of `first`, against the absolute rule
void check_table(const WbSchedule& s, uint64_t origin, uint64_t reach, uint32_t span) {
    std::vector<OpvWbDevSched> tab(s.seg.size());
    wb_sched_table(s, origin, reach, tab.data());
    for (size_t k = 0; k < s.seg.size(); ++k) {
        const OpvWbDevSched& t = tab[k];
        const std::vector<opv_wb_seg>& seg = s.seg[k];
        for (uint64_t first = 0; first < reach; first += span) {
            uint32_t n = 0;
            for (int i = 0; i < OPV_WB_TUNE_SEGS; ++i) n += t.start[i] <= (uint32_t)first;
            const uint32_t s0 = n ? n - 1 : 0, s1 = s0 + 1 < (uint32_t)OPV_WB_TUNE_SEGS ? s0 + 1 : s0;
            const uint32_t start1 = s1 != s0 ? t.start[s1] : 0xFFFFFFFFu;
            for (uint64_t j = first; j < first + span && j < reach; j += 1 + (j % 7 == 0 ? 0 : rnd() % 5)) {
                const uint64_t a = origin + j;
                size_t cur = seg.size();
                for (size_t i = 0; i < seg.size(); ++i)
                    if ((int64_t)(a - seg[i].start) >= 0) cur = i;
                if (cur == seg.size()) continue;                            // in front of the oldest live segment: nothing to hold
                const bool late = (uint32_t)j >= start1;
                const uint32_t e = late ? s1 : s0;
                const uint32_t d = (uint32_t)j - t.start[e];
                const uint64_t tri = ((uint64_t)d * (uint64_t)(d - 1u)) >> 1;
                const uint64_t phi = t.phase[e] + (uint64_t)d * t.inc[e] + (uint64_t)t.ramp[e] * tri;
                CHECK(phi == wb_seg_phase(seg[cur], a));
                if (failures) return;
            }
        }
    }
}

void print_segs(const char* tag, const WbSchedule& s, int k) {
    opv_wb_seg out[OPV_WB_TUNE_SEGS];
    const int n = wb_sched_copy(s, k, out, OPV_WB_TUNE_SEGS);
    std::printf("%s %d", tag, n);
    for (int i = 0; i < n; ++i) std::printf(" %" PRIu64 ":%" PRIu64 ":%" PRIu64 ":%" PRId64, out[i].start, out[i].phase, out[i].inc, out[i].ramp);
    std::printf("\n");
}

}  // namespace

int main() {
    const char* why = nullptr;
    // ---- a segment's phase: the edges of d, both signs of the ramp, an increment with the top bit set, random
    const uint64_t ds[] = {0, 1, (1ull << 31) - 1, (1ull << 31) + 1, (1ull << 32) - 1, (1ull << 32) + 1, 1ull << 63, ~0ull};
    for (int sign = -1; sign <= 1; sign += 2)
        for (uint64_t d : ds) {
            const opv_wb_seg s{12345, 0x0123456789ABCDEFull, 0xF000000100000000ull, sign * 38912345678901ll};
            CHECK(wb_seg_phase(s, s.start + d) == phase128(s, s.start + d));
            std::printf("phase %d %" PRIu64 " %" PRIu64 "\n", sign, d, wb_seg_phase(s, s.start + d));
        }
    for (int i = 0; i < 20000; ++i) {
        const opv_wb_seg s{rnd(), rnd(), rnd(), (int64_t)rnd()};
        const uint64_t a = rnd() >> (rnd() % 64);
        CHECK(wb_seg_phase(s, a) == phase128(s, a));
    }
    // ---- a successor, and what refuses one
    opv_wb_seg prev{0, 0, 0x1234567800000000ull, 0}, next{};
    CHECK(wb_seg_next(&prev, 1250, 271, 100000, -3.1e6, -2.5e5, &next, &why) == OPV_OK && next.start == 100000 && next.phase == wb_seg_phase(prev, 100000));
    std::printf("next %" PRIu64 " %" PRIu64 " %" PRId64 "\n", next.phase, next.inc, next.ramp);
    CHECK(wb_seg_next(nullptr, 4, 1, 0, 0, 0, &next, &why) == OPV_EINVAL && wb_seg_next(&prev, 4, 1, 0, 0, 0, nullptr, &why) == OPV_EINVAL);
    CHECK(wb_seg_next(&prev, 0, 1, 0, 0, 0, &next, &why) == OPV_EINVAL && wb_seg_next(&prev, 4, 0, 0, 0, 0, &next, &why) == OPV_EINVAL);
    CHECK(wb_seg_next(&prev, 4, 1, 0, 0.0 / 0.0, 0, &next, &why) == OPV_EINVAL && wb_seg_next(&prev, 4, 1, 0, 0, 1.0 / 0.0, &next, &why) == OPV_EINVAL);
    CHECK(wb_seg_next(&prev, 4, 1, 0, 0, 1.0e7, &next, &why) == OPV_OK && wb_seg_next(&prev, 4, 1, 0, 0, -1.0000001e7, &next, &why) == OPV_EINVAL);
    // ---- a schedule: retunes, refusals that change nothing, pruning, the device table
    const uint32_t inc[3] = {0x10000000u, 0xF0000000u, 0x00012345u};
    const uint64_t first = (1ull << 32) - 3000;
    WbSchedule s;
    wb_sched_reset(s, 4, 1, 3, inc);
    CHECK(wb_sched_plain(s));
    check_table(s, first - kWbSchedBack, 20000 + kWbSchedBack, 4096);
    uint64_t A = first;
    auto tune = [](int ch, uint64_t at, double f, double r) { return opv_wb_tune{ch, 0, at, f, r, 0}; };
    const std::vector<std::vector<opv_wb_seg>> before = s.seg;
    const opv_wb_tune bad_batches[][2] = {
        {tune(0, A + 10, 1e5, 0), tune(3, A + 10, 1e5, 0)},                 // a channel out of range, behind a good entry
        {tune(0, A + 10, 1e5, 0), tune(-1, A + 10, 1e5, 0)},
        {tune(1, A + 10, 0.0 / 0.0, 0), tune(0, A + 10, 1e5, 0)},
        {tune(1, A + 10, 0, 1.0 / 0.0), tune(0, A + 10, 1e5, 0)},
        {tune(1, A + 10, 0, 2e7), tune(0, A + 10, 1e5, 0)},
        {tune(1, A + 10, 1e5, 0), tune(1, A + 10 + OPV_WB_TUNE_GAP - 1, 1e5, 0)},   // two entries of one channel inside the gap
        {tune(1, A + 5000, 1e5, 0), tune(1, A + 10, 1e5, 0)},               // ... and out of order
    };
    for (const auto& b : bad_batches) {
        CHECK(wb_sched_retune(s, A, A, 2, b, &why) == OPV_EINVAL);
        CHECK(same(s.seg[0], before[0]) && same(s.seg[1], before[1]) && same(s.seg[2], before[2]) && wb_sched_plain(s));
    }
    CHECK(wb_sched_retune(s, A, A, -1, bad_batches[0], &why) == OPV_EINVAL && wb_sched_retune(s, A, A, 1, nullptr, &why) == OPV_EINVAL);
    CHECK(wb_sched_retune(s, A, A, 0, nullptr, &why) == OPV_OK && wb_sched_plain(s));
    {
        const opv_wb_tune past[2] = {tune(0, A + 10, 1e5, 0), tune(1, A + 4999, 1e5, 0)};
        CHECK(wb_sched_retune(s, A + 5000, A + 5000 - 320, 2, past, &why) == OPV_ESTATE && wb_sched_plain(s));
    }
    // channel 0: replaced at the object's first sample; channel 1: a ramp, then two more exactly a gap apart; channel 2 stays
    const opv_wb_tune good[] = {tune(0, A, -2.2e6, -3e5), tune(1, A + 777, 1.5e6, 4e5), tune(1, A + 777 + OPV_WB_TUNE_GAP, 1.4e6, 0),
                                tune(1, A + 777 + 2 * OPV_WB_TUNE_GAP, -1.4e6, -1e7)};
    CHECK(wb_sched_retune(s, A, A, 4, good, &why) == OPV_OK && !wb_sched_plain(s));
    CHECK(s.seg[0].size() == 1 && s.seg[0][0].start == A && !s.created[0] && s.seg[1].size() == 4 && s.created[1] && s.seg[2].size() == 1);
    print_segs("segs0", s, 0);
    print_segs("segs1", s, 1);
    CHECK(wb_sched_copy(s, 3, nullptr, 0) == OPV_EINVAL && wb_sched_copy(s, -1, nullptr, 0) == OPV_EINVAL && wb_sched_copy(s, 1, nullptr, 0) == 4);
    {
        opv_wb_tune given = tune(2, A + 100, 1e5, 0);
        given.phase_given = 1;
        given.phase = 0xDEADBEEF00000000ull;
        CHECK(wb_sched_retune(s, A, A, 1, &given, &why) == OPV_OK && s.seg[2].back().phase == given.phase);
    }
    for (uint64_t origin : {first - kWbSchedBack, first - 1, first + 776, first + 777, first + 778, first + 777 + OPV_WB_TUNE_GAP - 4095})
        for (uint32_t span : {4096u, 256u, 1000u}) check_table(s, origin, 30000, span);
    // pushes: the receive rule keeps what the carried history still needs, the transmit rule nothing behind A
    WbSchedule rx = s, tx = s;
    A = first + 777 + OPV_WB_TUNE_GAP + 100;
    wb_sched_prune(rx, A - 320);
    wb_sched_prune(tx, A);
    CHECK(rx.seg[1].size() == 3 && !rx.created[1] && rx.seg[1][0].start == first + 777);      // the ramp reaches into the history: kept
    CHECK(tx.seg[1].size() == 2 && tx.seg[1][0].start == first + 777 + OPV_WB_TUNE_GAP);
    wb_sched_prune(rx, first + 777 + OPV_WB_TUNE_GAP);                                          // a successor AT the oldest sample: dropped
    CHECK(rx.seg[1].size() == 2);
    check_table(rx, A - kWbSchedBack, 30000, 4096);
    check_table(tx, A, 30000, 256);
    print_segs("rx1", rx, 1);
    print_segs("tx1", tx, 1);
    // the 17th segment: sixteen fit (the first one replaced the creation segment), one more does not, and changes nothing
    {
        WbSchedule c;
        wb_sched_reset(c, 1250, 271, 1, inc);
        for (int i = 0; i < OPV_WB_TUNE_SEGS; ++i) {
            const opv_wb_tune t = tune(0, 500 + (uint64_t)i * OPV_WB_TUNE_GAP, 1e5 * i, 1e3 * i);
            CHECK(wb_sched_retune(c, 500, 500, 1, &t, &why) == OPV_OK);
        }
        CHECK(c.seg[0].size() == (size_t)OPV_WB_TUNE_SEGS);
        const std::vector<opv_wb_seg> full = c.seg[0];
        const opv_wb_tune t = tune(0, 500 + 16ull * OPV_WB_TUNE_GAP, 0, 0);
        CHECK(wb_sched_retune(c, 500, 500, 1, &t, &why) == OPV_ECAPACITY && same(c.seg[0], full));
        check_table(c, 500 - (uint64_t)kWbSchedBack, 80000, 4096);                              // (an origin in front of sample 0: it wraps)
        CHECK(wb_sched_retune(c, 500 + 3ull * OPV_WB_TUNE_GAP, 500 + 3ull * OPV_WB_TUNE_GAP - 95, 1, &t, &why) == OPV_OK && c.seg[0].size() == 15);
        wb_sched_reset(c, 1250, 271, 1, inc);
        CHECK(wb_sched_plain(c));
    }
    std::printf("failures %d\n", failures);
    return failures ? 1 : 0;
}
