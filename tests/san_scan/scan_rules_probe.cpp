// tests/san_scan/scan_rules_probe.cpp - TEST INFRASTRUCTURE: a stand-alone program over csrc/opv_scan_rules.cpp (built by the
// Makefile beside it with and without -fsanitize=address,undefined; tests/test_scan_host.py runs both and compares what they print).
//   argv[1]: rows for scan_carriers, one case per line: name f0 step half_width (hex doubles) ratio_q8 cap P row[0] .. row[P-1]
//   argv[2]: shapes, one per line: Lw H A N_0 N_1 ...
// Every buffer handed to the rules is a heap allocation of exactly the size the rule may touch. A wrong answer ends the program
// with an exit status of its own (2 .. 5), so that a clean sanitizer run of wrong code does not pass.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <limits>
#include <random>
#include <sstream>
#include <string>
#include <vector>

#include "opv_scan_rules.h"

namespace {

opv_scan_cfg base_cfg() {
    opv_scan_cfg c{};
    c.down = 7; c.up = 4; c.n_probes = 2; c.n_window = 9; c.hop = 5; c.n_avg = 3; c.out_shift = 5; c.ring_blocks = 2;
    return c;
}

int plan_of(const opv_scan_cfg& c, const std::vector<double>& probes, const std::vector<int16_t>& window) {
    std::vector<uint32_t> inc(probes.size());
    const char* why = nullptr;
    const int rc = scan_plan(&c, probes.data(), window.data(), inc.data(), &why);
    if ((rc != 0) != (why != nullptr)) std::exit(2);
    return rc;
}

// every limit at its edge (accepted) and one step outside (OPV_EINVAL)
int walk_plans() {
    struct Edit { int32_t opv_scan_cfg::*field; int32_t value; bool ok; };
    const Edit edits[] = {
        {&opv_scan_cfg::n_window, 0, false}, {&opv_scan_cfg::n_window, 1, true}, {&opv_scan_cfg::n_window, 4096, true}, {&opv_scan_cfg::n_window, 4097, false},
        {&opv_scan_cfg::hop, 0, false}, {&opv_scan_cfg::hop, 1, true}, {&opv_scan_cfg::hop, 65537, false},
        {&opv_scan_cfg::n_avg, 0, false}, {&opv_scan_cfg::n_avg, 1, true}, {&opv_scan_cfg::n_avg, 4097, false},
        {&opv_scan_cfg::out_shift, -1, false}, {&opv_scan_cfg::out_shift, 0, true}, {&opv_scan_cfg::out_shift, 40, true}, {&opv_scan_cfg::out_shift, 41, false},
        {&opv_scan_cfg::ring_blocks, 0, false}, {&opv_scan_cfg::ring_blocks, 1, true}, {&opv_scan_cfg::ring_blocks, 4096, true}, {&opv_scan_cfg::ring_blocks, 4097, false},
        {&opv_scan_cfg::up, 0, false}, {&opv_scan_cfg::up, 8, false}, {&opv_scan_cfg::down, 129, false}, {&opv_scan_cfg::down, 6, false}, {&opv_scan_cfg::down, 127, true},
    };
    int n = 0;
    for (const Edit& e : edits) {
        opv_scan_cfg c = base_cfg();
        c.*(e.field) = e.value;
        const std::vector<double> probes(2, 1000.0);
        const std::vector<int16_t> window((size_t)(c.n_window > 0 ? c.n_window : 1), 1);
        if ((plan_of(c, probes, window) == 0) != e.ok) std::exit(2);
        ++n;
    }
    // the span: exactly 2^20 and one more; the hop's and the count's own edges inside it
    const int32_t spans[][4] = {{1025, 1023, 1024, 1}, {1025, 1023, 1025, 0}, {1, 65536, 4096, 1}, {17, 65536, 1, 0}, {4096, 256, 256, 1}, {4096, 256, 257, 0}};
    for (const auto& s : spans) {
        opv_scan_cfg c = base_cfg();
        c.n_avg = s[0]; c.hop = s[1]; c.n_window = s[2];
        if ((plan_of(c, std::vector<double>(2, 0.0), std::vector<int16_t>((size_t)c.n_window, 1)) == 0) != (s[3] == 1)) std::exit(2);
        ++n;
    }
    // P: 1, 1024, 1025; the window's gain: exactly 2^21 and one more; probes that are not finite
    for (int P : {1, 1024, 1025}) {
        opv_scan_cfg c = base_cfg();
        c.n_probes = P;
        if ((plan_of(c, std::vector<double>((size_t)P, 5.0), std::vector<int16_t>(9, 1)) == 0) != (P <= 1024)) std::exit(2);
        ++n;
    }
    for (int extra : {0, 1, -1}) {
        opv_scan_cfg c = base_cfg();
        c.n_window = 65;
        std::vector<int16_t> window(65, (int16_t)-32768);
        window[64] = (int16_t)extra;
        if ((plan_of(c, std::vector<double>(2, 0.0), window) == 0) != (extra == 0)) std::exit(2);
        ++n;
    }
    for (double bad : {std::numeric_limits<double>::quiet_NaN(), std::numeric_limits<double>::infinity(), -std::numeric_limits<double>::infinity(), 1e300}) {
        if (plan_of(base_cfg(), std::vector<double>{1000.0, bad}, std::vector<int16_t>(9, 1)) == 0) std::exit(2);
        ++n;
    }
    const char* why = nullptr;
    if (scan_plan(nullptr, nullptr, nullptr, nullptr, &why) == 0 || scan_cfg_refusal(nullptr) == nullptr) std::exit(2);
    return n;
}

// what a push's plan must satisfy whatever the counts are
void check_push(const opv_scan_cfg& c, uint64_t n_before, uint64_t n_new) {
    const ScanPush p = scan_push_plan(&c, n_before, n_new);
    const uint64_t stride = (uint64_t)c.n_avg * (uint64_t)c.hop;
    if (p.b0 != scan_blocks(&c, n_before) || p.b1 != scan_blocks(&c, n_before + n_new) || p.b1 < p.b0) std::exit(3);
    if (p.start != p.b0 * stride || p.keep >= scan_span(&c)) std::exit(3);
    if (p.b1 * stride + p.keep != n_before + n_new && !(p.keep == 0 && p.b1 * stride >= n_before + n_new)) std::exit(3);
}

// every split of a short capture: the pieces' blocks add up to the capture's, and the carry always holds what the next block reads
long walk_splits() {
    std::mt19937_64 rng(7);
    long pushes = 0;
    const int32_t shapes[][3] = {{5, 3, 2}, {4, 4, 1}, {3, 7, 3}, {1, 1, 1}, {9, 2, 4}, {2, 11, 2}};
    for (const auto& s : shapes) {
        opv_scan_cfg c = base_cfg();
        c.n_window = s[0]; c.hop = s[1]; c.n_avg = s[2];
        for (int trial = 0; trial < 400; ++trial) {
            const uint64_t N = 150 + rng() % 100;
            uint64_t at = 0, blocks = 0;
            uint32_t hist = 0;
            while (at < N) {
                uint64_t n = trial == 0 ? N : rng() % 3 == 0 ? rng() % 4 : rng() % 40;
                if (n > N - at) n = N - at;
                check_push(c, at, n);
                const ScanPush p = scan_push_plan(&c, at, n);
                if (p.b1 > p.b0 && p.start < at && at - p.start > hist) std::exit(4);          // the block starts in front of the carry
                if (p.keep > hist + n) std::exit(4);                                           // the next carry is not all there
                blocks += p.b1 - p.b0;
                hist = p.keep;
                at += n;
                ++pushes;
            }
            if (blocks != scan_blocks(&c, N)) std::exit(4);
        }
    }
    return pushes;
}

// the launch shape: the runs cover a block's segments with no empty run, the groups cover the probes; printed, so that the test
// holds its own restatement of the rule (scan_model.scan_shape, which the GPU cases' preconditions rest on) to this one
void walk_shapes() {
    for (int P : {1, 3, 65, 256, 257, 512, 1024})
        for (int A : {1, 3, 64, 67, 100, 338, 800, 1599, 4096})
            for (uint64_t blocks : {0ull, 1ull, 2ull, 3ull, 5ull, 31ull, 38ull, 59ull, 62ull, 600ull, 2048ull, 2049ull, 4096ull}) {
                opv_scan_cfg c = base_cfg();
                c.n_probes = P; c.n_avg = A; c.hop = 1; c.n_window = 1;
                const ScanShape s = scan_shape(&c, blocks);
                if (s.run_len < 1 || s.runs < 1 || (uint64_t)s.runs * s.run_len < (uint64_t)A || (uint64_t)(s.runs - 1) * s.run_len >= (uint64_t)A) std::exit(5);
                if (s.pgroups * kScanLanes < (uint32_t)P || (s.pgroups - 1) * kScanLanes >= (uint32_t)P) std::exit(5);
                std::printf("shape:%d:%d:%" PRIu64 " %u %u %u\n", P, A, blocks, s.run_len, s.runs, s.pgroups);
            }
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) return 64;
    std::printf("plans %d\n", walk_plans());
    std::printf("splits %ld\n", walk_splits());
    walk_shapes();
    // ---- the block count and a push's plan at the host test's counts
    std::ifstream shapes(argv[2]);
    for (std::string line; std::getline(shapes, line);) {
        std::istringstream in(line);
        opv_scan_cfg c = base_cfg();
        in >> c.n_window >> c.hop >> c.n_avg;
        if (scan_cfg_refusal(&c)) return 3;
        std::printf("blocks:%d:%d:%d", c.n_window, c.hop, c.n_avg);
        for (uint64_t N; in >> N;) {
            std::printf(" %" PRIu64, scan_blocks(&c, N));
            for (uint64_t n : {(uint64_t)0, (uint64_t)1, (uint64_t)scan_span(&c), (uint64_t)((1ull << 31) - 1)})
                if (N + n <= (1ull << 63)) check_push(c, N, n);
        }
        std::printf("\n");
    }
    // ---- scan_carriers on the host test's rows
    std::ifstream rows(argv[1]);
    for (std::string line; std::getline(rows, line);) {
        std::istringstream in(line);
        std::string name, f0, step, hw;
        uint32_t ratio;
        size_t cap;
        int P;
        in >> name >> f0 >> step >> hw >> ratio >> cap >> P;
        std::vector<uint64_t> row((size_t)P);
        for (auto& v : row) in >> v;
        if (!in) return 65;
        std::vector<opv_scan_carrier> out(cap);
        const char* why = nullptr;
        const long n = scan_carriers(row.data(), P, std::strtod(f0.c_str(), nullptr), std::strtod(step.c_str(), nullptr), std::strtod(hw.c_str(), nullptr),
                                     ratio, cap ? out.data() : nullptr, cap, &why);
        if (n < 0 || (size_t)n > cap) return 66;
        std::printf("carriers:%s %ld", name.c_str(), n);
        for (long k = 0; k < n; ++k) std::printf(" %d %a %a", out[(size_t)k].probe, out[(size_t)k].centre_hz, out[(size_t)k].excess);
        std::printf("\n");
    }
    // ---- and its refusals
    const uint64_t one = 5;
    opv_scan_carrier c1;
    const char* why = nullptr;
    if (scan_carriers(&one, 0, 0.0, 1.0, 1.0, 0, &c1, 1, &why) != OPV_EINVAL || scan_carriers(&one, 1, 0.0, 0.0, 1.0, 0, &c1, 1, &why) != OPV_EINVAL ||
        scan_carriers(&one, 1, 0.0, 1.0, -1.0, 0, &c1, 1, &why) != OPV_EINVAL || scan_carriers(nullptr, 1, 0.0, 1.0, 1.0, 0, &c1, 1, &why) != OPV_EINVAL ||
        scan_carriers(&one, 1, 0.0, 1.0, 1.0, 0, nullptr, 1, &why) != OPV_EINVAL || scan_carriers(&one, 1, 0.0, 1.0, 1.0, 0, &c1, 1, &why) != 1)
        return 67;
    return 0;
}
