// opv_scan_internal.h — what opv_scan.hip hands k_scan.hip's two kernels, by value, filled once per push. Sample n of the object
// (0 = the first sample ever pushed) has the absolute index first_sample + n; this push holds samples [N, N + n_new) in src, and
// in front of src[0] lie the hist_len samples of hist_in (the carry: everything from the start of the first unfinished block on).
#ifndef OPV_SCAN_INTERNAL_H
#define OPV_SCAN_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

constexpr uint32_t OPV_SCAN_THREADS = 256;   // one lane per probe (= kScanLanes, asserted in opv_scan.hip)
constexpr uint32_t OPV_SCAN_WINDOW = 4096;   // Lw at most (= kScanMaxWindow)

// Arguments of k_scan_probe. Workgroup (x, y): x < blocks * runs takes run x % runs of the push's block x / runs - segments
// [run * run_len, + run_len) of its A - for probes [y * 256, + 256), and writes its sums to part[(x * P) + p]. Workgroups beyond
// (a push that completes nothing) only help with the carry. Every workgroup first copies its share of the next carry.
struct OpvScanArgs {
    const int* src;          // n_new packed (I | Q << 16) samples, device-visible
    const int* hist_in;      // the hist_len samples in front of src[0]
    int* hist_out;           // the other carry buffer: the last `keep` samples of (hist_in, src)
    const int16_t* lo;       // T[4096]
    const int16_t* window;   // window[Lw]
    const uint32_t* inc;     // inc[P]
    uint64_t* part;          // part[blocks * runs][P]
    int64_t base0;           // where the push's first completed block starts, as an index into src (negative: inside the carry)
    uint32_t a0_lo;          // low 32 bits of first_sample + N: the absolute index of src[0], all the closed-form phase needs
    uint32_t n_new, hist_len, keep;
    uint32_t P, Lw, H, A, S;
    uint32_t blocks, runs, run_len;
};
extern "C" __global__ void k_scan_probe(OpvScanArgs a);

// rows[((head + b) % ring) * P + p] = the sum over r < runs of part[(b * runs + r) * P + p], for b < blocks: one thread per (b, p)
struct OpvScanReduceArgs {
    const uint64_t* part;
    uint64_t* rows;
    uint32_t head, ring, blocks, runs, P;
};
extern "C" __global__ void k_scan_reduce(OpvScanReduceArgs a);

#endif
