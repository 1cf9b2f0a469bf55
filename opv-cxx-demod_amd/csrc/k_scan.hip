// k_scan.hip — k_scan_probe and k_scan_reduce: the wideband scan's probe bank (include/opv_demod.h, opv_scan_*). One launch of
// each per push serves all P probes and every block the push completes: mix the wide capture at +f_p down to 0 with the doors'
// closed-form integer LO, weigh a segment of Lw samples with the int16 window, sum (int64, |z| < 2^52), round, clamp to 25 bits,
// square, and add the segments of a block. The arithmetic is integer-exact and independent of summation order, so parity with the
// numpy model is `==`.
//
// Shape: workgroup (x, y) takes one run of segments of one block (opv_scan_internal.h) for probes [256 y, + 256), one lane per
// probe. Per segment it fetches the Lw samples ONCE into LDS and forms window[t] I and window[t] Q (int32, |.| <= 2^30) once per
// sample: they are the same for every probe, and z = sum_t window[t] (I c + Q s) = sum_t (window[t] I) c + (window[t] Q) s exactly.
// A lane then walks t with phi += inc from the closed-form start (uint32 wraparound keeps that exact), reads the products as an
// LDS broadcast and the LO by gather - from a table of (c | s << 16) pairs built once per workgroup through wb_lo_at, one gather
// per sample instead of two - and does four 32 x 32 + 64-bit multiply-adds. Each workgroup's sums go to a place of their own in
// `part`; k_scan_reduce adds a block's runs in a fixed order into the block's row of the ring: no atomics, no partial rows
// between pushes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k_wideband_common.h"
#include "opv_scan_internal.h"

namespace {

// floor((z + 2^(S-1)) / 2^S) - an arithmetic shift - clamped to 25 bits
__device__ __forceinline__ int64_t scan_round_clamp(int64_t z, uint32_t S) {
    const int64_t half = S ? (int64_t)1 << (S - 1) : 0;
    z = (z + half) >> S;
    return z < -(1 << 24) ? -(1 << 24) : z > (1 << 24) - 1 ? (1 << 24) - 1 : z;
}

// The carry of the NEXT push: the last `keep` samples of (hist_in, src) laid end to end, to the other buffer, so nobody's reads
// race it. A carry is up to a block's span (2^20 samples), not a door's filter length: every workgroup of the grid takes a share.
__device__ __forceinline__ void scan_write_next_carry(int* hist_out, const int* hist_in, uint32_t hist_len, const int* src, uint32_t n_new,
                                                      uint32_t keep, uint32_t tid) {
    const uint32_t from = hist_len + n_new - keep;                      // (keep <= hist_len + n_new: opv_scan_rules.h, scan_push_plan)
    const uint32_t wg = blockIdx.y * gridDim.x + blockIdx.x, n_wg = gridDim.x * gridDim.y;
    for (uint64_t i = (uint64_t)wg * OPV_SCAN_THREADS + tid; i < keep; i += (uint64_t)n_wg * OPV_SCAN_THREADS) {
        const uint32_t ci = from + (uint32_t)i;
        hist_out[i] = ci < hist_len ? hist_in[ci] : src[ci - hist_len];
    }
}

}  // namespace

extern "C" __global__ __launch_bounds__(256) void k_scan_probe(OpvScanArgs a) {
    __shared__ int raw[OPV_SCAN_WINDOW];          // the segment in hand: packed int16 I | Q << 16
    __shared__ int2 prod[OPV_SCAN_WINDOW];        // (window[t] I, window[t] Q)
    __shared__ uint32_t cs[4096];                 // (uint16) c | s << 16 of LO index i
    const uint32_t tid = threadIdx.x;
    const uint32_t Lw = a.Lw;

    scan_write_next_carry(a.hist_out, a.hist_in, a.hist_len, a.src, a.n_new, a.keep, tid);
    if (blockIdx.x >= a.blocks * a.runs) return;
    const uint32_t blk = blockIdx.x / a.runs, run = blockIdx.x - blk * a.runs;
    const uint32_t seg0 = run * a.run_len;
    const uint32_t seg1 = seg0 + a.run_len < a.A ? seg0 + a.run_len : a.A;

    for (uint32_t i = tid; i < 4096; i += OPV_SCAN_THREADS) {
        int c, s;
        wb_lo_at(a.lo, i << 20, c, s);
        cs[i] = ((uint32_t)c & 0xFFFFu) | ((uint32_t)s << 16);
    }
    const uint32_t p = blockIdx.y * OPV_SCAN_THREADS + tid;
    const uint32_t inc = p < a.P ? a.inc[p] : 0u;                       // (a lane without a probe computes probe "0 Hz" and stores nothing)
    uint64_t sum = 0;
    for (uint32_t seg = seg0; seg < seg1; ++seg) {
        // local sample t of the segment is src[base_i + t]: in front of src[0] lies the carry
        const int64_t base_i = a.base0 + (int64_t)((uint64_t)blk * a.A + seg) * (int64_t)a.H;
        __syncthreads();                                                // (the lanes of the segment before are done with prod)
        wb_fetch_span<OPV_SCAN_THREADS>(raw, a.hist_in, a.hist_len, a.src, a.n_new, base_i, Lw, tid, [](uint32_t j) { return j; });
        __syncthreads();
        for (uint32_t t = tid; t < Lw; t += OPV_SCAN_THREADS) {
            const int x = raw[t], w = a.window[t];
            prod[t] = make_int2(w * (int)(int16_t)(x & 0xFFFF), w * (x >> 16));
        }
        __syncthreads();
        // phase of local sample t: phi = (uint32)((first_sample + n) * inc) - the low 32 bits only, so 32-bit arithmetic that wraps
        uint32_t phi = (a.a0_lo + (uint32_t)(uint64_t)base_i) * inc;
        int64_t zr = 0, zi = 0;
#pragma unroll 4
        for (uint32_t t = 0; t < Lw; ++t) {
            const uint32_t e = cs[phi >> 20];
            const int c = (int16_t)(e & 0xFFFFu), s = (int)e >> 16;
            const int2 m = prod[t];
            zr += (int64_t)m.x * c + (int64_t)m.y * s;                  // w (I c + Q s)
            zi += (int64_t)m.y * c - (int64_t)m.x * s;                  // w (Q c - I s)
            phi += inc;
        }
        const int64_t yr = scan_round_clamp(zr, a.S), yi = scan_round_clamp(zi, a.S);
        sum += (uint64_t)(yr * yr) + (uint64_t)(yi * yi);
    }
    if (p < a.P) a.part[(uint64_t)blockIdx.x * a.P + p] = sum;
}

extern "C" __global__ __launch_bounds__(256) void k_scan_reduce(OpvScanReduceArgs a) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= (uint64_t)a.blocks * a.P) return;
    const uint32_t b = (uint32_t)(i / a.P), p = (uint32_t)(i - (uint64_t)b * a.P);
    // eight loads in flight per step: a block cut into hundreds of runs is one thread's chain of memory round trips otherwise
    // (uint64 addition: any order gives the same sum)
    const uint64_t* in = a.part + (uint64_t)b * a.runs * a.P + p;
    uint64_t s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    uint32_t r = 0;
    for (; r + 8 <= a.runs; r += 8) {
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) s[k] += in[(uint64_t)(r + k) * a.P];
    }
    for (; r < a.runs; ++r) s[0] += in[(uint64_t)r * a.P];
    a.rows[(uint64_t)((a.head + b) % a.ring) * a.P + p] = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]));
}
