// k_wideband_common.h — what the four wideband kernels (k_wb_ddc, k_wbr_ddc, k_wbtx_duc, k_wbtxr_duc) share, once each: the LO
// table and its closed-form lookup, the mix down and up, the round / clamp / pack tail, the front door's next carry and span
// fetch, the transmit bank's next carry. Everything is forced inline; T is the kernel's thread count. The helpers are handed plain
// values, not the kernel's argument struct: a reference to it gives the by-value kernel argument an address, and pointers loaded
// through it are no longer known to be global. What is a kernel's own - its shape and LDS layout, the index arithmetic of its
// resampling, its tap loop - stays in its .hip file.
#ifndef K_WIDEBAND_COMMON_H
#define K_WIDEBAND_COMMON_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "opv_wb_rules.h"

// the LO table T[4096] (opv_wb_lo_table), from global memory into LDS
template <uint32_t T>
__device__ __forceinline__ void wb_load_lo(int16_t* lo, const int16_t* table, uint32_t tid) {
    for (uint32_t i = tid; i < 4096; i += T) lo[i] = table[i];
}

// (c, s) = (cos, sin) of phase phi in turns / 2^32: the top 12 bits index T, the sine is the cosine a quarter turn back.
// (two results by reference, not a struct by value: returned by value the pair is packed into 64 bits before the call is
// inlined, and the 64-bit multiplies of wb_mix_up no longer see two sign-extended 16-bit factors)
__device__ __forceinline__ void wb_lo_at(const int16_t* lo, uint32_t phi, int& c, int& s) {
    const uint32_t ix = phi >> 20;
    c = lo[ix];
    s = lo[(ix - 1024u) & 4095u];
}

// the same pair from a phase in turns / 2^64 (the LO schedule's phi64): the one place that takes an index from it
__device__ __forceinline__ void wb_lo_at64(const int16_t* lo, uint64_t phi, int& c, int& s) {
    const uint32_t ix = (uint32_t)(phi >> 52);
    c = lo[ix];
    s = lo[(ix - 1024u) & 4095u];
}

// ---- where a kernel's LO comes from: a phase functor. Lo::channel(table, base, k, first) is asked once per (workgroup, channel)
// with `first`, the workgroup's first sample as an index within the push (wrapping 32 bits; the front door's may lie in front of the
// push); what it returns gives (c, s) of the workgroup's sample j: lo_of(lo, j, c, s). The bodies of the kernels are written once
// against it. `table` and `base` are handed over as plain values, like everything else here, not kept in members.
//
// WbLoFixed: the LO of an object that was never retuned, phi = (uint32)(a x inc_k) with a = a0_lo + first + j; table = inc[K], base = a0_lo
struct WbLoFixed {
    typedef uint32_t Table;
    struct Chan {
        uint32_t inc, a_base;
        __device__ __forceinline__ void operator()(const int16_t* lo, uint32_t j, int& c, int& s) const { wb_lo_at(lo, (a_base + j) * inc, c, s); }
    };
    static __device__ __forceinline__ Chan channel(const uint32_t* inc, uint32_t a0_lo, uint32_t k, uint32_t first) { return Chan{inc[k], a0_lo + first}; }
};

// WbLoTuned: the LO schedule; table = sched[K], channel k's table for this push (opv_wb_rules.h, OpvWbDevSched), base = back: local
// index first + back + j of the table is the workgroup's sample j. A workgroup spans at most OPV_WB_TUNE_GAP samples, so it meets at most
// two segments: both are fetched here, uniform per (workgroup, channel) - scalar loads - and a sample selects by one compare
// against the boundary. Per sample: d < 2^32, tri(d) = d (d - 1) / 2 < 2^63 exactly, then the low 64 bits of d x inc (32 x 64) and
// of ramp x tri (64 x 64).
struct WbLoTuned {
    typedef OpvWbDevSched Table;
    struct Chan {
        uint32_t base, start0, start1;
        uint64_t phase0, inc0, ramp0, phase1, inc1, ramp1;
        __device__ __forceinline__ void operator()(const int16_t* lo, uint32_t j, int& c, int& s) const {
            const uint32_t jj = base + j;
            const bool late = jj >= start1;
            const uint32_t d = jj - (late ? start1 : start0);
            const uint64_t tri = ((uint64_t)d * (uint64_t)(d - 1u)) >> 1;      // (d = 0: 0 x (2^32 - 1))
            wb_lo_at64(lo, (late ? phase1 : phase0) + (uint64_t)d * (late ? inc1 : inc0) + (late ? ramp1 : ramp0) * tri, c, s);
        }
    };
    static __device__ __forceinline__ Chan channel(const OpvWbDevSched* sched, uint32_t back, uint32_t k, uint32_t first) {
        const OpvWbDevSched* t = sched + k;
        Chan ch;
        ch.base = first + back;
        uint32_t n = 0;
#pragma unroll
        for (uint32_t i = 0; i < (uint32_t)OPV_WB_TUNE_SEGS; ++i) n += t->start[i] <= ch.base ? 1u : 0u;
        const uint32_t s0 = n ? n - 1u : 0u;                               // (nothing begins at or before the first sample: only
                                                                           // samples in front of the object's history, which are zeros)
        const uint32_t s1 = s0 + 1u < (uint32_t)OPV_WB_TUNE_SEGS ? s0 + 1u : s0;
        ch.start0 = t->start[s0];
        ch.start1 = s1 != s0 ? t->start[s1] : 0xFFFFFFFFu;
        ch.phase0 = t->phase[s0]; ch.inc0 = t->inc[s0]; ch.ramp0 = (uint64_t)t->ramp[s0];
        ch.phase1 = t->phase[s1]; ch.inc1 = t->inc[s1]; ch.ramp1 = (uint64_t)t->ramp[s1];
        return ch;
    }
};

// down: packed (I | Q << 16) times (c - i s)
__device__ __forceinline__ int2 wb_mix_down(int x, int c, int s) {
    const int I = (int16_t)(x & 0xFFFF), Q = x >> 16;
    return make_int2(I * c + Q * s, Q * c - I * s);
}

// up: the conjugate of the DDC's mix, (yr + i yi) times (c + i s), added to the sum over the channels
__device__ __forceinline__ void wb_mix_up(int64_t& wr, int64_t& wi, int yr, int yi, int c, int s) {
    wr += (int64_t)yr * c - (int64_t)yi * s;
    wi += (int64_t)yi * c + (int64_t)yr * s;
}

// floor((acc + 2^(S-1)) / 2^S) - an arithmetic shift - clamped to int16 and packed I | Q << 16
__device__ __forceinline__ int wb_round_pack(int64_t re, int64_t im, uint32_t S) {
    const int64_t half = S ? (int64_t)1 << (S - 1) : 0;
    re = (re + half) >> S;
    im = (im + half) >> S;
    re = re < -32768 ? -32768 : re > 32767 ? 32767 : re;
    im = im < -32768 ? -32768 : im > 32767 ? 32767 : im;
    return (int)(((uint32_t)im << 16) | ((uint32_t)re & 0xFFFFu));
}

// ---- the front door (k_wb_ddc, k_wbr_ddc)

// the carry of the NEXT push: the last `carry` samples of (carry, this push). It goes to the other buffer, so nobody's reads race it.
template <uint32_t T>
__device__ __forceinline__ void wb_write_next_carry(int* hist_out, const int* hist_in, uint32_t hist_len, const int* src, uint32_t n_new,
                                                    uint64_t n_before, uint32_t carry, uint32_t tid) {
    if (blockIdx.x != 0 || blockIdx.y != 0) return;
    const uint64_t have = n_before + n_new;
    const uint32_t keep = have < (uint64_t)carry ? (uint32_t)have : carry;
    const uint32_t from = hist_len + n_new - keep;                     // index into (hist_in, src) laid end to end
    for (uint32_t i = tid; i < keep; i += T) {
        const uint32_t ci = from + i;
        hist_out[i] = ci < hist_len ? hist_in[ci] : src[ci - hist_len];
    }
}

// The workgroup's span of wide samples into LDS: local sample j is src[base_i + j] - in front of src[0] lie the hist_len samples of
// hist_in - and lands in raw[slot(j)]. (slot by reference: a closure handed over by value is packed like wb_lo_at's pair would be,
// and the integer door's slot arithmetic then compiles to slower code)
template <uint32_t T, class Slot>
__device__ __forceinline__ void wb_fetch_span(int* raw, const int* hist_in, uint32_t hist_len, const int* src, uint32_t n_new, int64_t base_i,
                                              uint32_t span, uint32_t tid, const Slot& slot) {
    // (1) what lies in front of this push (the carry, zeros before sample 0) and behind it (zeros: no output of this push reads them)
    for (uint32_t j = tid; j < span; j += T) {
        const int64_t i = base_i + (int64_t)j;
        if (i < 0) {
            const int64_t h = (int64_t)hist_len + i;
            raw[slot(j)] = h >= 0 ? hist_in[h] : 0;
        } else if (i >= (int64_t)n_new) {
            raw[slot(j)] = 0;
        }
    }
    // (2) the part inside this push, in 16-byte pieces of the source wherever a whole piece lies inside both the push and the span
    const int64_t i_lo = base_i > 0 ? base_i : 0;
    const int64_t i_end = base_i + (int64_t)span < (int64_t)n_new ? base_i + (int64_t)span : (int64_t)n_new;
    if (i_end <= i_lo) return;
    const int64_t mis = (int64_t)(((uintptr_t)src >> 2) & 3u);         // src[4 q - mis] is 16-byte aligned
    const int64_t q_lo = (i_lo + mis) >> 2, q_hi = (i_end - 1 + mis) >> 2;
    for (int64_t q = q_lo + tid; q <= q_hi; q += T) {
        const int64_t i = 4 * q - mis;
        if (i >= i_lo && i + 4 <= i_end) {
            const int4 v = *(const int4*)(src + i);
            const uint32_t j = (uint32_t)(i - base_i);
            raw[slot(j)] = v.x;
            raw[slot(j + 1)] = v.y;
            raw[slot(j + 2)] = v.z;
            raw[slot(j + 3)] = v.w;
        } else {
            for (int64_t e = i; e < i + 4; ++e)
                if (e >= i_lo && e < i_end) raw[slot((uint32_t)(e - base_i))] = src[e];
        }
    }
}

// ---- the transmit bank (k_wbtx_duc, k_wbtxr_duc)

// the carry of the NEXT push: the last H samples of (carry, this push) of every channel, channel k by workgroup k % gridDim.x. It
// goes to the other buffer, so nobody's reads race it. (a push shorter than H: ci < H takes what is left of the old carry)
template <uint32_t T>
__device__ __forceinline__ void wbtx_write_next_carry(int* hist_out, const int* hist_in, uint32_t H, const int* const* in, uint32_t n_in, uint32_t K,
                                                      uint32_t tid) {
    for (uint32_t k = blockIdx.x; k < K; k += gridDim.x) {
        const int* src = in[k];
        const int* old = hist_in + (size_t)k * H;
        int* nxt = hist_out + (size_t)k * H;
        for (uint32_t i = tid; i < H; i += T) {
            const uint64_t ci = (uint64_t)n_in + i;                  // index into (old, src) laid end to end
            nxt[i] = ci < H ? old[ci] : src ? src[ci - H] : 0;
        }
    }
}

#endif
