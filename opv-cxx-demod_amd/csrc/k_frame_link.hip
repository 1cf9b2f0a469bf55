// k_frame_link.hip — the per-frame link report (include/opv_demod.h: opv_link): the decoded frame is re-encoded and held against
// the 2144 soft symbols it was decoded from. One wavefront per frame, behind k_frame_decode in the same round.
//
// No counterpart in the reference, which discards both sides of the comparison when FrameDecoder::decode returns
// (src/opv-demod.cpp:854-898). What is compared:
//   received: q_i, the 3-bit value of payload symbol i (:862-866) - the decoder's own quantiser (opv_frame_code.h, one
//             definition for both kernels) behind the same scale (st.fscale[], never re-summed): the integers are the decoder's;
//   expected: enc_i, bit i of randomise -> K=7 r=1/2 encode -> interleave (src/opv-mod.cpp:158-213) applied to the 134 decoded
//             bytes: the decoder's own trellis (:815-822: start state 0, G1 0x4F, G2 0x6D) run forwards over the decoded bits,
//             code bit j of it at payload symbol opv_interleave_addr(j) (:792-795).
// Trellis step t reads decoded bit t and its six predecessors: bit t is bit (1071 - t) & 7 of byte (1071 - t) >> 3 of the frame
// XOR the LFSR table (the packer, :878-884, backwards), so the seven bits t .. t - 6 are seven CONSECUTIVE bits of that byte
// string read as a little-endian number - one 16-bit LDS window and a shift; two zero bytes behind byte 133 are the zeros in
// front of t = 0. The algebra (window bit order, which parity is G1, the direction of the deinterleaver) was checked against the
// oracle's encoder in a numpy model before the kernel was written (scripts/models/frame_link_model.py).
//
// A lane takes steps t = lane, lane + 64, ... (17 trips, the last for lanes < 48) and both code bits of each; its 34 gathered
// doubles are requested before the first is used - the decoder's gather, opv_gather_payload (one round trip instead of 17). Three
// counts and two fp64 sums per lane, then an XOR butterfly over the wave in a fixed order: no atomics, so a frame's record is
// the same bits in every run and in both kernels below. Lane 0 stores the 40 bytes.
// Bytes: 17 152 B of soft symbols in (from L2 where the decoder has just read them; from HBM in bulk rounds), 134 B of frame in,
// 40 B out per frame. 136 B of LDS. No MFMA. 116 registers: four waves per SIMD, which is what a wave that lives for one frame
// and four dependent memory round trips needs - 512 000 frames in 1.9 ms, 4.6 TB/s (profiles/link_report_cost.txt).
#include <hip/hip_runtime.h>
#include <math.h>

#include "../../include/opv_demod.h"
#include "opv_device.h"
#include "opv_div_rules.h"
#include "opv_frame_code.h"

static_assert(sizeof(opv_link) == 40, "opv_link is 40 bytes");

namespace {

__constant__ OpvLfsrTable kLinkLfsr = opv_make_lfsr();

constexpr int kLinkLds = OPV_FB + 2;                              // the randomised frame + the zeros in front of t = 0

// One frame by one wave. payload = soft[(first + i) & mask], i < 2144; `scale` is the decoder's (ref :856-858), `metric` what the
// decoder returned for it, `frame` its 134 bytes. All arguments are wave-uniform.
__device__ __forceinline__ void link_one(const double* __restrict__ soft, uint32_t first, uint32_t mask, double scale, int32_t metric,
                                         const uint8_t* __restrict__ frame, opv_link* __restrict__ rec, uint8_t* s_bits) {
    int lane = threadIdx.x;
    // (opaque to the compiler: k_frame_link calls this in a loop, and with a lane number it can see through it hoists the 34
    // address and window computations of a lane out of that loop - 176 registers instead of 116, two waves per SIMD instead of
    // four, 2.4 ms instead of 1.9 ms for 512 000 frames). An empty barrier, no instruction: the one line of this file that is not
    // plain C++. The occupancy itself is stated where it belongs, __launch_bounds__(64, 4) on both kernels (at most 128 registers);
    // what rests on this line, and so on how one hipcc hoists, is that those four waves come WITHOUT scratch (with the bounds alone
    // this compiler spills 204 bytes per lane). Results never depend on it; `hipcc -Rpass-analysis=kernel-resource-usage` shows both.
    asm volatile("" : "+v"(lane));
    if (metric < 0) {                                             // dropped by the decoder (ref :859): valid = 0, every field 0
        if (lane == 0) { rec->valid = 0; rec->bit_errors = 0; rec->weak = 0; rec->nonfinite = 0; rec->m1 = 0.0; rec->m2 = 0.0; rec->ma = 0.0; }
        return;
    }
    for (int q = lane; q < kLinkLds; q += 64) s_bits[q] = q < OPV_FB ? (uint8_t)(frame[q] ^ kLinkLfsr.b[q]) : (uint8_t)0;
    double sv[2 * kLaneSteps];
    opv_gather_payload(soft, first, mask, lane, sv);
    __syncthreads();
    const double inv = -3.5 / scale;
    int n_err = 0, n_weak = 0, n_nonf = 0;
    double s2 = 0.0, sa = 0.0;
#pragma unroll
    for (int k = 0; k < kLaneSteps; ++k) {
        const int t = lane + 64 * k;
        if (t < OPV_FBITS) {
            // decoded bits t .. t - 6 = bits p .. p + 6 of the byte string, p = 1071 - t; f as the reference forms it (:819): the step's
            // input bit on top of the state, whose bit 0 is the newest earlier bit
            const uint32_t p = (uint32_t)(OPV_FBITS - 1 - t);
            const uint32_t w = (uint32_t)s_bits[p >> 3] | ((uint32_t)s_bits[(p >> 3) + 1] << 8);
            const uint32_t v = (w >> (p & 7u)) & 0x7Fu;
            const uint32_t f = ((v & 1u) << 6) | (v >> 1);
            const int e[2] = {(int)opv_code_g1(f), (int)opv_code_g2(f)};                   // code bits 2 t and 2 t + 1 (:820-824)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const double s = sv[2 * k + h];
                const int qv = opv_quantise3_unclamped(s, scale, inv);                         // the decoder's value; both tests below hold with or without its clamp
                n_err += ((qv >= 4) ? 1 : 0) != e[h];
                n_weak += (qv == 3 || qv == 4);
                n_nonf += !(fabs(s) <= 1.7976931348623157e308);                            // NaN or +-Inf
                s2 += s * s;
                sa += e[h] ? -s : s;
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {                      // fixed order: the same bits in every run
        n_err += __shfl_xor(n_err, off, 64);
        n_weak += __shfl_xor(n_weak, off, 64);
        n_nonf += __shfl_xor(n_nonf, off, 64);
        s2 += __shfl_xor(s2, off, 64);
        sa += __shfl_xor(sa, off, 64);
    }
    if (lane == 0) {
        rec->valid = 1; rec->bit_errors = n_err; rec->weak = n_weak; rec->nonfinite = n_nonf;
        rec->m1 = scale; rec->m2 = s2 / (double)OPV_CODED; rec->ma = sa / (double)OPV_CODED;
    }
    __syncthreads();                                              // the next frame reuses the buffer
}

}  // namespace

// grid = n_streams x per_stream (the round's estimate of frames per stream), flattened and strided like k_frame_scale_wave:
// frames dec_from + blockIdx.x % per_stream, + per_stream, ... up to n_frames, so that a released backlog is covered too.
// ring: [n_streams][cap_frames] records, frame f of a stream at slot f % cap_frames like the frame ring.
extern "C" __global__ __launch_bounds__(64, 4) void k_frame_link(OpvStream* __restrict__ streams, opv_link* __restrict__ ring, uint32_t cap_frames,
                                                               uint32_t per_stream) {
    __shared__ uint8_t s_bits[kLinkLds];
    const uint32_t sidx = blockIdx.x / per_stream;
    const OpvStream& st = streams[sidx];
    const uint32_t n_frames = st.n_frames, mask = (uint32_t)(st.cap_soft - 1);
    for (uint32_t f = st.dec_from + blockIdx.x % per_stream; f < n_frames; f += per_stream) {
        const uint32_t slot = f % cap_frames;
        link_one(st.soft, (uint32_t)st.frec[slot].payload_sym, mask, st.fscale[slot], st.metrics[slot], st.frames + (size_t)slot * OPV_FB,
                 ring + (size_t)sidx * cap_frames + slot, s_bits);
    }
}

// the stand-alone twin over plain arrays (opv_link_payloads), behind k_payload_scale and k_decode_payloads: one payload per wave
extern "C" __global__ __launch_bounds__(64, 4) void k_link_payloads(const double* __restrict__ soft, uint32_t n, const double* __restrict__ scales,
                                                                  const uint8_t* __restrict__ frames, const int32_t* __restrict__ metrics,
                                                                  opv_link* __restrict__ out) {
    __shared__ uint8_t s_bits[kLinkLds];
    const uint32_t f = blockIdx.x;
    if (f >= n) return;
    link_one(soft + (size_t)f * OPV_CODED, 0u, 0xFFFFFFFFu, scales[f], metrics[f], frames + (size_t)f * OPV_FB, out + f, s_bits);
}

// receive diversity (k_diversity.hip): the record of every combined payload of the round, behind k_div_decode; flattened and
// strided like k_frame_link
extern "C" __global__ __launch_bounds__(64, 4) void k_div_link(OpvDivGroup* __restrict__ groups, uint32_t per_group) {
    __shared__ uint8_t s_bits[kLinkLds];
    const OpvDivGroup& g = groups[blockIdx.x / per_group];
    const uint32_t n_frames = g.n_frames;
    for (uint32_t f = g.dec_from + blockIdx.x % per_group; f < n_frames; f += per_group) {
        const uint32_t slot = f % g.cap;
        link_one(g.payload + (size_t)slot * OPV_CODED, 0u, 0xFFFFFFFFu, g.scale[slot], g.metrics[slot], g.frames + (size_t)slot * OPV_FB,
                 (opv_link*)g.link + slot, s_bits);
    }
}
