// frame_code_probe.cpp — test support for csrc/opv_frame_code.h (plain C++, no GPU): a C face for ctypes
// (tests/test_frame_code_host.py) over the table, the address map, the two polynomials and the quantiser, as g++ compiles them.
#include <math.h>
#include <stdint.h>

#include "opv_frame_code.h"

extern "C" {
void probe_lfsr_table(uint8_t out[OPV_FB]) {
    constexpr OpvLfsrTable t = opv_make_lfsr();
    for (int i = 0; i < OPV_FB; ++i) out[i] = t.b[i];
}
uint32_t probe_interleave_addr(uint32_t i) { return opv_interleave_addr(i); }
// randomise -> encode (last byte first, MSB first; reg = (in << 6) | sr) -> interleave: the coded bits in encoder order and on air
void probe_encode_frame(const uint8_t frame[OPV_FB], uint8_t coded[OPV_CODED], uint8_t on_air[OPV_CODED]) {
    constexpr OpvLfsrTable t = opv_make_lfsr();
    unsigned sr = 0;
    uint32_t o = 0;
    for (int byte = OPV_FB - 1; byte >= 0; --byte)
        for (int bit = 7; bit >= 0; --bit) {
            const unsigned in = ((unsigned)(frame[byte] ^ t.b[byte]) >> bit) & 1u, reg = (in << 6) | sr;
            coded[o] = (uint8_t)opv_code_g1(reg);
            coded[o + 1] = (uint8_t)opv_code_g2(reg);
            on_air[opv_interleave_addr(o)] = coded[o];
            on_air[opv_interleave_addr(o + 1)] = coded[o + 1];
            o += 2;
            sr = ((sr << 1) | in) & 0x3Fu;
        }
}
// the decoder's front half on one payload: scale = mean |soft| summed in index order, then opv_quantise3 of every value in
// payload order. Returns 0 for a payload the decoder drops (scale < 1e-10; q untouched), else 1.
int probe_quantise_payload(const double soft[OPV_CODED], int32_t q[OPV_CODED]) {
    double sum = 0.0;
    for (int i = 0; i < OPV_CODED; ++i) sum += fabs(soft[i]);
    const double scale = sum / (double)OPV_CODED;
    if (scale < 1e-10) return 0;
    const double inv = -3.5 / scale;
    for (int i = 0; i < OPV_CODED; ++i) q[i] = opv_quantise3(soft[i], scale, inv);
    return 1;
}
}
