// opv_iq_format.h — the sample formats a typed push accepts (include/opv_demod.h: OPV_IQ_*, opv_push_iq_fmt and its kin) and THE rule
// that turns one component of each into the int16 the receiver runs on. Each function is written ONCE as a __host__ __device__
// function: k_push_convert (opv_push.hip) runs it on the device behind the link, opv_iq_convert (opv_iq_format.cpp) on the host with
// no device at all (tests/test_iq_formats_host.py, tests/san_iq_formats/), like the diversity rules (opv_div_rules.h). No rule lives
// anywhere else; tests/iq_format_model.py states it a third time in numpy and the tests compare with ==.
//
// The rule per component (I and Q alike), with an int16 result:
//   format  bytes / sample  source alignment  result
//   CS16    4               4                 identity
//   CS8     2               2                 x * 256              (-32768 .. 32512)
//   CU8     2               2                 (2 u - 255) * 128    (-32640 .. 32640)
//   CF32    8               4                 see below
// CS8:  a full-scale 8-bit capture is a full-scale 16-bit one, so out_shift and the offset search's power scaling mean what they
//       mean for int16.
// CU8:  the centre is 127.5, exactly, with no DC term.
// CF32: t = x * 32767.0f as ONE fp32 multiplication, round to nearest even; r = rint(t) with ties to even; the result is
//       clamp(r, -32767, 32767); NaN gives 0 and +-Inf gives +-32767. On the device the multiplication is __fmul_rn and the rounding
//       rintf: nothing here may be contracted or replaced by fast-math (the library is built with -ffp-contract=off).
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/opv_demod.h"   // OPV_IQ_CS16 .. OPV_IQ_CF32

#if defined(__HIPCC__)
#define OPV_IQ_HD __host__ __device__
#else
#define OPV_IQ_HD
#endif

// bytes of one (I, Q) sample; 0 for a format that does not exist
OPV_IQ_HD inline size_t opv_iq_bytes_of(int fmt) {
    return fmt == OPV_IQ_CS16 ? 4u : fmt == OPV_IQ_CS8 || fmt == OPV_IQ_CU8 ? 2u : fmt == OPV_IQ_CF32 ? 8u : 0u;
}
// what a source address must be a multiple of; 0 for a format that does not exist
OPV_IQ_HD inline size_t opv_iq_align_of(int fmt) {
    return fmt == OPV_IQ_CS16 || fmt == OPV_IQ_CF32 ? 4u : fmt == OPV_IQ_CS8 || fmt == OPV_IQ_CU8 ? 2u : 0u;
}

OPV_IQ_HD inline int16_t opv_iq_from_cs8(int8_t x) { return (int16_t)((int)x * 256); }
OPV_IQ_HD inline int16_t opv_iq_from_cu8(uint8_t u) { return (int16_t)((2 * (int)u - 255) * 128); }
OPV_IQ_HD inline int16_t opv_iq_from_cf32(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float t = __fmul_rn(x, 32767.0f);
#else
    const float t = x * 32767.0f;
#endif
    if (!(t == t)) return 0;                               // NaN
    float r = rintf(t);                                    // ties to even (the default rounding mode; v_rndne_f32 on the device)
    if (r > 32767.0f) r = 32767.0f;                        // (+-Inf included)
    if (r < -32767.0f) r = -32767.0f;
    return (int16_t)(int)r;
}

// one component of format kFmt at `p` (CS8, CU8 or CF32; CS16 is a copy and never comes here)
template <int kFmt>
OPV_IQ_HD inline int16_t opv_iq_component(const void* p, size_t i) {
    if (kFmt == OPV_IQ_CS8) return opv_iq_from_cs8(((const int8_t*)p)[i]);
    if (kFmt == OPV_IQ_CU8) return opv_iq_from_cu8(((const uint8_t*)p)[i]);
    return opv_iq_from_cf32(((const float*)p)[i]);
}
