// opv_iq_format.cpp — the host-only entries of the typed pushes: the rule of opv_iq_format.h over a block in host memory, no device
// involved (tests/test_iq_formats_host.py holds it to tests/iq_format_model.py; tests/san_iq_formats/ runs it under sanitizers).
// Plain C++, like opv_div_rules.cpp.
#include "opv_iq_format.h"

#include <string.h>

extern "C" size_t opv_iq_sample_bytes(int fmt) { return opv_iq_bytes_of(fmt); }

template <int kFmt>
static void convert_block(const void* in, int16_t* out, size_t n_samples) {
    for (size_t i = 0; i < 2 * n_samples; ++i) out[i] = opv_iq_component<kFmt>(in, i);
}

extern "C" int opv_iq_convert(int fmt, const void* in, int16_t* out, size_t n_samples) {
    const size_t align = opv_iq_align_of(fmt);
    if (!align) return OPV_EINVAL;
    if (n_samples == 0) return OPV_OK;
    if (!in || !out) return OPV_EINVAL;
    if (((uintptr_t)in & (align - 1)) != 0 || ((uintptr_t)out & 1u) != 0) return OPV_EINVAL;
    switch (fmt) {
    case OPV_IQ_CS16: memmove(out, in, n_samples * 4); break;
    case OPV_IQ_CS8: convert_block<OPV_IQ_CS8>(in, out, n_samples); break;
    case OPV_IQ_CU8: convert_block<OPV_IQ_CU8>(in, out, n_samples); break;
    default: convert_block<OPV_IQ_CF32>(in, out, n_samples); break;
    }
    return OPV_OK;
}
