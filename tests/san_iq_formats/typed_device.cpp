// typed_device.cpp - TEST INFRASTRUCTURE (tests/san_iq_formats/Makefile): the typed batch push for the sanitized opv-rx-bridge. The
// stand-in device of tests/san/fake_device.cpp knows int16 only; this file puts opv_push_iq_batch_fmt in front of its opv_push_iq,
// widening on the host by the product's own rule (csrc/opv_iq_format.cpp, sanitized as well), so that `opv-rx-bridge --format`
// - its reads, its 8-byte carry of a split sample - runs under ASan + UBSan without a GPU. Never linked into the product.
#include <cstdint>
#include <vector>

#include "../../include/opv_demod.h"

extern "C" int opv_push_iq_batch_fmt(opv_ctx* c, int fmt, int count, const int* streams, const void* const* samples, const size_t* n) {
    std::vector<int16_t> wide;
    for (int i = 0; i < count; ++i) {
        wide.resize(2 * n[i]);
        if (opv_iq_convert(fmt, samples[i], wide.data(), n[i]) < 0) return OPV_EINVAL;   // reads every byte the host says is there
        if (int r = opv_push_iq(c, streams[i], wide.data(), n[i])) return r;
    }
    return OPV_OK;
}
