// iq_formats_probe.cpp - TEST INFRASTRUCTURE (tests/san_iq_formats/Makefile): the rule of the typed IQ pushes, csrc/opv_iq_format.h and
// its host entry opv_iq_convert, as a stand-alone program, so that it runs under ASan + UBSan without Python and without a device.
//   usage: iq_formats_probe <file of float32 values (an even count)>
// It prints, one line each: every value of cs8 and of cu8 through the header's functions; the file's values through
// opv_iq_convert(CF32); the answers of opv_iq_sample_bytes and of the refusals. Every buffer is a heap block of exactly the size the
// call may touch, and every call is repeated at every length 0 .. 17 and source offset the formats allow, so that a read or a write
// one element outside is the sanitizer's to report. tests/test_iq_formats_host.py compares the lines with tests/iq_format_model.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "opv_iq_format.h"

static int fails = 0;
#define EXPECT(cond)                                                        \
    do {                                                                    \
        if (!(cond)) { printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); ++fails; } \
    } while (0)

// n samples of `fmt` copied to a fresh block that starts `off` bytes behind a 16-byte boundary and ends where the samples end,
// converted into a fresh block of exactly n samples; the result must equal the header's functions applied one by one
template <int kFmt>
static void exact_blocks(const std::vector<uint8_t>& raw) {
    const size_t per = opv_iq_bytes_of(kFmt), align = opv_iq_align_of(kFmt);
    for (size_t n = 0; n <= 17; ++n)
        for (size_t off = 0; off < 16; off += align) {
            if (n * per > raw.size()) continue;
            uint8_t* block = (uint8_t*)malloc(off + n * per ? off + n * per : 1);   // (16-byte aligned; the samples end where it ends)
            uint8_t* src = block + off;
            memcpy(src, raw.data(), n * per);
            int16_t* out = (int16_t*)malloc(n ? n * 4 : 1);
            EXPECT(opv_iq_convert(kFmt, src, out, n) == OPV_OK);
            for (size_t i = 0; i < 2 * n; ++i) EXPECT(out[i] == opv_iq_component<kFmt>(src, i));
            free(out);
            free(block);
        }
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s <float32 file>\n", argv[0]); return 2; }
    printf("bytes %zu %zu %zu %zu %zu %zu\n", opv_iq_sample_bytes(OPV_IQ_CS16), opv_iq_sample_bytes(OPV_IQ_CS8), opv_iq_sample_bytes(OPV_IQ_CU8),
           opv_iq_sample_bytes(OPV_IQ_CF32), opv_iq_sample_bytes(4), opv_iq_sample_bytes(-1));
    // ---- every value of the 8-bit formats, through the header's functions and through the entry point
    std::vector<uint8_t> all(256);
    for (int v = 0; v < 256; ++v) all[v] = (uint8_t)v;
    std::vector<int16_t> out(256);
    printf("cs8");
    EXPECT(opv_iq_convert(OPV_IQ_CS8, all.data(), out.data(), 128) == OPV_OK);
    for (int v = 0; v < 256; ++v) { EXPECT(out[v] == opv_iq_from_cs8((int8_t)all[v])); printf(" %d", out[v]); }
    printf("\ncu8");
    EXPECT(opv_iq_convert(OPV_IQ_CU8, all.data(), out.data(), 128) == OPV_OK);
    for (int v = 0; v < 256; ++v) { EXPECT(out[v] == opv_iq_from_cu8(all[v])); printf(" %d", out[v]); }
    printf("\n");
    // ---- the file's floats
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    std::vector<float> x;
    float buf[4096];
    for (size_t got; (got = fread(buf, 4, 4096, f)) > 0;) x.insert(x.end(), buf, buf + got);
    fclose(f);
    if (x.size() % 2) { fprintf(stderr, "odd count of floats\n"); return 2; }
    std::vector<int16_t> y(x.size());
    EXPECT(opv_iq_convert(OPV_IQ_CF32, x.data(), y.data(), x.size() / 2) == OPV_OK);
    printf("cf32");
    for (size_t i = 0; i < y.size(); ++i) { EXPECT(y[i] == opv_iq_from_cf32(x[i])); printf(" %d", y[i]); }
    printf("\n");
    // ---- CS16 is a copy
    std::vector<int16_t> z(y.size());
    EXPECT(opv_iq_convert(OPV_IQ_CS16, y.data(), z.data(), y.size() / 2) == OPV_OK && z == y);
    // ---- blocks of exactly the size a call may touch
    std::vector<uint8_t> raw8(64), rawf(17 * 8);
    for (size_t i = 0; i < raw8.size(); ++i) raw8[i] = (uint8_t)(37 * i + 11);
    memcpy(rawf.data(), x.data(), x.size() * 4 < rawf.size() ? x.size() * 4 : rawf.size());
    exact_blocks<OPV_IQ_CS8>(raw8);
    exact_blocks<OPV_IQ_CU8>(raw8);
    exact_blocks<OPV_IQ_CF32>(rawf);
    // ---- refusals: a format that does not exist, null pointers, a pointer off its format's alignment; n = 0 asks for nothing
    alignas(16) char store[64] = {};
    int16_t o[16];
    printf("refusals %d %d %d %d %d %d %d %d\n", opv_iq_convert(4, store, o, 1), opv_iq_convert(-1, store, o, 1), opv_iq_convert(OPV_IQ_CS8, nullptr, o, 1),
           opv_iq_convert(OPV_IQ_CS8, store, nullptr, 1), opv_iq_convert(OPV_IQ_CF32, store + 2, o, 1), opv_iq_convert(OPV_IQ_CS8, store + 1, o, 1),
           opv_iq_convert(OPV_IQ_CS16, store + 2, o, 1), opv_iq_convert(OPV_IQ_CF32, nullptr, nullptr, 0));
    printf("fails %d\n", fails);
    return fails ? 1 : 0;
}
