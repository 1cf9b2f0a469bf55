"""The rule of the typed IQ pushes (include/opv_demod.h: OPV_IQ_*; csrc/opv_iq_format.h is the product's one definition), stated
a third time in numpy. One component (I and Q alike) of a block in the radio's format -> the int16 the receiver runs on:

    cs16  identity
    cs8   x * 256                 (-32768 .. 32512)
    cu8   (2 u - 255) * 128       (-32640 .. 32640): the centre is 127.5, exactly, with no DC term
    cf32  t = x * 32767.0f as ONE fp32 multiplication, round to nearest even; r = rint(t), ties to even;
          clamp(r, -32767, 32767); NaN gives 0, +-Inf gives +-32767

The tests compare the product with this by ==. Also here: the inputs the CPU and the GPU tests share (every value of the 8-bit
formats, the CF32 list of the issue), and `quantise`, an inverse used to make typed captures from int16 ones. Needs no device."""
import numpy as np

FORMATS = {"cs16": np.int16, "cs8": np.int8, "cu8": np.uint8, "cf32": np.float32}
CODES = {"cs16": 0, "cs8": 1, "cu8": 2, "cf32": 3}
SAMPLE_BYTES = {"cs16": 4, "cs8": 2, "cu8": 2, "cf32": 8}


def iq_format_model(fmt, block):
    """int16 array of the same length as the flat component array `block` (dtype FORMATS[fmt])"""
    a = np.asarray(block).reshape(-1)
    assert a.dtype == FORMATS[fmt], (fmt, a.dtype)
    if fmt == "cs16":
        return a.copy()
    if fmt == "cs8":
        return (a.astype(np.int32) * 256).astype(np.int16)
    if fmt == "cu8":
        return ((2 * a.astype(np.int32) - 255) * 128).astype(np.int16)
    with np.errstate(over="ignore", invalid="ignore"):
        t = a * np.float32(32767.0)                        # float32 x float32: one fp32 multiplication
        assert t.dtype == np.float32
        r = np.clip(np.rint(t), np.float32(-32767.0), np.float32(32767.0))
    return np.where(np.isnan(t), np.float32(0.0), r).astype(np.int16)


def quantise(fmt, iq16):
    """the block of `fmt` nearest to the int16 block: what a radio of that format would have delivered of the same signal"""
    v = np.asarray(iq16, np.int16).reshape(-1).astype(np.float64)
    if fmt == "cs16":
        return v.astype(np.int16)
    if fmt == "cs8":
        return np.clip(np.rint(v / 256.0), -128, 127).astype(np.int8)
    if fmt == "cu8":
        return np.clip(np.rint((v / 128.0 + 255.0) / 2.0), 0, 255).astype(np.uint8)
    return (v / 32767.0).astype(np.float32)


def cf32_special_values():
    """the CF32 values of the issue, in one float32 array of even length: +-0, the smallest denormal, +-1 and the floats next to
    them on both sides, the ties (k + 0.5) / 32767 as fp32 delivers them for k = 0, 1, 2, 16382, 16383 and their negatives, 1e30,
    -1e30, NaN, +-Inf, and 10^5 random values in [-1.5, 1.5]"""
    one = np.float32(1.0)
    inf = np.float32(np.inf)
    fixed = [np.float32(0.0), np.float32(-0.0), np.float32(1e-45), np.float32(-1e-45), one, -one,
             np.nextafter(one, inf), np.nextafter(one, -inf), np.nextafter(-one, inf), np.nextafter(-one, -inf)]
    for k in (0, 1, 2, 16382, 16383):
        tie = np.float32((k + 0.5) / 32767.0)
        fixed += [tie, -tie, np.nextafter(tie, inf), np.nextafter(tie, -inf)]
    fixed += [np.float32(1e30), np.float32(-1e30), np.float32(np.nan), inf, -inf, np.float32(0.5), np.float32(-0.5)]
    rnd = np.random.default_rng(20261021).uniform(-1.5, 1.5, 100000).astype(np.float32)
    out = np.concatenate([np.array(fixed, np.float32), rnd])
    return out if out.size % 2 == 0 else np.concatenate([out, np.zeros(1, np.float32)])


def every_byte_pair(fmt):
    """all 65 536 (I, Q) byte pairs of an 8-bit format as one block of 65 536 samples"""
    i, q = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    return np.stack([i.reshape(-1), q.reshape(-1)], axis=1).reshape(-1).astype(np.uint8).view(FORMATS[fmt])
