"""CPU-only: the typed IQ pushes' host half (include/opv_demod.h: OPV_IQ_*, opv_push_iq_fmt and its kin). The header declares every
new name, the library and the binding export them, the ABI stays 7; the refusals that need no device; opv_iq_convert == the numpy
model (tests/iq_format_model.py) on every value of cs8 and cu8 and on the CF32 list (+-0, the smallest denormal, +-1 and their
neighbours, the ties of the rounding, 1e30, NaN, +-Inf, 10^5 random values); and the same rule as a stand-alone program under
ASan + UBSan (tests/san_iq_formats/), and `opv-rx-bridge --format` as the sanitized build of tests/san/. Nothing is loaded into
Python under a sanitizer."""
import ctypes as C
import os
import re
import socket
import subprocess

import numpy as np
import pytest

from amd_lib import ROOT
from fixtures_built import amd  # noqa: F401
from iq_format_model import CODES, FORMATS, SAMPLE_BYTES, cf32_special_values, every_byte_pair, iq_format_model, quantise

EINVAL = -1
NEW_NAMES = ["opv_push_iq_fmt", "opv_push_iq_batch_fmt", "opv_push_iq_batch_fmt_async", "opv_wb_push_fmt", "opv_wb_push_fmt_async",
             "opv_scan_push_fmt", "opv_convert_iq_device", "opv_iq_convert", "opv_iq_sample_bytes"]


def test_header_exports_and_abi(amd):
    header = (ROOT / "include" / "opv_demod.h").read_text()
    L = amd.lib()
    for name in NEW_NAMES:
        assert re.search(r"^(?:int|size_t) " + name + r"\(", header, re.M), f"{name} is not declared in the header"
        assert name in amd.EXPORTS and hasattr(L, name), name
    assert re.search(r"enum \{ OPV_IQ_CS16 = 0, OPV_IQ_CS8 = 1, OPV_IQ_CU8 = 2, OPV_IQ_CF32 = 3 \};", header)
    assert re.search(r"^#define OPV_ABI_VERSION 7\b", header, re.M) and L.opv_abi_version() == 7
    assert [L.opv_iq_sample_bytes(f) for f in (0, 1, 2, 3, 4, -1)] == [4, 2, 2, 8, 0, 0]
    assert {k: L.opv_iq_sample_bytes(v) for k, v in CODES.items()} == SAMPLE_BYTES
    assert {k: v[0] for k, v in amd.IQ_FORMATS.items()} == CODES and {k: v[1] for k, v in amd.IQ_FORMATS.items()} == FORMATS


def test_refusals_without_a_device(amd):
    L = amd.lib()
    buf = np.zeros(64, np.uint8)
    out = np.zeros(32, np.int16)
    assert buf.ctypes.data % 8 == 0
    src, dst = buf.ctypes.data, out.ctypes.data
    for bad in (4, -1, 1 << 20):
        assert L.opv_iq_convert(bad, src, dst, 4) == EINVAL
    for fmt in range(4):
        assert L.opv_iq_convert(fmt, None, dst, 4) == EINVAL and L.opv_iq_convert(fmt, src, None, 4) == EINVAL
        assert L.opv_iq_convert(fmt, src, dst, 4) == 0
    assert L.opv_iq_convert(CODES["cf32"], src + 2, dst, 4) == EINVAL       # a CF32 pointer 2 bytes off
    assert L.opv_iq_convert(CODES["cf32"], src + 4, dst, 4) == 0
    assert L.opv_iq_convert(CODES["cs8"], src + 1, dst, 4) == EINVAL and L.opv_iq_convert(CODES["cs8"], src + 2, dst, 4) == 0
    # the entry points that take an object refuse a null one, and a format that does not exist, before they touch a device
    one = C.c_size_t(4)
    ptr = C.c_void_p(src)
    sid = C.c_int(0)
    assert L.opv_push_iq_fmt(None, 0, 1, src, 4) == EINVAL
    assert L.opv_push_iq_batch_fmt(None, 1, 1, C.byref(sid), C.byref(ptr), C.byref(one)) == EINVAL
    assert L.opv_push_iq_batch_fmt_async(None, 1, 1, C.byref(sid), C.byref(ptr), C.byref(one)) == EINVAL
    assert L.opv_convert_iq_device(None, 1, src, dst, 4) == EINVAL
    for fmt in (1, 7):
        assert L.opv_wb_push_fmt(None, fmt, src, 4) == EINVAL and L.opv_wb_push_fmt_async(None, fmt, src, 4) == EINVAL
        assert L.opv_scan_push_fmt(None, fmt, src, 4) == EINVAL
    with pytest.raises(amd.OpvError):
        amd.iq_convert("cs12", buf)


@pytest.mark.parametrize("fmt", ["cs8", "cu8"])
def test_every_value_of_the_8_bit_formats(amd, fmt):
    x = np.arange(256, dtype=np.uint8).view(FORMATS[fmt])
    got, exp = amd.iq_convert(fmt, x), iq_format_model(fmt, x)
    assert got.dtype == np.int16 and np.array_equal(got, exp)
    lit = [int(v) * 256 for v in x] if fmt == "cs8" else [(2 * int(v) - 255) * 128 for v in x]      # the table's words, in python integers
    assert exp.tolist() == lit and (min(lit), max(lit)) == ((-32768, 32512) if fmt == "cs8" else (-32640, 32640))
    pairs = every_byte_pair(fmt)
    assert pairs.size == 2 * 65536 and np.array_equal(amd.iq_convert(fmt, pairs), iq_format_model(fmt, pairs))


def test_cf32_equals_the_model(amd):
    x = cf32_special_values()
    assert x.size >= 100000 and np.isnan(x).sum() == 1 and np.isinf(x).sum() == 2
    got, exp = amd.iq_convert("cf32", x), iq_format_model("cf32", x)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, (bad.size, x[bad[:5]], got[bad[:5]], exp[bad[:5]])
    # the model itself, against the rule's words in python's exact arithmetic: t rounded to fp32 once, then ties to even
    for v, e in zip(x[:64], exp[:64]):
        if np.isnan(v):
            assert e == 0
            continue
        t = float(np.float32(float(v) * 32767.0)) if np.isfinite(v) else float(v)     # (a double holds the exact product of two floats)
        assert e == max(-32767, min(32767, round(t) if np.isfinite(t) else (32767 if t > 0 else -32767))), (v, e)
    assert exp[np.isposinf(x)].tolist() == [32767] and exp[np.isneginf(x)].tolist() == [-32767]
    assert exp[x == np.float32(1e30)].tolist() == [32767] and exp[x == np.float32(-1e30)].tolist() == [-32767]
    ties = [np.float32((k + 0.5) / 32767.0) for k in (0, 1, 2, 16382, 16383)]
    assert {int(v) for v in iq_format_model("cf32", np.array(ties, np.float32))} <= set(range(0, 16385))


def test_cs16_is_the_identity_and_quantise_inverts_the_rule(amd):
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, 4096).astype(np.int16)
    assert np.array_equal(amd.iq_convert("cs16", x), x)
    for fmt in ("cs8", "cu8", "cf32"):
        q = quantise(fmt, x)
        assert q.dtype == FORMATS[fmt]
        back = iq_format_model(fmt, q).astype(np.int32)
        assert np.max(np.abs(back - x)) <= {"cs8": 255, "cu8": 128, "cf32": 1}[fmt]
        again = quantise(fmt, back.astype(np.int16))                    # a block of the format survives the round trip
        assert np.array_equal(iq_format_model(fmt, again), back.astype(np.int16))


def test_iq_format_rule_under_sanitizers(tmp_path):
    """tests/san_iq_formats/: csrc/opv_iq_format.cpp (and the header's functions) linked into a program with its own main, once
    with -fsanitize=address,undefined and once plain. It converts every 8-bit value, this module's CF32 list (read from a file) and
    heap blocks of exactly the size a call may touch at every short length and source offset, and answers the refusals. The
    sanitized build reports nothing, exits 0 and prints what the plain build prints; what it prints is the model's, by ==."""
    out_dir = tmp_path / "san_iq_formats"
    p = subprocess.run(["make", "-C", str(ROOT / "tests" / "san_iq_formats"), f"OUT={out_dir}"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    x = cf32_special_values()
    floats = tmp_path / "values.f32"
    x.tofile(floats)
    env = dict(ASAN_OPTIONS="exitcode=99:detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")
    outs = []
    for exe in ("iq_formats_san", "iq_formats_plain"):
        q = subprocess.run([str(out_dir / exe), str(floats)], capture_output=True, text=True, env=env, timeout=300)
        assert q.returncode == 0 and "Sanitizer" not in q.stderr and "runtime error" not in q.stderr, (exe, q.returncode, q.stdout[-500:], q.stderr[-3000:])
        outs.append(q.stdout.splitlines())
    assert outs[0] == outs[1]
    lines = {ln.split()[0]: ln.split()[1:] for ln in outs[0]}
    assert lines["bytes"] == ["4", "2", "2", "8", "0", "0"] and lines["fails"] == ["0"]
    every = np.arange(256, dtype=np.uint8)
    assert list(map(int, lines["cs8"])) == iq_format_model("cs8", every.view(np.int8)).tolist()
    assert list(map(int, lines["cu8"])) == iq_format_model("cu8", every).tolist()
    assert np.array_equal(np.array(lines["cf32"], np.int64), iq_format_model("cf32", x))
    assert lines["refusals"] == ["-1", "-1", "-1", "-1", "-1", "-1", "-1", "0"]


def _udp_listener():
    for port in range(43100 + os.getpid() % 2000, 60000, 59):
        s = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        try:
            s.bind(("127.0.0.1", port))
            s.setblocking(False)
            return port, s
        except OSError:
            s.close()
    raise RuntimeError("no free port")


@pytest.mark.parametrize("fmt", ["cu8", "cf32", "bad"])
def test_rx_bridge_format_under_asan(amd, oracle, iq10, fmt, tmp_path):
    """`opv-rx-bridge --format F -` (what `rtl_sdr - | opv-rx-bridge --format cu8 -` runs) under ASan + UBSan, against the stand-in
    device of tests/san/ with tests/san_iq_formats/typed_device.cpp in front of it for the typed batch push: stdin written in ragged
    pieces that split samples - 8-byte ones of cf32 too, the carry's new size - and closed in the middle of one. The datagrams out
    are the oracle's frames for the model-converted whole samples. A format that does not exist is refused with exit code 2 - and so
    is an existing one by the bridge of tests/san/, whose stand-in has no typed push: the bridge refers to it weakly and says so."""
    out_dir = tmp_path / "san_iq_formats"
    p = subprocess.run(["make", "-C", str(ROOT / "tests" / "san_iq_formats"), f"OUT={out_dir}", "bridge"], capture_output=True, text=True)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    exe = str(out_dir / "opv-rx-bridge-asan")
    env = dict(os.environ, ASAN_OPTIONS="exitcode=99:detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="exitcode=99:halt_on_error=1:print_stacktrace=1")
    if fmt == "bad":
        for args in (["--format", "cs12", "-"], ["--format", "", "-"]):
            q = subprocess.run([exe] + args, input=b"", capture_output=True, env=env, timeout=60)
            assert q.returncode == 2 and b"--format takes" in q.stderr, (args, q.stderr[-300:])
        p = subprocess.run(["make", "-C", str(ROOT / "opv-cxx-demod_amd"), "-j8", "san"], capture_output=True, text=True)
        assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
        plain = str(ROOT / "opv-cxx-demod_amd" / "build" / "san" / "asan" / "opv-rx-bridge")
        q = subprocess.run([plain, "--format", "cu8", "-"], input=b"\x80" * 64, capture_output=True, env=env, timeout=60)
        assert q.returncode == 2 and b"no typed pushes" in q.stderr and b"Sanitizer" not in q.stderr, q.stderr[-500:]
        q = subprocess.run([plain, "-q", "--format", "cs16", "-"], input=b"\x00" * 1001, capture_output=True, env=env, timeout=60)
        assert q.returncode == 1 and b"Sanitizer" not in q.stderr, q.stderr[-500:]       # int16 by name: as without the flag (no frames: 1)
        return
    per = SAMPLE_BYTES[fmt]
    typed = quantise(fmt, iq10[: 2 * (4 * 86720 + 4321)])
    raw = typed.tobytes()
    cut = len(raw) - (per - 1)                                # stdin ends inside a sample
    port, sock = _udp_listener()
    b = subprocess.Popen([exe, "-q", "-P", str(port), "--format", fmt, "-"], stdin=subprocess.PIPE, stderr=subprocess.PIPE, env=env)
    at = k = 0
    sizes = [16384, 1, 3, 70001, 5, 7]
    while at < cut:
        n = min(sizes[k % len(sizes)], cut - at)
        b.stdin.write(raw[at:at + n])
        b.stdin.flush()
        at += n
        k += 1
    b.stdin.close()
    err = b.stderr.read().decode(errors="replace")
    rc = b.wait(timeout=600)
    assert rc != 99 and "Sanitizer" not in err and "runtime error" not in err, err[-4000:]
    assert rc == 0, err[-2000:]
    got = []
    while True:
        try:
            got.append(sock.recv(2048))
        except BlockingIOError:
            break
    sock.close()
    whole = cut // per
    exp = oracle.receive(iq_format_model(fmt, typed[: 2 * whole]), streaming=True, want_soft=False)["frames"]
    assert len(exp) >= 3 and all(len(g) == 134 for g in got)
    assert np.array_equal(np.frombuffer(b"".join(got), np.uint8).reshape(-1, 134), exp), (len(got), len(exp))
