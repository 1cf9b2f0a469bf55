"""CPU-only: csrc/opv_stream_rules.{h,cpp} - the rules that keep a stream's device buffers consistent (what compaction keeps and
its re-base, the runs of a ring, the launch shape of the table-driven kernels, the migration blob's checks) - compiled with g++
into a shared object (tests/stream_rules_probe.cpp gives it a C face) and called through ctypes; and that file's own
probe_blob_shift, the far-position shift of a blob that tests/test_gpu_far_positions.py relies on. Every check is exact."""
import ctypes
import struct
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "opv-cxx-demod_amd" / "csrc"
U64 = ctypes.c_uint64
U32 = ctypes.c_uint32


@pytest.fixture(scope="module")
def rules(tmp_path_factory):
    so = tmp_path_factory.mktemp("rules") / "librules.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-Wall", "-ffp-contract=off", "-shared", "-I", str(CSRC), "-o", str(so),
                    str(ROOT / "tests" / "stream_rules_probe.cpp"), str(CSRC / "opv_stream_rules.cpp")], check=True)
    L = ctypes.CDLL(str(so))
    L.probe_iq_keep.restype = U64
    L.probe_iq_keep.argtypes = [U64]
    L.probe_iq_rebase.argtypes = [U64, ctypes.POINTER(U64)]
    L.probe_ring_runs.argtypes = [U64, U64, U64, ctypes.POINTER(U64)]
    L.probe_table_launch.argtypes = [U32, U32, U32, U32, ctypes.POINTER(U32)]
    L.probe_parse_blob.restype = ctypes.c_char_p
    L.probe_parse_blob.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(U32)]
    L.probe_offset.restype = ctypes.c_long
    L.probe_offset.argtypes = [ctypes.c_char_p]
    L.probe_blob_payload_off.restype = U64
    L.probe_blob_magic.restype = U64
    return L


def keep_formula(origin):
    return ((origin - 16) & ~3) if origin >= 16 else 0


def test_iq_keep_is_the_formula_a_multiple_of_four_and_within_reach(rules):
    for origin in list(range(41)) + [2**31 - 1]:
        k = rules.probe_iq_keep(origin)
        assert k == keep_formula(origin), origin
        assert k % 4 == 0 and (k == 0 or k <= origin - 16), origin
    assert rules.probe_iq_keep(2**31 - 1) == 2**31 - 20 and rules.probe_iq_keep(19) == 0 and rules.probe_iq_keep(20) == 4


def test_rebase_keeps_absolute_indices_and_floors_last_round_avail(rules):
    for origin, n_avail, lra, base in ((86736, 200000, 173440, 0), (86720 * 3 + 5, 86720 * 3 + 900, 10, 4096), (16, 16, 16, 7), (40, 41, 0, 2**40)):
        keep = rules.probe_iq_keep(origin)
        v = (U64 * 5)(n_avail, lra, origin, n_avail, base)
        rules.probe_iq_rebase(keep, v)
        got_avail, got_lra, got_origin, got_st_avail, got_base = list(v)
        assert got_origin + got_base == origin + base                      # the absolute chunk origin is what it was
        assert got_avail == n_avail - keep and got_st_avail == n_avail - keep
        assert got_lra == max(lra - keep, 0)                               # (unsigned in C++: a wrap would be ~2^64)
        assert 16 <= got_origin < 20 or keep == 0


def test_ring_runs_against_a_numpy_ring(rules):
    out = (U64 * 3)()
    for cap in (1, 2, 5, 4096):
        ring = np.arange(cap, dtype=np.int64)
        for first in sorted({0, 1, cap - 1, cap, cap + 1, 2 * cap - 1, 7 * cap + cap // 2}):
            p0 = first % cap
            for n in sorted({0, 1, cap - p0, min(cap - p0 + 1, cap), cap}):
                rules.probe_ring_runs(first, n, cap, out)
                q0, run0, run1 = list(out)
                assert q0 == p0 and run0 + run1 == n and run0 <= cap - p0, (cap, first, n)
                got = np.concatenate([ring[q0:q0 + run0], ring[:run1]])
                assert np.array_equal(got, (first + np.arange(n)) % cap), (cap, first, n)


def parent_compact_shape(m, most):
    """opv_capi.hip's compact_streams before the rules moved (most in samples)"""
    slices = 1 if m >= 1024 else (1024 + m - 1) // m
    by_size = most // (256 * 4)
    if slices > by_size:
        slices = by_size if by_size else 1
    grid = m * slices
    if grid > 2048:
        grid = 2048
    return slices, grid


def parent_gather_shape(m, most, blocks):
    """opv_capi.hip's push_deferred before the rules moved (most in bytes)"""
    slices = 1 if m >= 1024 else (1024 + m - 1) // m
    by_size = most // (256 * 16)
    if slices > by_size:
        slices = by_size if by_size else 1
    grid = m * slices
    if grid > blocks:
        grid = blocks
    return slices, grid


def test_launch_shape_is_the_two_formulas_it_replaced(rules):
    out = (U32 * 2)()
    for m in (1, 2, 14, 1023, 1024, 5000):
        for unit, cap, parent in ((4, 2048, lambda mo: parent_compact_shape(m, mo)), (16, 32, lambda mo: parent_gather_shape(m, mo, 32)),
                                  (16, 7, lambda mo: parent_gather_shape(m, mo, 7))):
            for most in (0, 1, unit, 256 * unit, 1023 * unit, 1023 * 256 * unit, 347 * 1024):
                rules.probe_table_launch(m, most, unit, cap, out)
                slices, grid = list(out)
                assert (slices, grid) == parent(most), (m, unit, cap, most)
                assert 1 <= grid <= cap and slices >= 1


# ---- the migration blob -------------------------------------------------------------------------------------------------------
class Blob:
    """a valid two-stream blob with empty segments, built field by field at the offsets the library reports"""

    def __init__(self, L):
        self.L = L
        self.sz_h, self.sz_e = L.probe_offset(b"sizeof.header"), L.probe_offset(b"sizeof.entry")
        self.payload_off = L.probe_blob_payload_off(2)
        self.b = bytearray(self.payload_off + 1024)
        self.put("h.magic", L.probe_blob_magic(), "Q")
        for name, v in (("h.version", 1), ("h.sizeof_stream", L.probe_offset(b"sizeof.stream")), ("h.sizeof_header", self.sz_h),
                        ("h.sizeof_entry", self.sz_e), ("h.count", 2)):
            self.put(name, v, "I")
        self.put("h.total_bytes", len(self.b), "Q")
        self.put("h.payload_off", self.payload_off, "Q")
        self.put("h.payload_bytes", 1024, "Q")
        for i in range(2):
            self.put("e.off", 512 * i, "Q", i)
            self.put("e.len", 512, "Q", i)
            for k in range(8):
                self.put("e.seg_off", 16 * k, "Q", i, 8 * k)
        # stream 1: cursors that are not zero, consistent with empty segments
        for name, v in (("e.popped", 3), ("st.n_frames", 3), ("e.events_first", 5), ("e.events_popped", 5), ("st.n_events", 5),
                        ("e.chunks_first", 2), ("st.n_chunks", 2)):
            self.put(name, v, "I", 1)
        self.put("st.iq_base", 1000, "Q", 1)

    def at(self, name, entry=None, extra=0):
        off = self.L.probe_offset(name.encode())
        assert off >= 0, name
        return off + extra + (0 if name.startswith("h.") else self.sz_h + self.sz_e * entry)

    def put(self, name, v, fmt, entry=None, extra=0):
        struct.pack_into("<" + fmt, self.b, self.at(name, entry, extra), v)
        return self

    def copy(self):
        c = Blob.__new__(Blob)
        c.__dict__.update(self.__dict__)
        c.b = bytearray(self.b)
        return c


def why(L, data, with_entries=1):
    n = U32(0)
    return L.probe_parse_blob(bytes(data), len(data), with_entries, ctypes.byref(n)).decode(), n.value


def poked(blob, at, width):
    b = bytearray(blob)
    for i in range(at, at + width):
        b[i] ^= 0x5A
    return b


TRUNCATED = "stream blob: truncated"
SHORT = "stream blob: missing or shorter than its header"
OTHER_BUILD = "stream blob: written by another build of the library (format version / struct sizes differ)"
SEG_OUTSIDE = "stream blob: a segment lies outside its stream's payload"
CONTRADICT = "stream blob: a stream's indices contradict its segments"


def test_parse_blob_accepts_a_consistent_blob_and_refuses_each_mutation_with_its_text(rules):
    good = Blob(rules)
    assert why(rules, good.b) == ("", 2) and why(rules, good.b, 0) == ("", 2)
    assert why(rules, bytes(good.b) + b"\x00" * 99) == ("", 2)                   # (a buffer larger than the blob is fine)
    # the refusals test_refusals_leave_the_destination_usable makes on a device, here with their texts
    assert why(rules, good.b[:-100])[0] == TRUNCATED                             # truncated in the payload
    assert why(rules, good.b[:40])[0] == SHORT                                   # ... in the header
    assert why(rules, good.b[:good.sz_h + 100])[0] == TRUNCATED                  # ... in the directory
    assert why(rules, b"")[0] == SHORT
    assert why(rules, poked(good.b, 0, 8))[0] == "stream blob: wrong magic"
    assert why(rules, poked(good.b, 8, 4))[0] == OTHER_BUILD                     # format version
    assert why(rules, poked(good.b, 12, 4))[0] == OTHER_BUILD                    # sizeof(OpvStream)
    assert why(rules, poked(good.b, good.at("h.sizeof_header"), 4))[0] == OTHER_BUILD
    assert why(rules, poked(good.b, good.at("h.sizeof_entry"), 4))[0] == OTHER_BUILD
    # a directory that stops inside an entry, with total_bytes saying so: the count no longer fits
    cut = good.copy().put("h.total_bytes", good.sz_h + good.sz_e + 8, "Q")
    assert why(rules, cut.b)[0] == "stream blob: stream count does not fit the blob"
    assert why(rules, good.copy().put("h.count", 2**31, "I").b)[0] == "stream blob: stream count does not fit the blob"
    assert why(rules, good.copy().put("h.count", 1000, "I").b)[0] == "stream blob: stream count does not fit the blob"
    assert why(rules, good.copy().put("h.payload_off", good.payload_off + 8, "Q").b)[0] == "stream blob: payload offset / length out of range"
    assert why(rules, good.copy().put("e.off", 520, "Q", 1).b)[0] == "stream blob: a stream's payload lies outside the blob"
    assert why(rules, good.copy().put("e.len", 513, "Q", 1).b)[0] == "stream blob: a stream's payload lies outside the blob"
    # segments
    assert why(rules, good.copy().put("e.seg_off", 24, "Q", 0, 8).b)[0] == SEG_OUTSIDE          # not a multiple of 16
    assert why(rules, good.copy().put("e.seg_off", 528, "Q", 1, 8 * 7).b)[0] == SEG_OUTSIDE     # behind its entry
    assert why(rules, good.copy().put("e.seg_n", 129, "Q", 0, 0).put("st.n_avail", 129, "Q", 0).b)[0] == SEG_OUTSIDE   # 516 bytes of IQ in 512
    assert why(rules, good.copy().put("e.seg_n", 2**31, "Q", 0, 8 * 3).b)[0] == "stream blob: segment length out of range"
    assert why(rules, good.copy().put("e.seg_n", 2**63, "Q", 1, 8 * 6).b)[0] == "stream blob: segment length out of range"
    # indices: a soft tail of 25 symbols from an even index is taken, the same tail from an odd index is not
    def soft(first, n):
        return good.copy().put("st.n_soft", 101, "Q", 0).put("st.trk_next", 101, "Q", 0).put("st.cap_soft", 4096, "Q", 0).put("e.soft_first", first, "Q", 0).put("e.seg_n", n, "Q", 0, 8)
    assert why(rules, soft(76, 25).b) == ("", 2)
    assert why(rules, soft(75, 26).b)[0] == CONTRADICT                           # soft_first odd
    assert why(rules, soft(78, 23).b)[0] == CONTRADICT                           # ... behind what the tracker can still read
    assert why(rules, good.copy().put("e.popped", 2, "I", 1).b)[0] == CONTRADICT
    assert why(rules, good.copy().put("st.overflow", 1, "i", 0).b)[0] == CONTRADICT
    assert why(rules, good.copy().put("e.last_round_avail", 1, "Q", 0).b)[0] == CONTRADICT
    # without the directory (opv_blob_streams) only the header is judged
    assert why(rules, good.copy().put("e.popped", 2, "I", 1).b, 0) == ("", 2)


# ---- the far-position shift (tests/stream_rules_probe.cpp: probe_blob_shift) ---------------------------------------------------
SEGS = ["iq", "soft", "frec", "frames", "metrics", "fscale", "events", "chunks"]


def live_blob(L):
    """the two-stream blob above, grown to streams past symbol 24: a soft tail of 40 symbols, two unpopped frame records and three
    events per stream, one stream HUNTING and one LOCKED"""
    g = Blob(L)
    elem = {s: L.probe_offset(b"segelem.%d" % k) for k, s in enumerate(SEGS)}
    assert elem["frec"] == L.probe_offset(b"sizeof.frec") and elem["events"] == L.probe_offset(b"sizeof.event") and min(elem.values()) >= 4
    n = dict(iq=0, soft=40, frec=2, frames=2, metrics=2, fscale=2, events=3, chunks=0)
    off, length = {}, 0
    for s in SEGS:
        off[s] = length
        length += (n[s] * elem[s] + 15) & ~15
    g.b = g.b[:g.payload_off] + bytearray(2 * length)
    g.put("h.total_bytes", len(g.b), "Q").put("h.payload_bytes", 2 * length, "Q")
    g.rec = {}
    for i in range(2):
        g.put("e.off", length * i, "Q", i).put("e.len", length, "Q", i)
        for k, s in enumerate(SEGS):
            g.put("e.seg_off", off[s], "Q", i, 8 * k).put("e.seg_n", n[s], "Q", i, 8 * k)
        n_soft = 5000 + 2 * i
        for name, v in (("st.n_soft", n_soft), ("st.trk_next", n_soft), ("st.trk_anchor", 4990), ("st.cap_soft", 4096),
                        ("e.soft_first", n_soft - 40), ("st.total_samples", 200000), ("st.iq_base", 1000 * i)):
            g.put(name, v, "Q", i)
        g.put("st.trk_state", 2 * i, "i", i)
        for name, v in (("e.popped", 3 * i), ("st.n_frames", 3 * i + 2), ("e.events_first", 5 * i), ("e.events_popped", 5 * i),
                        ("st.n_events", 5 * i + 3), ("e.chunks_first", 2 * i), ("st.n_chunks", 2 * i)):
            g.put(name, v, "I", i)
        at = g.payload_off + length * i
        g.rec[i] = [at + off["frec"] + k * elem["frec"] + L.probe_offset(f.encode()) for k in range(2) for f in ("frec.payload_sym", "frec.release_sym")]
        g.rec[i] += [at + off["events"] + k * elem["events"] + L.probe_offset(b"event.sym_idx") for k in range(3)]
        for j, a in enumerate(g.rec[i]):
            struct.pack_into("<Q", g.b, a, 2800 + 1000 * j + i)
    return g


SYM_FIELDS = ["st.n_soft", "st.trk_anchor", "st.trk_next", "e.soft_first"]
SAMP_FIELDS = ["st.total_samples", "st.iq_base"]
KEPT_FIELDS = [("st.origin", "Q"), ("st.n_avail", "Q"), ("e.last_round_avail", "Q"), ("st.fo_sum", "d"), ("st.n_frames", "I"), ("st.n_events", "I"),
               ("st.n_chunks", "I"), ("e.popped", "I"), ("e.events_first", "I"), ("e.events_popped", "I"), ("e.chunks_first", "I")]


def shift(L, data, d_sym, d_samp):
    buf = (ctypes.c_char * len(data)).from_buffer_copy(bytes(data))
    rc = L.probe_blob_shift(buf, len(data), d_sym, d_samp)
    return rc, bytearray(buf.raw)


@pytest.mark.parametrize("d", [4, 2**31, 2**32 - 4, 2**40 + 8])
def test_blob_shift_moves_every_absolute_index_and_nothing_else(rules, d):
    rules.probe_blob_shift.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64, U64]
    g = live_blob(rules)
    assert why(rules, g.b) == ("", 2)
    d_samp = d + 12
    rc, out = shift(rules, g.b, d, d_samp)
    assert rc == 0 and why(rules, out) == ("", 2)
    q = lambda b, at: struct.unpack_from("<Q", b, at)[0]
    moved = set()
    for i in range(2):
        for fields, by in ((SYM_FIELDS, d), (SAMP_FIELDS, d_samp)):
            for f in fields:
                assert q(out, g.at(f, i)) == q(g.b, g.at(f, i)) + by, (f, i)
                moved.add(g.at(f, i))
        for a in g.rec[i]:                                                       # payload_sym, release_sym of each record; sym_idx of each event
            assert q(out, a) == q(g.b, a) + d, (i, a)
            moved.add(a)
        for f, fmt in KEPT_FIELDS:
            assert struct.unpack_from("<" + fmt, out, g.at(f, i)) == struct.unpack_from("<" + fmt, g.b, g.at(f, i)), (f, i)
    # every other byte of the blob is what it was
    same = bytearray(out)
    for a in moved:
        same[a:a + 8] = g.b[a:a + 8]
    assert same == g.b and len(moved) == 2 * (6 + 7)
    # a second shift adds up; a buffer longer than the blob keeps its tail
    rc, twice = shift(rules, out, 2**32, 4)
    assert rc == 0 and q(twice, g.at("st.n_soft", 1)) == 5002 + d + 2**32 and q(twice, g.at("st.iq_base", 1)) == 1000 + d_samp + 4
    rc, longer = shift(rules, bytes(g.b) + b"\xA5" * 40, d, d_samp)
    assert rc == 0 and longer[:len(out)] == out and longer[len(out):] == b"\xA5" * 40


def test_blob_shift_refusals_leave_the_bytes_untouched(rules):
    rules.probe_blob_shift.argtypes = [ctypes.c_void_p, ctypes.c_size_t, U64, U64]
    g = live_blob(rules)
    def low(n_soft, trk_next):                                                   # a blob that holds together, stream 1 short of symbol 24
        return g.copy().put("st.n_soft", n_soft, "Q", 1).put("st.trk_next", trk_next, "Q", 1).put("e.soft_first", 0, "Q", 1).put("e.seg_n", n_soft, "Q", 1, 8).b
    for data in (low(23, 23), low(30, 22), low(0, 0)):
        assert why(rules, data) == ("", 2)
    refused = [(g.b, 1, 0, 2), (g.b, 2, 0, 2), (g.b, 2**32 + 2, 0, 2), (g.b, 0, 3, 2), (g.b, 4, 6, 2), (g.b, 2**32, 2**32 + 1, 2),   # not multiples of 4
               (low(23, 23), 4, 4, 3), (low(30, 22), 2**32, 4, 3), (low(0, 0), 4, 4, 3),   # n_soft < 24, trk_next < 23
               (Blob(rules).b, 4, 4, 3),                                         # the synthetic blob above: n_soft = 0 in both streams
               (g.b[:-8], 4, 4, 1), (poked(g.b, 0, 8), 4, 4, 1),                 # does not pass parse_blob before the shift
               (g.copy().put("e.popped", 1, "I", 1).b, 4, 4, 1),
               (low(24, 23), 4, 4, 4)]                                           # ... or after it: 24 symbols behind symbol 23 + d do not reach back to d
    for data, d_sym, d_samp, code in refused:
        rc, out = shift(rules, data, d_sym, d_samp)
        assert rc == code and out == bytearray(data), (d_sym, d_samp, rc)
    assert shift(rules, low(24, 24), 4, 4)[0] == 0
