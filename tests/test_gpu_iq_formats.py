"""GPU: typed IQ pushes (include/opv_demod.h: OPV_IQ_*; csrc/opv_push.hip: k_push_convert), int16 for int16. A block of cs8, cu8
or cf32 crosses PCIe in its own format and is widened on the device; what opv_tap_iq then returns must be tests/iq_format_model.py
of what was pushed, == on every int16, whichever route the block took (read in place from pinned memory, or copied raw into the
context's device stage: pageable memory, OPV_PUSH_NO_GATHER), at every alignment of source and destination and every length at
which the kernel cuts head, body and tail differently. tests/test_gpu_push_bytes.py is the pattern (its int16 kernel is untouched).

Then the same through the wideband door and the scan (== tests/wideband_models.py / tests/scan_model.py on the model-converted
int16), opv_convert_iq_device, a noisy capture end to end against the oracle, and the refusals on a live context.

Known limit, as in test_gpu_push_bytes.py: opv_tap_iq cannot see past a stream's n_avail, so a write BEHIND the last block of a
stream is not observable here; a write into another stream's buffer or short of a block's end is."""

import numpy as np
import pytest

from fixtures import amd, torch_dev  # noqa: F401
from iq_format_model import CODES, FORMATS, SAMPLE_BYTES, cf32_special_values, every_byte_pair, iq_format_model, quantise
from oracle_lib import Oracle, impair
from scan_model import hann_window, scan_blocks, scan_model
from stream_checks import check_stream
from stream_runs import code_raised_by, collect, state_tuple
from wideband_models import halved_taps, per_phase_taps, wb_model, wb_model_inc, wbr_model, wbr_model_inc, wbr_outputs

pytestmark = pytest.mark.gpu

EINVAL, ECAPACITY = -1, -4
TYPED = ["cs8", "cu8", "cf32"]
LENGTHS = [1, 2, 3, 7, 8, 9, 15, 16, 17, 1023, 1025, 4099]     # samples: below, at and beside one 16-byte group of cs8 / cu8 (8 samples) and of
                                                                # cf32 (2), two groups, 256 lanes x 4 / x 16


def random_block(rng, fmt, n_components):
    """components of `fmt` that reach every value of the 8-bit formats and both sides of the cf32 clamp, its ties included"""
    if fmt == "cf32":
        x = rng.uniform(-1.2, 1.2, n_components).astype(np.float32)
        k = rng.integers(-32768, 32768, n_components // 4)
        x[: k.size] = ((k + 0.5) / 32767.0).astype(np.float32)
        return rng.permutation(x)
    return rng.integers(0, 256, n_components).astype(np.uint8).view(FORMATS[fmt])


class PinnedPool:
    """one pinned torch buffer of random components of `fmt`; take(n, off_bytes) -> a view of n samples that starts off_bytes behind
    a 16-byte boundary"""

    def __init__(self, rng, fmt, n_bytes):
        import torch
        self.fmt, self.per = fmt, SAMPLE_BYTES[fmt]
        self.t = torch.empty(n_bytes, dtype=torch.uint8).pin_memory()
        self.a = self.t.numpy()
        self.a[:] = random_block(rng, fmt, n_bytes // FORMATS[fmt]().itemsize).view(np.uint8)
        assert self.a.ctypes.data % 16 == 0
        self.at = 0

    def take(self, n, off_bytes=0):
        lo = self.at + off_bytes
        v = self.a[lo: lo + n * self.per]
        assert v.size == n * self.per, "pool exhausted"
        assert v.ctypes.data % 16 == off_bytes
        self.at = (lo + n * self.per + 15) // 16 * 16
        return v.view(FORMATS[self.fmt])


def source_offsets(fmt):
    """bytes behind a 16-byte boundary: 0 .. 7 source samples of cs8 / cu8; 0 .. 1 source samples of cf32, and both 4 bytes off"""
    return [0, 8, 4, 12] if fmt == "cf32" else [2 * k for k in range(8)]


def assert_streams_hold(d, expected, tag):
    for k, parts in enumerate(expected):
        want = np.concatenate(parts) if parts else np.zeros(0, np.int16)
        got = d.iq(k)
        assert got.size == want.size, f"{tag}: stream {k} holds {got.size // 2} samples, pushed {want.size // 2}"
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{tag}: stream {k}: {bad.size} int16 differ, the first at {bad[0]} of {want.size}: {got[bad[0]]} vs {want[bad[0]]}"


def push(d, ids, blocks, mode, fmt):
    if mode == "async":
        d.push_batch(ids, blocks, wait=False, fmt=fmt)
        d.push_wait()
    else:
        d.push_batch(ids, blocks, fmt=fmt)


@pytest.mark.parametrize("mode", ["gather", "async", "copies", "pageable"])
@pytest.mark.parametrize("fmt", TYPED)
def test_alignment_matrix(amd, monkeypatch, fmt, mode):
    """16 streams in ONE batch. Stream k's destination starts k // 4 samples into a quad (a first int16 opv_push_iq of 0 .. 3
    samples - which also proves that formats mix within one stream); its source starts offs[(k + 4 batch) % len(offs)] bytes behind
    a 16-byte boundary, offs = 0 .. 7 source samples of cs8 / cu8 (a batch holds every offset twice, at two destination offsets;
    the second batch, behind the first, and the lengths' residues mod 4 bring the other pairs), or 0, 8, 4, 12 bytes of cf32 (each
    batch: all 16 pairs). Twice per length, for every length of LENGTHS. Through the table (pinned blocks read in place), through opv_push_iq_batch_fmt_async +
    opv_push_wait, through the stage with OPV_PUSH_NO_GATHER set, and from pageable memory."""
    if mode == "copies":
        monkeypatch.setenv("OPV_PUSH_NO_GATHER", "1")
    rng = np.random.default_rng(20261021)
    offs = source_offsets(fmt)
    pool = PinnedPool(rng, fmt, len(LENGTHS) * 2 * 16 * (max(LENGTHS) * SAMPLE_BYTES[fmt] + 48))
    for L in LENGTHS:
        d = amd.Demod(16, max_samples=2 * max(LENGTHS) + 64, streaming=True)
        try:
            expected = [[] for _ in range(16)]
            for k in range(16):
                if k // 4:
                    head = rng.integers(-32768, 32768, 2 * (k // 4)).astype(np.int16)
                    d.push(k, head)
                    expected[k].append(head)
            for batch in range(2):
                blocks = [pool.take(L, offs[(k + 4 * batch) % len(offs)]) for k in range(16)]
                if mode == "pageable":
                    blocks = [b.copy() for b in blocks]
                push(d, list(range(16)), blocks, mode, fmt)
                for k in range(16):
                    expected[k].append(iq_format_model(fmt, blocks[k]))
                assert_streams_hold(d, expected, f"{fmt}, {mode}, {L} samples, batch {batch}")
        finally:
            d.close()


@pytest.mark.parametrize("blocks_env", [None, "1", "7"])
@pytest.mark.parametrize("fmt", ["cs8", "cf32"])
def test_slicing_with_a_large_and_a_tiny_pair(amd, monkeypatch, fmt, blocks_env):
    """Two streams, 86 723 samples beside ONE sample: table_launch cuts each pair into slices by the large block's 16-byte groups
    (cs8: 173 446 bytes -> 42 slices; cf32: 693 784 bytes -> 169), so the small pair's slices are empty and the work items exceed the
    grid of 32 blocks - and of 1 and 7 (OPV_PUSH_GATHER_BLOCKS). Second batch: the streams swap roles, the large block lands one
    sample into a quad and starts one source sample behind a 16-byte boundary (a head of 7 samples / of 1)."""
    if blocks_env:
        monkeypatch.setenv("OPV_PUSH_GATHER_BLOCKS", blocks_env)
    rng = np.random.default_rng(7)
    big, per = 86723, SAMPLE_BYTES[fmt]
    pool = PinnedPool(rng, fmt, 2 * (big + 16) * per + 256)
    d = amd.Demod(2, max_samples=2 * big + 64, streaming=True)
    try:
        expected = [[], []]
        for batch, (n0, n1) in enumerate([(big, 1), (1, big)]):
            blocks = [pool.take(n0, per * batch), pool.take(n1, per * batch)]
            d.push_batch([0, 1], blocks, fmt=fmt)
            expected[0].append(iq_format_model(fmt, blocks[0]))
            expected[1].append(iq_format_model(fmt, blocks[1]))
            assert_streams_hold(d, expected, f"{fmt}, blocks {blocks_env}, batch {batch}")
    finally:
        d.close()


def test_more_pairs_than_the_grid(amd):
    """1030 streams, one cu8 block of 1 + k % 61 samples each in one batch: one slice per pair, and the grid's 32 blocks stride over
    1030 work items; then a second batch behind it (every destination offset, every source offset)"""
    rng = np.random.default_rng(11)
    S = 1030
    pool = PinnedPool(rng, "cu8", 2 * S * (2 * 61 + 48))
    d = amd.Demod(S, max_samples=4096, streaming=True)
    try:
        expected = [[] for _ in range(S)]
        for batch in range(2):
            blocks = [pool.take(1 + k % 61, 2 * ((k // 61) % 8)) for k in range(S)]
            d.push_batch(list(range(S)), blocks, fmt="cu8")
            for k in range(S):
                expected[k].append(iq_format_model("cu8", blocks[k]))
            assert_streams_hold(d, expected, f"1030 pairs, batch {batch}")
    finally:
        d.close()


@pytest.mark.parametrize("fmt", TYPED)
def test_every_value(amd, fmt):
    """all 65 536 (I, Q) byte pairs of cs8 / cu8, and the CPU test's cf32 list (+-0, the smallest denormal, +-1 and their neighbours,
    the ties, 1e30, NaN, +-Inf, 10^5 random values), each in ONE opv_push_iq_fmt from pinned memory (a table of one, read in place)
    and in one from pageable memory (through the stage)"""
    import torch
    x = cf32_special_values() if fmt == "cf32" else every_byte_pair(fmt)
    exp = iq_format_model(fmt, x)
    pinned_t = torch.from_numpy(x.copy()).pin_memory()
    d = amd.Demod(2, max_samples=x.size // 2 + 64, streaming=True)
    try:
        d.push(0, pinned_t.numpy(), fmt=fmt)
        d.push(1, x.copy(), fmt=fmt)
        assert_streams_hold(d, [[exp], [exp]], f"every value of {fmt}")
    finally:
        d.close()


@pytest.mark.parametrize("fmt", TYPED)
def test_convert_iq_device_equals_the_model(amd, torch_dev, fmt):
    """opv_convert_iq_device on 4099 samples at every source offset of the alignment matrix, into an output 0 .. 3 samples behind a
    16-byte boundary: == the model, and the int16 on either side of the output keep their canary"""
    torch, dev = torch_dev
    rng = np.random.default_rng(17)
    n, per = 4099, SAMPLE_BYTES[fmt]
    d = amd.Demod(1, max_samples=4096, streaming=True)
    try:
        for j, off in enumerate(source_offsets(fmt)):
            x = random_block(rng, fmt, 2 * n)
            raw = np.zeros(16 + n * per, np.uint8)
            raw[off: off + n * per] = x.view(np.uint8)
            src = torch.from_numpy(raw).to(dev)
            out = torch.full((2 * n + 16,), 12345, dtype=torch.int16, device=dev)
            torch.cuda.synchronize()
            assert src.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0
            dst_off = j % 4
            d.convert_device(fmt, src.data_ptr() + off, out.data_ptr() + 4 * dst_off, n)
            d.sync()
            got = out.cpu().numpy()
            assert np.array_equal(got[2 * dst_off: 2 * dst_off + 2 * n], iq_format_model(fmt, x)), (fmt, off)
            assert np.all(got[: 2 * dst_off] == 12345) and np.all(got[2 * dst_off + 2 * n:] == 12345), (fmt, off)
        # cs16 is a copy; a misaligned input and a bad format are refused
        y = torch.from_numpy(rng.integers(-32768, 32768, 2 * n).astype(np.int16)).to(dev)
        out = torch.zeros(2 * n, dtype=torch.int16, device=dev)
        torch.cuda.synchronize()
        d.convert_device("cs16", y.data_ptr(), out.data_ptr(), n)
        d.sync()
        assert torch.equal(out, y)
        L = amd.lib()
        assert L.opv_convert_iq_device(d.h, 9, y.data_ptr(), out.data_ptr(), n) == EINVAL
        assert L.opv_convert_iq_device(d.h, CODES["cf32"], y.data_ptr() + 2, out.data_ptr(), 8) == EINVAL
        assert L.opv_convert_iq_device(d.h, CODES["cs8"], y.data_ptr(), out.data_ptr() + 2, 8) == EINVAL
    finally:
        d.close()


# ------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def capture(amd):
    """a 4-frame BERT capture, noisy (16 dB), at an amplitude that leaves an 8-bit radio about 5 bits of signal"""
    ora = Oracle()
    return impair(ora.modulate(ora.bert_frames(4)), amp=8000.0, f0_hz=150.0, ebn0_db=16.0, seed=3)


@pytest.mark.parametrize("fmt", TYPED)
def test_end_to_end_against_the_oracle(amd, capture, fmt):
    """the capture quantised on the host to the format and pushed typed in odd pieces (16 384 samples, with a 1-sample and a 7-sample
    piece among them, pinned and pageable in turn): the stream's IQ == the model, and frames, metas, events and opv_stream_state are
    those of the ORACLE run on the model-converted int16 (tests/stream_checks.py: check_stream, edge_ties == 0)"""
    import torch
    q = quantise(fmt, capture)
    n = q.size // 2
    model = iq_format_model(fmt, q)
    exp = Oracle().receive(model, streaming=True)
    assert len(exp["frames"]) == 4, "the plan's capture decodes on the oracle"
    pinned = torch.from_numpy(q.copy()).pin_memory().numpy()
    cuts, at, j = [0], 0, 0
    while at < n:
        at = min(n, at + (1 if j == 1 else 7 if j == 3 else 16384))
        cuts.append(at)
        j += 1
    d = amd.Demod(1, max_samples=n + 64, streaming=True)
    try:
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            piece = pinned[2 * lo: 2 * hi] if j % 2 == 0 else q[2 * lo: 2 * hi].copy()
            d.push(0, piece, fmt=fmt)
        assert np.array_equal(d.iq(0), model)
        d.flush(0)
        d.process()
        d.sync()
        got = collect(d, 0)
        assert got["state"].stalled == 0
        check_stream(amd, got, exp, f"typed {fmt}")
    finally:
        d.close()


# ------------------------------------------------------------------ the wideband door and the scan
def typed_sources(q):
    import torch
    t = torch.from_numpy(q.copy()).pin_memory()
    return {"pinned": t.numpy(), "pageable": q.copy(), "_keep": t}


@pytest.mark.parametrize("where", ["pinned", "pageable"])
@pytest.mark.parametrize("fmt", ["cs8", "cf32"])
def test_wideband_doors_equal_their_models(amd, fmt, where):
    """an integer door (D = 2, K = 2, 33 taps) and a rational one (down / up = 3 / 2, 9 taps, the pair of
    test_gpu_wideband_rational.py's refusal case) fed the same typed capture in three pieces, the second asynchronously: every fed
    stream's opv_tap_iq == tests/wideband_models.py on the model-converted int16"""
    rng = np.random.default_rng(23)
    N = 3 * 1201 + 2
    q = random_block(rng, fmt, 2 * N)
    if fmt == "cf32":
        q = np.where(np.isfinite(q), q, np.float32(0.25)).astype(np.float32)
    wide = iq_format_model(fmt, q)
    T = amd.wb_lo_table()
    D, S = 2, 20
    centres = [400000.0, -650000.0]
    taps = halved_taps(rng, 33)
    exp_int = wb_model(T, wide, D, wb_model_inc(D, centres), taps, S)
    M, U, Sr = 3, 2, 17
    rtaps = per_phase_taps(rng, 9, U, 1 << 17)
    exp_rat = wbr_model(T, wide, M, U, wbr_model_inc(M, U, centres), rtaps, Sr)
    assert exp_int.shape == (2, 2 * ((N + 1) // 2)) and exp_rat.shape == (2, 2 * wbr_outputs(M, U, N))
    src = typed_sources(q)[where]
    d = amd.Demod(4, max_samples=N + 64, streaming=True)
    a = amd.Wideband(d, D, [0, 1], centres, taps, S)
    b = amd.Wideband.rational(d, M, U, [2, 3], centres, rtaps, Sr)
    try:
        cuts = [0, 1201, 1201 + 7, N]
        for j, (lo, hi) in enumerate(zip(cuts, cuts[1:])):
            for wb in (a, b):
                if j == 1:
                    wb.push_async(src[2 * lo: 2 * hi], fmt=fmt)
                else:
                    wb.push(src[2 * lo: 2 * hi], fmt=fmt)
            d.push_wait()
        for k in range(2):
            assert np.array_equal(d.iq(k), exp_int[k]), (fmt, where, "integer", k)
            assert np.array_equal(d.iq(2 + k), exp_rat[k]), (fmt, where, "rational", k)
        # a format that does not exist and a misaligned block are refused, and change nothing
        L = amd.lib()
        before = [d.iq(k).tobytes() for k in range(4)]
        buf = np.zeros(64, np.float32)
        assert L.opv_wb_push_fmt(a.h, 9, buf.ctypes.data, 4) == EINVAL and L.opv_wb_push_fmt(b.h, CODES["cf32"], buf.ctypes.data + 2, 4) == EINVAL
        assert L.opv_wb_push_fmt_async(a.h, CODES["cs8"], buf.ctypes.data + 1, 4) == EINVAL
        assert before == [d.iq(k).tobytes() for k in range(4)]
    finally:
        a.close()
        b.close()
        d.close()


@pytest.mark.parametrize("where", ["pinned", "pageable"])
@pytest.mark.parametrize("fmt", ["cs8", "cf32"])
def test_scan_row_equals_its_model(amd, fmt, where):
    """a Scan with 8 probes and one block, fed a typed capture in three pieces: its row == tests/scan_model.py on the model-converted int16"""
    rng = np.random.default_rng(29)
    P, Lw, H, A, S = 8, 64, 32, 4, 12
    N = (A - 1) * H + Lw + 5
    q = random_block(rng, fmt, 2 * N)
    wide = iq_format_model(fmt, q)
    window = hann_window(Lw)
    probes = list(np.linspace(-3e6, 3e6, P))
    exp = scan_model(amd.wb_lo_table(), wide, wbr_model_inc(4, 1, probes), window, H, A, S, 0)
    assert exp.shape == (1, P) == (scan_blocks(Lw, H, A, N), P) and exp.max() > 0
    src = typed_sources(q)[where]
    d = amd.Demod(1, max_samples=1 << 12, streaming=True)
    sc = amd.Scan(d, 4, 1, probes, window, H, A, S, ring_blocks=1)
    try:
        cuts = [0, 61, 62, N]
        for lo, hi in zip(cuts, cuts[1:]):
            sc.push(src[2 * lo: 2 * hi], fmt=fmt)
        rows, first = sc.pop()
        assert first == 0 and np.array_equal(rows, exp), (fmt, where)
        L = amd.lib()
        assert L.opv_scan_push_fmt(sc.h, 9, src.ctypes.data, 4) == EINVAL
        assert L.opv_scan_push_fmt(sc.h, CODES["cf32"], src.ctypes.data + 2, 4) == EINVAL
    finally:
        sc.close()
        d.close()


# ------------------------------------------------------------------ refusals
def test_refusals_on_a_live_context_change_nothing(amd):
    """a bad format, a misaligned cf32 source, and OPV_ECAPACITY - after which opv_get_state and opv_tap_iq show the stream unchanged;
    in a batch, the streams before the refused block have been pushed, as with int16"""
    rng = np.random.default_rng(31)
    L = amd.lib()
    d = amd.Demod(3, max_samples=64, streaming=True)
    try:
        held = rng.integers(-32768, 32768, 2 * 60).astype(np.int16)
        d.push(1, held)
        x = random_block(rng, "cf32", 2 * 16)
        b8 = random_block(rng, "cs8", 2 * 16)

        before = state_tuple(d.state(1))

        def unchanged():
            return state_tuple(d.state(1)) == before and np.array_equal(d.iq(1), held) and d.iq(0).size == 0

        assert L.opv_push_iq_fmt(d.h, 1, 9, x.ctypes.data, 2) == EINVAL and L.opv_push_iq_fmt(d.h, 1, -1, x.ctypes.data, 2) == EINVAL
        assert unchanged()
        assert L.opv_push_iq_fmt(d.h, 1, CODES["cf32"], x.ctypes.data + 2, 2) == EINVAL and unchanged()
        assert L.opv_push_iq_fmt(d.h, 1, CODES["cu8"], b8.ctypes.data + 1, 2) == EINVAL and unchanged()
        assert code_raised_by(amd, lambda: d.push(1, x[: 2 * 5], fmt="cf32")) == ECAPACITY and unchanged()
        assert code_raised_by(amd, lambda: d.push(1, b8[: 2 * 5], fmt="cs8")) == ECAPACITY and unchanged()
        assert L.opv_push_iq_fmt(d.h, 5, CODES["cs8"], b8.ctypes.data, 2) == EINVAL and unchanged()
        # a batch: stream 0 is pushed, stream 1 refuses, stream 2 is not reached
        assert code_raised_by(amd, lambda: d.push_batch([0, 1, 2], [b8[:8], b8[: 2 * 5], b8[:8]], fmt="cs8")) == ECAPACITY
        assert np.array_equal(d.iq(0), iq_format_model("cs8", b8[:8])) and np.array_equal(d.iq(1), held) and d.iq(2).size == 0
        d.push(1, x[: 2 * 4], fmt="cf32")                                    # what fits is taken
        assert np.array_equal(d.iq(1), np.concatenate([held, iq_format_model("cf32", x[: 2 * 4])]))
    finally:
        d.close()


# ------------------------------------------------------------------ the receive bridge
def test_rx_bridge_takes_typed_inputs(amd, capture, tmp_path):
    """`opv-rx-bridge --format F` on the device: the module's noisy capture as a cu8 file and as a cf32 file, one bridge each (a
    format applies to all inputs of a bridge) -> 134-byte datagrams == the oracle's frames for the model-converted int16. The
    bridge's buffers are pinned, so its blocks are read in place by k_push_convert."""
    import os
    import socket
    import subprocess
    exe = str(amd.PKG / "bin" / "opv-rx-bridge")
    for j, fmt in enumerate(["cu8", "cf32"]):
        q = quantise(fmt, capture)
        exp = Oracle().receive(iq_format_model(fmt, q), streaming=True, want_soft=False)["frames"]
        assert len(exp) == 4
        f = tmp_path / f"capture.{fmt}"
        q.tofile(f)
        port = 41000 + (os.getpid() % 2000) * 4 + j
        so = socket.socket(socket.AF_INET, socket.SOCK_DGRAM)
        so.setsockopt(socket.SOL_SOCKET, socket.SO_RCVBUF, 1 << 22)
        so.bind(("127.0.0.1", port))
        so.setblocking(False)
        try:
            r = subprocess.run([exe, "-q", "-P", str(port), "--format", fmt, str(f)], capture_output=True, timeout=120)
            assert r.returncode == 0, r.stderr.decode()
            got = []
            while True:
                try:
                    got.append(so.recv(2048))
                except BlockingIOError:
                    break
        finally:
            so.close()
        assert all(len(g) == 134 for g in got)
        assert np.array_equal(np.frombuffer(b"".join(got), np.uint8).reshape(-1, 134), exp), (fmt, len(got))
