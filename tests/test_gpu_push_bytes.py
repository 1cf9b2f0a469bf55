"""GPU: the serving path's gather kernel, byte for byte. k_push_gather (csrc/opv_push.hip) carries every live stream's samples
across PCIe - one launch per opv_push_iq_batch, a table of (source, destination, bytes, wide) pairs, each pair cut into `slices`
work items (opv_stream_rules.h: table_launch) - and the other tests hold it only through demodulated output, with tolerances. Here
a scratch context that never runs opv_process takes blocks of random int16 (views of pinned torch buffers, every value of the
type) and after every batch opv_tap_iq must return, for every stream, the numpy concatenation of what was pushed to it: == on
every int16. The shapes are the smallest that reach each branch of the kernel and of push_deferred's choice of route.

Which route a block took is not visible from outside; what sends a block to hipMemcpyAsync instead (pageable memory, a source that
is not 4-byte aligned, a batch of one block, OPV_PUSH_NO_GATHER) is push_deferred's rule, and both routes must deliver the bytes.

Known limit: opv_tap_iq cannot see past a stream's n_avail, so a write BEHIND the last block of a stream (an overrun of the
destination) is not observable here; a write into another stream's buffer or short of a block's end is."""
import numpy as np
import pytest

from fixtures import amd  # noqa: F401

pytestmark = pytest.mark.gpu

LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 1023, 1025, 4099]     # samples: below, at and beside one quad, one 16-quad row, 256 lanes x 4 / x 16


class PinnedPool:
    """one pinned torch buffer of random int16; take(n, off) -> a view of n samples that starts `off` samples (4 bytes each) behind
    a 16-byte boundary, off2 = 1: one int16 (2 bytes) further still"""

    def __init__(self, rng, n_int16):
        import torch
        self.t = torch.empty(n_int16, dtype=torch.int16).pin_memory()
        self.a = self.t.numpy()
        self.a[:] = rng.integers(-32768, 32768, n_int16)
        assert self.a.ctypes.data % 16 == 0
        self.at = 0

    def take(self, n, off=0, off2=0):
        lo = self.at + 2 * off + off2
        v = self.a[lo: lo + 2 * n]
        assert v.size == 2 * n, "pool exhausted"
        assert v.ctypes.data % 16 == 4 * off + 2 * off2
        self.at = (lo + 2 * n + 7) // 8 * 8
        return v


def assert_streams_hold(d, expected, tag):
    for k, parts in enumerate(expected):
        want = np.concatenate(parts) if parts else np.zeros(0, np.int16)
        got = d.iq(k)
        assert got.size == want.size, f"{tag}: stream {k} holds {got.size // 2} samples, pushed {want.size // 2}"
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"{tag}: stream {k}: {bad.size} int16 differ, the first at {bad[0]} of {want.size}: {got[bad[0]]} vs {want[bad[0]]}"


def push(d, ids, blocks, mode):
    if mode == "async":
        d.push_batch(ids, blocks, wait=False)
        d.push_wait()
    else:
        d.push_batch(ids, blocks)


@pytest.mark.parametrize("mode", ["gather", "async", "copies"])
def test_alignment_matrix(amd, monkeypatch, mode):
    """16 streams in ONE batch: the source starts 0..3 samples into a quad x the destination does (a first opv_push_iq of 0..3
    samples), so that the one pair that may move int4 shares its table with fifteen that move ints; twice per block length (the
    second batch lands behind the first: other destination offsets), for every length of LENGTHS. The same through
    opv_push_iq_batch_async + opv_push_wait, and over the per-block copies (OPV_PUSH_NO_GATHER)."""
    if mode == "copies":
        monkeypatch.setenv("OPV_PUSH_NO_GATHER", "1")
    rng = np.random.default_rng(20261020)
    pool = PinnedPool(rng, 2 * len(LENGTHS) * 2 * 16 * (max(LENGTHS) + 8))
    for L in LENGTHS:
        d = amd.Demod(16, max_samples=2 * max(LENGTHS) + 64, streaming=True)
        try:
            expected = [[] for _ in range(16)]
            for k in range(16):
                if k % 4:
                    head = rng.integers(-32768, 32768, 2 * (k % 4)).astype(np.int16)
                    d.push(k, head)
                    expected[k].append(head)
            for batch in range(2):
                blocks = [pool.take(L, off=k // 4) for k in range(16)]
                push(d, list(range(16)), blocks, mode)
                for k in range(16):
                    expected[k].append(blocks[k].copy())
                assert_streams_hold(d, expected, f"{mode}, {L} samples, batch {batch}")
        finally:
            d.close()


@pytest.mark.parametrize("blocks_env", [None, "1", "7"])
def test_slicing_with_a_large_and_a_tiny_pair(amd, monkeypatch, blocks_env):
    """Two streams, 86 723 samples beside ONE sample: table_launch cuts each pair into 84 slices (the large block's 16-byte moves
    over 256 lanes), so the small pair has 83 empty slices and the 168 work items exceed the grid of 32 blocks - and of 1 and 7
    (OPV_PUSH_GATHER_BLOCKS). First batch: the large pair is wide with a 3-sample tail; second batch: the streams swap roles,
    the large block lands one sample into a quad and moves ints, the single sample three."""
    if blocks_env:
        monkeypatch.setenv("OPV_PUSH_GATHER_BLOCKS", blocks_env)
    rng = np.random.default_rng(7)
    big = 86723
    pool = PinnedPool(rng, 2 * 2 * (big + 16) + 64)
    d = amd.Demod(2, max_samples=2 * big + 64, streaming=True)
    try:
        expected = [[], []]
        for batch, (n0, n1) in enumerate([(big, 1), (1, big)]):
            blocks = [pool.take(n0), pool.take(n1)]
            d.push_batch([0, 1], blocks)
            expected[0].append(blocks[0].copy())
            expected[1].append(blocks[1].copy())
            assert_streams_hold(d, expected, f"blocks {blocks_env}, batch {batch}")
    finally:
        d.close()


def test_more_than_1024_pairs(amd):
    """1030 streams, one block of 1 + k % 61 samples each in one batch: table_launch gives one slice per pair and the grid's 32
    blocks stride over 1030 work items; then a second batch behind it (every destination offset)"""
    rng = np.random.default_rng(11)
    S = 1030
    pool = PinnedPool(rng, 2 * S * 2 * 72)
    d = amd.Demod(S, max_samples=4096, streaming=True)
    try:
        expected = [[] for _ in range(S)]
        for batch in range(2):
            blocks = [pool.take(1 + k % 61, off=(k // 61) % 4) for k in range(S)]
            d.push_batch(list(range(S)), blocks)
            for k in range(S):
                expected[k].append(blocks[k].copy())
            assert_streams_hold(d, expected, f"1030 pairs, batch {batch}")
    finally:
        d.close()


@pytest.mark.parametrize("mode", ["gather", "async"])
def test_mixed_sources_in_one_batch(amd, mode):
    """Beside gathered blocks, in the same batch: two blocks for the SAME stream (the second lands behind the first), a block in
    pageable memory, and a pinned block whose address is 2 bytes off a sample boundary - the last two must take the copy route
    (push_deferred) and arrive exact; twice, over the lengths that matter to either route."""
    rng = np.random.default_rng(13)
    pool = PinnedPool(rng, 1 << 18)
    d = amd.Demod(6, max_samples=1 << 15, streaming=True)
    try:
        expected = [[] for _ in range(6)]
        for batch, L in enumerate([5, 1025, 4099]):
            odd = pool.take(L + 3, off=1, off2=1)
            assert odd.ctypes.data % 4 == 2
            jobs = [(0, pool.take(L)), (1, pool.take(L + 1, off=2)), (2, pool.take(3)), (1, pool.take(L + 2, off=3)),
                    (3, rng.integers(-32768, 32768, 2 * L).astype(np.int16)), (4, odd), (5, pool.take(4 * L)), (2, pool.take(L, off=1))]
            push(d, [s for s, _ in jobs], [b for _, b in jobs], mode)
            for s, b in jobs:
                expected[s].append(b.copy())
            assert_streams_hold(d, expected, f"{mode}, mixed batch {batch}")
    finally:
        d.close()
