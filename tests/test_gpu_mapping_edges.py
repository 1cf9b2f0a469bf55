"""GPU: the stream-to-wave mapping at the exact stream counts where csrc/opv_round_rules.h (frontend_kernel) changes the kernel
or its launch shape - 16 | 17 (forced sixteen per wave: one wave | a workgroup of four), n_cu | n_cu + 1 (the fp64 ring | the
int16 ring), 512 | 513, 2048 | 2049, 8192 | 8193, 16384 | 16385 - ties the rule to what the built library launches: the kernel's
name is a literal of this file (tests/test_round_rules_host.py holds the rule itself, on the CPU, for every stream count).

At most one side of an edge fills its last workgroup; on the other that workgroup serves a single stream. So each context gets
the suite's clean 10-frame capture (iq10) on its FIRST and its LAST stream only - every other stream receives nothing (idle slots
beside running ones: what the late-armed rows of test_gpu_mapping_matrix exercise) - and both are held to the oracle with
stream_checks.check_stream in full: frames, metrics, release symbols, events, symbol count, every soft symbol, estimate, final
carry and the chunk log."""
import time

import pytest

from fixtures import amd  # noqa: F401
from stream_checks import check_stream
from stream_runs import collect, explain

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def expected(oracle, iq10):
    return oracle.receive(iq10, streaming=True)


# (streams, opv_set_frontend argument, the kernel opv_process must have launched)
EDGES = [(16, 0, "k_msk_frontend_rb"), (17, 0, "k_msk_frontend_rb"), ("n_cu", 0, "k_msk_frontend_rb"), ("n_cu+1", 0, "k_msk_frontend_rb"),
         (512, 0, "k_msk_frontend_rb"), (513, 0, "k_msk_frontend_rb_wg4"), (2048, 0, "k_msk_frontend_rb_wg4"), (2049, 0, "k_msk_frontend_x4_wg4"),
         (8192, 0, "k_msk_frontend_x4_wg4"), (8193, 0, "k_msk_frontend_x16_wg4"), (16384, 0, "k_msk_frontend_x16_wg4"),
         (16385, 0, "k_msk_frontend_x16_wg8"),
         (16, 16, "k_msk_frontend_x16"), (17, 16, "k_msk_frontend_x16_wg4"), (17, 4, "k_msk_frontend_x4_wg4"), (2049, 1, "k_msk_frontend_rb_wg4")]


@pytest.mark.parametrize("S,forced,kernel", EDGES, ids=[f"{s}-{f}" for s, f, _ in EDGES])
def test_mapping_at_its_edges_first_and_last_stream_vs_oracle(amd, iq10, expected, S, forced, kernel):
    if isinstance(S, str):
        import torch
        n_cu = torch.cuda.get_device_properties(0).multi_processor_count
        assert 17 < n_cu < 511, n_cu                                          # (the edge lies inside k_msk_frontend_rb's range)
        S = n_cu + (1 if S.endswith("+1") else 0)
    t0 = time.perf_counter()
    d = amd.Demod(S, max_samples=iq10.size // 2 + 64, streaming=True)
    t1 = time.perf_counter()
    try:
        if forced:
            d.set_frontend(forced)
        for k in (0, S - 1):
            d.push(k, iq10)
            d.flush(k)
        d.process()
        d.sync()
        assert d.frontend_kernel() == kernel, (S, forced, d.frontend_kernel())
        for k in (0, S - 1):
            got, tag = collect(d, k), f"{kernel} S={S} forced={forced} stream {k}"
            try:
                assert got["state"].stalled == 0, f"{tag}: stalled 0x{got['state'].stalled:x}"
                check_stream(amd, got, expected, tag)
            except AssertionError:
                explain(d, k, got, expected, tag)
                raise
        for k in {1, S // 2, S - 2} - {0, S - 1}:                             # the idle slots stayed idle
            st = d.state(k)
            assert (st.total_symbols, st.frames_released, st.n_chunks, st.stalled) == (0, 0, 0, 0), (k, st.total_symbols, st.frames_released)
    finally:
        t2 = time.perf_counter()
        d.close()
    print(f"S={S} forced={forced}: {kernel}; context created in {t1 - t0:.2f} s, round + checks {t2 - t1:.2f} s, closed in {time.perf_counter() - t2:.2f} s")
