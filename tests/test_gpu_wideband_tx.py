"""GPU: the wideband transmit bank (opv_wbtx_*, csrc/k_wideband_tx.hip + csrc/opv_wideband_tx.hip). k_wbtx_duc is integer-exact,
so every wide sample it writes is held to the numpy int64 model of tests/wideband_models.py with ==, for any split of the
inputs into pushes and any mix of present and absent channels; and the product's own chain - transmit bank, up-converter bank, DDC
bank, demodulators - is closed end to end: the wide capture == the model, each received stream's IQ == the DDC model of it, and each
stream is held to the ORACLE on that IQ like every other pushed stream of the suite.

Every output buffer has a canary in front of and behind it: a push writes n_in x U samples and nothing else."""
import ctypes as C

import numpy as np
import pytest

from fixtures import amd, torch_dev  # noqa: F401
from stream_checks import check_stream
from stream_runs import CHUNK, code_raised_by, collect
from wideband_device import (CANARY, LOOP_D4, PLAN_D4, Inputs, Out, assert_equal, assert_exactness_preconditions, exactness_inputs,
                             loop_taps_d4, loopback_on_the_cpu, plan_taps_d4, run_absent_channel_schedule)
from wideband_models import WIDE_RATE, tx_phase_taps, wb_model, wb_model_inc, wbtx_model

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6


# ------------------------------------------------------------------ 1. exactness
CASES = {
    # name: (U, L, K, S, first_sample, n_in, input)
    "U1_L1_K1_S0": (1, 1, 1, 0, 0, 1000, "unit"),                            # S = 0: no rounding term
    "U3_L2_K5_wrap32": (3, 2, 5, 32, (1 << 32) - 1000, 700, "random"),       # phase 2 has no tap; the phase product wraps inside the capture
    "U4_L143_K33_wrap40": (4, 143, 33, 32, (1 << 40) + 7, 600, "random"),    # 36 / 36 / 36 / 35 taps per phase
    "U16_L1024_K5": (16, 1024, 5, 31, 0, 450, "random"),
    "U1_L143_K5_clamps": (1, 143, 5, 29, (1 << 32) - 1000, 2000, "fullscale"),   # full-scale input, gain 4 per channel: both clamps fire
    "U4_L2_K1_halfway": (4, 2, 1, 3, 0, 300, "halfway"),                     # sums at negative half-way points
    "U1_L2_K256_bound": (1, 2, 256, 40, 0, 600, "bound"),                    # the largest sum the limits allow, unclamped after S = 40
}


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_integer_model_on_every_sample(amd, torch_dev, case):
    """two pushes, the cut inside the filter's history (the second push's first outputs read samples of the first push and, where
    the history is longer than the first push, the zeros in front of it), more outputs than one workgroup's tile; == the model"""
    U, L, K, S, first, N, kind = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T = amd.wb_lo_table()
    chans, taps, centres = exactness_inputs(kind, rng, "tx", U * WIDE_RATE, K, N, L, U)
    inc = amd.wbtx_plan(U, centres, taps, S, first)
    assert np.array_equal(inc, wb_model_inc(U, centres))
    exp = wbtx_model(T, chans, U, inc, taps, S, first)
    assert exp.size == 2 * N * U and N * U > 256, "more than one workgroup of outputs"
    w = None
    if kind == "halfway":
        # centre 0: w = 32767 x I on phases 0 and 1 (a tap of 1 each), 0 on phases 2 and 3 (no tap). With S = 3 a sum is half-way when
        # w = 4 (mod 8), i.e. I = 4 (mod 8): I = -4
        w = np.zeros(N * U, np.int64)
        w[0::U] = w[1::U] = 32767 * chans[0][0::2].astype(np.int64)
    assert_exactness_preconditions(kind, exp, unclamped=("random", "unit"), halfway=(w, exp[0::2]))
    if "wrap32" in case:
        assert first < (1 << 32) <= first + N * U
    H = -(-(L - 1) // U)
    cut = (H + 1) // 2 if H > 1 else N // 2
    assert 0 < cut < N and (H <= 1 or cut < H)
    d = amd.Demod(1, max_samples=1 << 16)
    tx = amd.WidebandTx(d, U, centres, taps, S, first)
    try:
        src, out = Inputs(torch_dev, chans), Out(torch_dev, N * U)
        tx.push([src.ptr(k) for k in range(K)], cut, out.ptr())
        assert tx.samples() == cut
        tx.push([src.ptr(k, cut) for k in range(K)], N - cut, out.ptr(cut * U))
        assert tx.samples() == N
        assert_equal(out.get(), exp, case)
    finally:
        tx.close()
        d.close()


# ------------------------------------------------------------------ 2. pushes
def test_any_split_absent_channels_shared_buffers_and_reset(amd, torch_dev):
    """pushes of 1 sample, of fewer than ceil((L - 1) / U) samples and of 0 samples; a channel absent (null) from some pushes and
    present in the next, and the other way round; two channels reading the same buffer; an all-null push; then reset and a second
    run at another first_sample: all == the model fed with zeros where a channel was absent"""
    rng = np.random.default_rng(22)
    U, L, S, K = 4, 23, 31, 4
    H = -(-(L - 1) // U)
    assert H == 6
    centres = [300000.0, -700000.0, 0.0, 300000.0]
    taps = tx_phase_taps(rng, L, U)
    # (n_in, channels present): channel 3 always reads channel 0's buffer
    schedule = [(1, {0, 1, 2, 3}), (H - 2, {0, 2, 3}), (0, {0, 1, 2, 3}), (1, {0, 1, 2, 3}), (H - 1, {1, 3}), (200, {0, 1, 2, 3}),
                (H - 3, set()), (2, {2}), (150, {0, 1, 3}), (1, {1})]
    N = sum(n for n, _ in schedule)
    data = [rng.integers(-32768, 32768, 2 * N).astype(np.int16) for _ in range(3)]
    T = amd.wb_lo_table()
    d = amd.Demod(1, max_samples=1 << 16)
    tx = amd.WidebandTx(d, U, centres, taps, S, 12345)
    try:
        src = Inputs(torch_dev, data)
        for first in (12345, (1 << 32) - 77):
            fed = [x.copy() for x in data] + [data[0].copy()]
            out = Out(torch_dev, N * U)
            run_absent_channel_schedule(tx, src, out, schedule, K, fed, lambda at: at * U)
            exp = wbtx_model(T, fed, U, wb_model_inc(U, centres), taps, S, first)
            assert N * U > 256 and (np.abs(exp.astype(np.int32)) < 32767).mean() > 0.6
            assert_equal(out.get(), exp, f"first_sample {first}")
            tx.reset((1 << 32) - 77)                                         # the second pass starts from an empty history at another phase
            assert tx.samples() == 0
    finally:
        tx.close()
        d.close()


# ------------------------------------------------------------------ 3. refusals are atomic
def test_refused_pushes_change_nothing(amd, torch_dev):
    """every refusal answers its documented code, writes nothing, leaves samples() alone, and the pushes around it still == the
    model of the accepted pushes alone; an object whose context was closed first is detached"""
    torch, dev = torch_dev
    rng = np.random.default_rng(33)
    U, L, S, K = 4, 9, 31, 2
    centres, taps = [250000.0, -400000.0], tx_phase_taps(rng, L, U)
    N, piece = 600, 200
    data = [rng.integers(-32768, 32768, 2 * N).astype(np.int16) for _ in range(K)]
    exp = wbtx_model(amd.wb_lo_table(), data, U, wb_model_inc(U, centres), taps, S)
    d = amd.Demod(1, max_samples=1 << 16)
    tx = amd.WidebandTx(d, U, centres, taps, S)
    L_ = amd.lib()
    try:
        src, out = Inputs(torch_dev, data), Out(torch_dev, N * U)
        scratch = Out(torch_dev, piece * U)
        canary = scratch.buf.cpu().numpy().copy()
        tx.push([src.ptr(0), src.ptr(1)], piece, out.ptr())
        ins = [src.ptr(0, piece), src.ptr(1, piece)]
        tab = (C.c_void_p * K)(*ins)
        refusals = [
            (EINVAL, lambda: amd._chk(L_.opv_wbtx_push(tx.h, None, piece, C.c_void_p(scratch.ptr())))),         # null table
            (EINVAL, lambda: amd._chk(L_.opv_wbtx_push(tx.h, tab, piece, None))),                               # null output
            (EINVAL, lambda: tx.push(ins, piece, src.ptr(1, piece + piece - 1))),                               # the output starts inside input 1
            (EINVAL, lambda: tx.push(ins, piece, src.ptr(0, piece) - 4 * (piece * U - 1))),                     # the output ends inside input 0
            (EINVAL, lambda: tx.push([ins[0], None], piece, src.ptr(0, piece))),                                # the output IS an input
            (EINVAL, lambda: tx.push(ins, (1 << 31) // U, scratch.ptr())),                                      # n_in x U = 2^31
            (EINVAL, lambda: tx.push(ins, 1 << 40, scratch.ptr())),
            (EINVAL, lambda: tx.push(ins, piece, scratch.ptr() + 2)),                                           # misaligned output
            (EINVAL, lambda: tx.push([ins[0] + 2, ins[1]], piece, scratch.ptr())),                              # misaligned input
            (EINVAL, lambda: amd._chk(L_.opv_wbtx_push(None, tab, piece, C.c_void_p(scratch.ptr())))),          # null object
        ]
        for code, call in refusals:
            assert code_raised_by(amd, call) == code
            assert tx.samples() == piece
        torch.cuda.synchronize()
        assert np.array_equal(scratch.buf.cpu().numpy(), canary) and np.array_equal(src.t.cpu().numpy(), np.stack(data))
        tx.push(ins, 0, scratch.ptr())                                       # nothing to do is not misuse, and changes nothing
        assert tx.samples() == piece and np.array_equal(scratch.buf.cpu().numpy(), canary)
        tx.push([src.ptr(0, piece), src.ptr(1, piece)], N - piece, out.ptr(piece * U))
        assert_equal(out.get(), exp, "around the refusals")
        # a detached object: its context goes first
        d2 = amd.Demod(1, max_samples=1 << 16)
        tx2 = amd.WidebandTx(d2, U, centres, taps, S)
        tx2.push([src.ptr(0), src.ptr(1)], piece, scratch.ptr())
        assert_equal(scratch.get(), exp[: 2 * piece * U], "before the context went")
        d2.close()
        scratch.buf.fill_(CANARY)
        torch.cuda.synchronize()
        assert code_raised_by(amd, lambda: tx2.push(ins, piece, scratch.ptr())) == ESTATE
        assert code_raised_by(amd, lambda: tx2.reset(0)) == ESTATE
        assert tx2.samples() == piece and np.array_equal(scratch.buf.cpu().numpy(), canary)
        tx2.close()
        assert amd.lib().opv_wbtx_samples(None) == 0
    finally:
        tx.close()
        d.close()


# ------------------------------------------------------------------ 4. loopback: transmit bank -> up-converters -> DDC bank -> demodulators
@pytest.fixture(scope="module")
def loop(amd, oracle):
    """the chain on the CPU, from the two models and the oracle alone: -> dict(tx[k], chans[k], wide, model[k], exp[k]). All three
    channels start at sample 0 and the run ends with the modulator's 4000 silent samples. The filters delay by 2 x 160 wide samples =
    two symbols exactly, so the reference's timing loop starts on a symbol boundary."""
    U, D = LOOP_D4["U"], PLAN_D4["D"]
    return loopback_on_the_cpu(
        amd, oracle, LOOP_D4,
        lambda T, chans: wbtx_model(T, chans, U, wb_model_inc(U, LOOP_D4["centres"]), loop_taps_d4(), LOOP_D4["out_shift"]),
        lambda T, wide: wb_model(T, wide, D, wb_model_inc(D, PLAN_D4["centres"]), plan_taps_d4(), PLAN_D4["out_shift"]))


def test_loopback_through_the_products_own_chain(amd, torch_dev, loop):
    """a TxBank of 3 streams modulates one frame per round; WidebandTx puts the three captures at -1.1, 0.0 and +1.6 MHz of a wide
    capture at 8.672 MS/s (an all-null push of 4000 samples is the tail); every wide block goes straight into Wideband.push_device,
    which feeds a 4-stream Demod. The wide capture == wbtx_model, each stream's IQ == wb_model of it, each stream passes
    check_stream against the oracle on that IQ, frames == the transmitted ones on slots 0 - 2 and none on slot 3."""
    torch, dev = torch_dev
    F, U, tail = LOOP_D4["frames"], LOOP_D4["U"], LOOP_D4["tail"]
    n_wide = (F * CHUNK + tail) * U
    d = amd.Demod(4, max_samples=n_wide // PLAN_D4["D"] + 64, streaming=True)
    bank = amd.TxBank(d, 3)
    up = amd.WidebandTx(d, U, LOOP_D4["centres"], loop_taps_d4(), LOOP_D4["out_shift"])
    wb = amd.Wideband(d, PLAN_D4["D"], [0, 1, 2, 3], PLAN_D4["centres"], plan_taps_d4(), PLAN_D4["out_shift"])
    try:
        lanes = torch.zeros((3, 2 * CHUNK), dtype=torch.int16, device=dev)
        assert lanes.data_ptr() % 16 == 0 and (lanes.stride(0) * 2) % 16 == 0
        out = Out(torch_dev, n_wide)
        ptrs = [lanes[k].data_ptr() for k in range(3)]
        for r in range(F):
            assert bank.round([0, 1, 2], [loop["tx"][k][r: r + 1] for k in range(3)], ptrs) >= 0
            up.push(ptrs, CHUNK, out.ptr(r * CHUNK * U))
            wb.push_device(out.ptr(r * CHUNK * U), CHUNK * U)
        up.push([None] * 3, tail, out.ptr(F * CHUNK * U))
        wb.push_device(out.ptr(F * CHUNK * U), tail * U)
        assert up.samples() == F * CHUNK + tail
        assert_equal(out.get(), loop["wide"], "wide capture")
        for k in range(4):
            assert_equal(d.iq(k), loop["model"][k], f"slot {k} IQ")
        wb.flush()
        d.process()
        d.sync()
        for k, exp in enumerate(loop["exp"]):
            got = collect(d, k)
            assert got["state"].stalled == 0
            check_stream(amd, got, exp, f"loopback slot {k}", edge_ties=0, offset_ties=None)
            if k < 3:
                assert np.array_equal(got["frames"], loop["tx"][k]), k
            else:
                assert len(got["frames"]) == 0 and d.state(k).frames_released == 0
    finally:
        wb.close()
        up.close()
        bank.close()
        d.close()
