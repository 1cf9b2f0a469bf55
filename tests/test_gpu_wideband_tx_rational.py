"""GPU: the rational up-converter bank (opv_wbtx_create_rational, csrc/k_wideband_tx_rational.hip + csrc/opv_wideband_tx.hip): a
wide capture at 2 168 000 x down / up S/s. k_wbtxr_duc is integer-exact, so every wide sample it writes is held to the numpy int64
model of tests/wideband_models.py with ==, for any split of the inputs into pushes and any mix of present and absent
channels; with up = 1 it must deliver the bytes of the integer bank; and the product's own chain - transmit bank, rational
up-converter bank, rational DDC bank, demodulators - is closed end to end at 10 MS/s (1250 / 271): the wide capture == the model,
each received stream's IQ == the door's model of it, and each stream is held to the ORACLE on that IQ.

Every output buffer has a canary in front of and behind it: a push writes W(N + n_in) - W(N) samples and nothing else."""
import ctypes as C

import numpy as np
import pytest

from fixtures import amd, torch_dev  # noqa: F401
from stream_runs import CHUNK, code_raised_by
from wideband_device import (CANARY, LOOP_10M, PLAN_10M, Inputs, Out, assert_equal, assert_exactness_preconditions, check_plan_streams_10m,
                             exactness_inputs, first_one_tap_window, loop_taps_10m, loopback_on_the_cpu, plan_taps_10m, push_pieces,
                             run_absent_channel_schedule)
from wideband_models import WIDE_RATE, tx_phase_taps, wbr_model, wbr_model_inc, wbtx_model, wbtxr_model, wbtxr_outputs

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = -1, -6


def phase_of(M, U, n):
    return (np.arange(n, dtype=np.int64) * U) % M


# ------------------------------------------------------------------ 1. exactness
CASES = {
    # name: (down, up, L, K, S, first_sample, n_in, input)
    "3_2_L1_empty_phases": (3, 2, 1, 1, 0, 0, 1000, "unit"),               # J = 1: every output with p != 0 is exactly 0; S = 0: no rounding term
    "625_542_ragged_wrap32": (625, 542, 625 * 3 + 17, 5, 32, (1 << 32) - 1000, 1500, "random"),   # ragged last tap row; the phase product wraps
    "1250_271_K33_wrap40": (1250, 271, 1250 * 8, 33, 33, (1 << 40) + 7, 700, "random"),
    "7680_271_J64": (7680, 271, 7680 * 64, 5, 33, 0, 300, "random"),       # the 1 MB table and the largest J
    "32_1_L1024": (32, 1, 1024, 5, 32, 0, 300, "random"),                  # the largest ratio
    "8192_8191_all_rows": (8192, 8191, 16384, 3, 31, 0, 9000, "random"),   # the phase walks through all 8192 rows
    "1_1_L64_K5_clamps": (1, 1, 64, 5, 29, (1 << 32) - 1000, 2000, "fullscale"),   # full-scale input, gain 4 per channel: both clamps fire
    "3_2_L2_halfway": (3, 2, 2, 1, 3, 0, 300, "halfway"),                  # sums at negative half-way points
    "1_1_L2_K256_bound": (1, 1, 2, 256, 40, 0, 600, "bound"),              # the largest sum the limits allow, unclamped after S = 40
}


@pytest.mark.parametrize("case", list(CASES))
def test_outputs_equal_the_integer_model_on_every_sample(amd, torch_dev, case):
    """two pushes, the cut inside the filter's history and (up > 1) inside a resampling period, so that the second push starts at a
    phase other than 0; more outputs than one workgroup's tile; == the model"""
    M, U, L, K, S, first, N, kind = CASES[case]
    rng = np.random.default_rng(sum(map(ord, case)))
    T = amd.wb_lo_table()
    chans, taps, centres = exactness_inputs(kind, rng, "tx", M * WIDE_RATE / U, K, N, L, M)
    if kind == "unit":
        centres[0] = 0.0                                                   # (the empty-phase case below reads its expectation off centre 0)
    inc = amd.wbtxr_plan(M, U, centres, taps, S, first)
    assert np.array_equal(inc, wbr_model_inc(M, U, centres))
    exp = wbtxr_model(T, chans, M, U, inc, taps, S, first)
    W = amd.wbtxr_outputs(M, U, N)
    assert W == wbtxr_outputs(M, U, N) and exp.size == 2 * W and W > 256, "more than one workgroup of outputs"
    p_n = phase_of(M, U, W)
    if kind == "unit":
        # centre 0, one tap of 1 at phase 0: w = 32767 x (I, Q) where p_n = 0, exactly 0 elsewhere
        assert not exp[0::2][p_n != 0].any() and not exp[1::2][p_n != 0].any() and (p_n != 0).sum() > W // 4
        q_0 = ((np.arange(W, dtype=np.int64) * U) // M)[p_n == 0]
        assert np.array_equal(exp[0::2][p_n == 0], 32767 * chans[0][0::2].astype(np.int64)[q_0]) and exp[0::2].any() and exp[1::2].any()
    w = None
    if kind == "halfway":
        # centre 0: w = 32767 x I[q_n] on phases 0 and 1 (a tap of 1 each), 0 on phase 2 (no tap). With S = 3 a sum is half-way when
        # w = 4 (mod 8), i.e. I = 4 (mod 8): I = -4
        q_n = (np.arange(W, dtype=np.int64) * U) // M
        w = np.where(p_n < 2, 32767 * chans[0][0::2].astype(np.int64)[q_n], 0)
        assert (p_n == 2).any()
    assert_exactness_preconditions(kind, exp, unclamped=("random",), halfway=(w, exp[0::2]))
    if "wrap32" in case:
        assert first < (1 << 32) <= first + W
    if "all_rows" in case:
        assert np.unique(p_n).size == M
    if "ragged" in case:
        assert L % M
    H = -(-L // M) - 1
    cut = (H + 1) // 2 if H > 1 else N // 2
    while U > 1 and (cut * M) % U == 0:
        cut += 1
    assert 0 < cut < N and (H <= 1 or cut < H) and (U == 1 or (cut * M) % U)
    d = amd.Demod(1, max_samples=1 << 16)
    tx = amd.WidebandTx.rational(d, M, U, centres, taps, S, first)
    try:
        src, out = Inputs(torch_dev, chans), Out(torch_dev, W)
        push_pieces(tx, src, out, M, U, K, [0, cut, N])
        assert_equal(out.get(), exp, case)
    finally:
        tx.close()
        d.close()


# ------------------------------------------------------------------ 2. up = 1 is the integer bank
@pytest.mark.parametrize("M,L", [(1, 64), (4, 143), (16, 1024)])
def test_up_1_delivers_the_bytes_of_the_integer_bank(amd, torch_dev, M, L):
    """a rational object (down = M, up = 1) and an opv_wbtx_create object (interp = M) fed the same inputs in the same pieces: the
    same bytes, == both models"""
    rng = np.random.default_rng(50 + M)
    K, S, first, N = 5, 32, (1 << 32) - 1000, 700
    centres = list(rng.uniform(-M * WIDE_RATE / 2, M * WIDE_RATE / 2, K))
    chans, taps = [rng.integers(-32768, 32768, 2 * N).astype(np.int16) for _ in range(K)], tx_phase_taps(rng, L, M)
    T = amd.wb_lo_table()
    inc = amd.wbtxr_plan(M, 1, centres, taps, S, first)
    assert np.array_equal(inc, amd.wbtx_plan(M, centres, taps, S, first))
    exp = wbtx_model(T, chans, M, inc, taps, S, first)
    assert np.array_equal(exp, wbtxr_model(T, chans, M, 1, inc, taps, S, first))
    assert amd.wbtxr_outputs(M, 1, N) == N * M > 256 and (np.abs(exp.astype(np.int32)) < 32767).mean() > 0.6
    d = amd.Demod(1, max_samples=1 << 16)
    a = amd.WidebandTx.rational(d, M, 1, centres, taps, S, first)
    b = amd.WidebandTx(d, M, centres, taps, S, first)
    try:
        src, outs = Inputs(torch_dev, chans), (Out(torch_dev, N * M), Out(torch_dev, N * M))
        cuts = [0, 1, 6, (N // 2) | 1, N - 2, N]
        for tx, out in zip((a, b), outs):
            push_pieces(tx, src, out, M, 1, K, cuts)
        x, y = outs[0].get(), outs[1].get()
        assert_equal(x, y, "rational vs integer object")
        assert_equal(x, exp, "rational object vs model")
    finally:
        a.close()
        b.close()
        d.close()


# ------------------------------------------------------------------ 3. pushes
def test_any_split_absent_channels_shared_buffers_and_reset(amd, torch_dev):
    """at 1250 / 271: pushes of 1 sample (4 or 5 wide samples: both occur), of fewer than J - 1 samples and of 0 samples; a channel
    absent (null) from some pushes and present in the next, and the other way round; two channels reading the same buffer; an
    all-null push; then reset and a second run at another first_sample: all == the model fed with zeros where a channel was absent"""
    rng = np.random.default_rng(23)
    M, U, S, K = 1250, 271, 32, 4
    L = M * 8 - 3
    H = -(-L // M) - 1
    assert H == 7
    fw = M * WIDE_RATE / U
    centres = [300000.0, -700000.0, 0.0, 0.3 * fw]
    taps = tx_phase_taps(rng, L, M)
    # (n_in, channels present): channel 3 always reads channel 0's buffer
    everyone = {0, 1, 2, 3}
    schedule = [(1, everyone), (H - 2, {0, 2, 3}), (0, everyone), (1, everyone), (H - 1, {1, 3}), (200, everyone),
                (H - 3, set()), (2, {2}), (150, {0, 1, 3}), (1, {1}), (1, everyone), (1, everyone), (1, {0, 3})]
    N = sum(n for n, _ in schedule)
    W = wbtxr_outputs(M, U, N)
    data = [rng.integers(-32768, 32768, 2 * N).astype(np.int16) for _ in range(3)]
    T = amd.wb_lo_table()
    inc = wbr_model_inc(M, U, centres)
    d = amd.Demod(1, max_samples=1 << 16)
    tx = amd.WidebandTx.rational(d, M, U, centres, taps, S, 12345)
    try:
        src = Inputs(torch_dev, data)
        for first in (12345, (1 << 32) - 77):
            fed = [x.copy() for x in data] + [data[0].copy()]
            out = Out(torch_dev, W)
            run_absent_channel_schedule(tx, src, out, schedule, K, fed, lambda at: wbtxr_outputs(M, U, at))
            starts = np.cumsum([0] + [n for n, _ in schedule])
            single = {amd.wbtxr_outputs(M, U, int(at) + 1) - amd.wbtxr_outputs(M, U, int(at)) for at, (n, _) in zip(starts, schedule) if n == 1}
            assert single == {4, 5}, single
            exp = wbtxr_model(T, fed, M, U, inc, taps, S, first)
            assert W > 256 and exp.size == 2 * W and (np.abs(exp.astype(np.int32)) < 32767).mean() > 0.6
            assert_equal(out.get(), exp, f"first_sample {first}")
            tx.reset((1 << 32) - 77)                                         # the second pass starts from an empty history at another phase
            assert tx.samples() == 0
    finally:
        tx.close()
        d.close()


# ------------------------------------------------------------------ 4. refusals are atomic
def test_refused_pushes_change_nothing(amd, torch_dev):
    """every refusal answers its documented code, writes nothing, leaves samples() alone, and the pushes around it still == the
    model of the accepted pushes alone; the overlap test takes the output range from the rational count: an output that ends where
    an input begins is accepted, one sample further it is refused; an object whose context was closed first is detached"""
    torch, dev = torch_dev
    rng = np.random.default_rng(34)
    M, U, S, K = 5, 3, 31, 2
    L = M * 4 + 2
    centres, taps = [250000.0, -400000.0], tx_phase_taps(rng, L, M)
    N, piece = 600, 200
    data = [rng.integers(-32768, 32768, 2 * N).astype(np.int16) for _ in range(K)]
    exp = wbtxr_model(amd.wb_lo_table(), data, M, U, wbr_model_inc(M, U, centres), taps, S)
    cum = [wbtxr_outputs(M, U, i * piece) for i in range(4)]
    n_w = [b - a for a, b in zip(cum, cum[1:])]
    assert (piece * M) % U and len(set(n_w)) == 2 and n_w[1] != piece * (M // U) and n_w[1] != piece * -(-M // U)
    d = amd.Demod(1, max_samples=1 << 16)
    tx = amd.WidebandTx.rational(d, M, U, centres, taps, S)
    L_ = amd.lib()
    try:
        src, out = Inputs(torch_dev, data), Out(torch_dev, cum[3])
        scratch = Out(torch_dev, n_w[1] + 8)
        canary = scratch.buf.cpu().numpy().copy()
        # one sample of canary, room for exactly the wide samples of the last push, and right behind it the last piece of channel 0 once more
        adj = torch.full((2 * (n_w[2] + 1 + piece),), CANARY, dtype=torch.int16, device=dev)
        adj[2 * (n_w[2] + 1):] = torch.from_numpy(data[0][2 * 2 * piece:]).to(dev)
        adj_in = adj.data_ptr() + 4 * (n_w[2] + 1)
        tx.push([src.ptr(0), src.ptr(1)], piece, out.ptr())
        ins = [src.ptr(0, piece), src.ptr(1, piece)]
        tab = (C.c_void_p * K)(*ins)
        refusals = [
            (EINVAL, lambda: amd._chk(L_.opv_wbtx_push(tx.h, None, piece, C.c_void_p(scratch.ptr())))),         # null table
            (EINVAL, lambda: amd._chk(L_.opv_wbtx_push(tx.h, tab, piece, None))),                               # null output
            (EINVAL, lambda: tx.push(ins, piece, src.ptr(1, piece + piece - 1))),                               # the output starts inside input 1
            (EINVAL, lambda: tx.push(ins, piece, src.ptr(0, piece) - 4 * (n_w[1] - 1))),                        # the output ends inside input 0
            (EINVAL, lambda: tx.push([ins[0], None], piece, src.ptr(0, piece))),                                # the output IS an input
            (EINVAL, lambda: tx.push(ins, ((1 << 31) * U) // M + 1, scratch.ptr())),                            # 2^31 wide samples or more
            (EINVAL, lambda: tx.push(ins, 1 << 31, scratch.ptr())),
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
        tx.push(ins, piece, out.ptr(cum[1]))
        # the last push reads channel 0 from `adj`: an output one sample into that input is refused, the one that ends where it begins is taken
        last = [adj_in, src.ptr(1, 2 * piece)]
        assert code_raised_by(amd, lambda: tx.push(last, piece, adj.data_ptr() + 8)) == EINVAL and tx.samples() == 2 * piece
        tx.push(last, piece, adj.data_ptr() + 4)
        assert tx.samples() == N
        torch.cuda.synchronize()
        got = adj.cpu().numpy()
        assert (got[:2] == CANARY).all() and np.array_equal(got[2 * (n_w[2] + 1):], data[0][2 * 2 * piece:])
        assert_equal(np.concatenate([out.get()[: 2 * cum[2]], got[2: 2 * (n_w[2] + 1)]]), exp, "around the refusals")
        # a detached object: its context goes first
        d2 = amd.Demod(1, max_samples=1 << 16)
        tx2 = amd.WidebandTx.rational(d2, M, U, centres, taps, S)
        tx2.push([src.ptr(0), src.ptr(1)], piece, scratch.ptr())
        assert_equal(scratch.get()[: 2 * n_w[0]], exp[: 2 * n_w[0]], "before the context went")
        d2.close()
        scratch.buf.fill_(CANARY)
        torch.cuda.synchronize()
        assert code_raised_by(amd, lambda: tx2.push(ins, piece, scratch.ptr())) == ESTATE
        assert code_raised_by(amd, lambda: tx2.reset(0)) == ESTATE
        assert tx2.samples() == piece and np.array_equal(scratch.buf.cpu().numpy(), canary)
        tx2.close()
    finally:
        tx.close()
        d.close()


# ------------------------------------------------------------------ 5. loopback at 10 MS/s: transmit bank -> up-converters -> rational door -> demodulators
@pytest.fixture(scope="module")
def loop(amd, oracle):
    """the chain on the CPU, from the two models and the oracle alone: -> dict(tx[k], chans[k], wide, model[k], exp[k]). All three
    channels start at sample 0 and the run ends with the modulator's 4000 silent samples."""
    M, U = LOOP_10M["down"], LOOP_10M["up"]
    chain = loopback_on_the_cpu(
        amd, oracle, LOOP_10M,
        lambda T, chans: wbtxr_model(T, chans, M, U, wbr_model_inc(M, U, LOOP_10M["centres"]), loop_taps_10m(), LOOP_10M["out_shift"]),
        lambda T, wide: wbr_model(T, wide, M, U, wbr_model_inc(M, U, PLAN_10M["centres"]), plan_taps_10m(), PLAN_10M["out_shift"]))
    # on top of its preconditions, from the reference alone: no one-tap window on slots 0 - 2; the empty slot's one-tap windows are why
    # check_plan_streams_10m's slot rule is the one to use
    for k in range(3):
        assert first_one_tap_window(chain["exp"][k])[1] == 0, f"loopback plan: channel {k} shows a one-tap window"
    assert first_one_tap_window(chain["exp"][3])[1] >= 1
    return chain


def test_loopback_at_10_msps_through_the_products_own_chain(amd, torch_dev, loop):
    """a TxBank of 3 streams modulates one frame per round; WidebandTx.rational(1250, 271) puts the three captures at -3.1, 0.0 and
    +1.7 MHz of a wide capture at 10 MS/s (an all-null push of 4000 samples is the tail); every wide block goes straight into
    Wideband.rational(1250, 271).push_device, which feeds a 4-stream Demod (the last slot, +3.9 MHz, is empty). The wide capture ==
    wbtxr_model, each stream's IQ == wbr_model of it, each stream passes check_plan_streams_10m against the oracle on that IQ, frames
    == the transmitted ones on slots 0 - 2 and none on slot 3."""
    torch, dev = torch_dev
    F, M, U, tail = LOOP_10M["frames"], LOOP_10M["down"], LOOP_10M["up"], LOOP_10M["tail"]
    n_in = F * CHUNK + tail
    n_wide = wbtxr_outputs(M, U, n_in)
    assert wbtxr_outputs(M, U, CHUNK) * U == CHUNK * M and 2 * n_wide == loop["wide"].size      # a frame is a whole number of wide samples
    d = amd.Demod(4, max_samples=loop["model"].shape[1] // 2 + 64, streaming=True)
    bank = amd.TxBank(d, 3)
    up = amd.WidebandTx.rational(d, M, U, LOOP_10M["centres"], loop_taps_10m(), LOOP_10M["out_shift"])
    wb = amd.Wideband.rational(d, M, U, [0, 1, 2, 3], PLAN_10M["centres"], plan_taps_10m(), PLAN_10M["out_shift"])
    try:
        lanes = torch.zeros((3, 2 * CHUNK), dtype=torch.int16, device=dev)
        assert lanes.data_ptr() % 16 == 0 and (lanes.stride(0) * 2) % 16 == 0
        out = Out(torch_dev, n_wide)
        ptrs = [lanes[k].data_ptr() for k in range(3)]
        for r in range(F + 1):
            lo, hi = wbtxr_outputs(M, U, r * CHUNK), wbtxr_outputs(M, U, min((r + 1) * CHUNK, n_in))
            if r < F:
                assert bank.round([0, 1, 2], [loop["tx"][k][r: r + 1] for k in range(3)], ptrs) >= 0
                up.push(ptrs, CHUNK, out.ptr(lo))
            else:
                up.push([None] * 3, tail, out.ptr(lo))
            wb.push_device(out.ptr(lo), hi - lo)
        assert up.samples() == n_in
        assert_equal(out.get(), loop["wide"], "wide capture")
        for k in range(4):
            assert_equal(d.iq(k), loop["model"][k], f"slot {k} IQ")
        wb.flush()
        d.process()
        d.sync()
        check_plan_streams_10m(amd, d, loop, "loopback")                       # (pops every slot's frames: == the oracle's)
        for k in range(3):                                                 # ... which are the transmitted ones, and none on slot 3
            assert np.array_equal(loop["exp"][k]["frames"], loop["tx"][k]) and d.state(k).frames_released == len(loop["tx"][k]), k
        assert len(loop["exp"][3]["frames"]) == 0 and d.state(3).frames_released == 0
    finally:
        wb.close()
        up.close()
        bank.close()
        d.close()
