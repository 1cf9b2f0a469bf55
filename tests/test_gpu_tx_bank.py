"""GPU: the transmit bank (include/opv_demod.h, opv_txb_*; csrc/k_tx_bank.hip, csrc/opv_tx_bank.hip) - N live modulators on the
device, their state carried from round to round. The criterion is exact everywhere: what a stream's rounds wrote `==` what the
host modulator (= `opv-mod`, tests/test_capi_and_host.py's sha256 pins) makes of the same frames. The model of the carried
sign parity is tests/tx_bank_model.py, pinned to the host modulator by tests/test_tx_bank_host.py."""
import numpy as np
import pytest

import tx_bank_model as M
from fixtures_built import amd  # noqa: F401
from stream_runs import code_raised_by
from tx_bank_runs import CANARY, ECAPACITY, EINVAL, ESTATE, FS, GAP, Lanes, stream_frames
from tx_bank_runs import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def test_any_split_into_rounds_equals_one_call(amd, dev):
    """5 streams with their own callsigns and tokens, 4 frames each, over six rounds of a fixed schedule: a zero-frame entry,
    streams absent from rounds, 1+1+2 / 4 at once / 3+1 / 2+2 / 1+1+1+1, entries in non-ascending stream order. Every stream's
    346 880 samples == the host's, every canary intact, the state where the model says."""
    frames = [stream_frames(amd, k, 4) for k in range(5)]
    schedule = [([2, 0, 4], [3, 1, 1]), ([1, 3], [4, 0]), ([4, 0, 3], [1, 1, 2]), ([3, 4], [2, 1]), ([0, 2], [2, 1]), ([4], [1])]
    d = amd.Demod(1, max_samples=1 << 16)
    bank = amd.TxBank(d, 5)
    out = Lanes(dev, 5, 4)
    assert sum(streams != sorted(streams) for streams, _ in schedule) >= 2 and any(0 in counts for _, counts in schedule)
    done = [0] * 5
    for streams, counts in schedule:
        patched = bank.round(streams, [frames[s][done[s]:done[s] + n] for s, n in zip(streams, counts)],
                             [out.ptr(s, done[s]) for s in streams])
        print("round", streams, counts, "host-patched samples:", patched)
        for s, n in zip(streams, counts):
            done[s] += n
        for s in range(5):                                                   # streams not named stand still
            assert bank.state(s) == (done[s] * M.FSYMS, M.sign_parity(amd, frames[s][:done[s]])), (s, done)
    assert done == [4] * 5
    for s in range(5):
        want = amd.modulate(frames[s])[:2 * 4 * FS]
        assert want.size == 2 * 346880
        assert np.array_equal(out.lane(s), want), s
        assert bank.state(s)[0] == 8672
    assert out.canaries_intact()
    bank.close()
    d.close()


def test_reset_and_state_move_between_banks(amd, dev):
    """opv_txb_reset: the stream's next frame starts with the silent symbol again and equals the host's frame 0.
    opv_txb_get_state on one bank + opv_txb_set_state on a fresh bank of another size: the run continues there (2 + 2 frames)
    with == to the run that did not move."""
    fr = stream_frames(amd, 7, 4)
    host = amd.modulate(fr)[:2 * 4 * FS]
    d = amd.Demod(1, max_samples=1 << 16)
    a = amd.TxBank(d, 3)
    out = Lanes(dev, 4, 4)
    a.round([1, 2], [fr[:2], fr[:2]], [out.ptr(0), out.ptr(1)])
    assert np.array_equal(out.lane(0)[:4 * FS], host[:4 * FS])
    # reset: frame 3 of the run, sent as the first frame after a reset, is what the host makes of it alone
    a.reset(1)
    assert a.state(1) == (0, 0) and a.state(2) == (2 * M.FSYMS, M.sign_parity(amd, fr[:2]))
    a.round([1], [fr[3:]], [out.ptr(0, 2)])
    alone = amd.modulate(fr[3:])[:2 * FS]
    assert not alone[:2 * M.SPS].any() and alone[2 * M.SPS:4 * M.SPS].any()
    assert np.array_equal(out.lane(0)[4 * FS:6 * FS], alone)
    assert not np.array_equal(alone, host[6 * FS:])                          # (mid-run the same frame is another signal)
    # move stream 2 of bank a to stream 5 of a bank of 7; both continue
    b = amd.TxBank(d, 7)
    sym, par = a.state(2)
    b.set_state(5, sym, par)
    assert b.state(5) == (sym, par) and b.state(4) == (0, 0)
    b.round([5], [fr[2:]], [out.ptr(2, 2)])
    a.round([2], [fr[2:]], [out.ptr(1, 2)])
    assert np.array_equal(out.lane(1), host)                                 # the run that did not move
    assert np.array_equal(out.lane(2)[4 * FS:], host[4 * FS:])               # and its continuation elsewhere
    assert a.state(2) == b.state(5) == (4 * M.FSYMS, M.sign_parity(amd, fr))
    # states no modulator can be in
    for bad in ((0, 2, 0), (0, -1, 0), (0, 0, 1), (65536 * M.FSYMS + 1, 0, 0)):
        assert code_raised_by(amd, lambda: b.set_state(0, *bad)) == EINVAL
    assert code_raised_by(amd, lambda: b.set_state(7, 0, 0)) == EINVAL and code_raised_by(amd, lambda: b.reset(7)) == EINVAL
    assert b.state(0) == (0, 0)
    b.reset()
    assert all(b.state(s) == (0, 0) for s in range(7))
    assert out.canaries_intact() and (out.lane(3) == CANARY).all()
    a.close()
    b.close()
    d.close()


def test_far_positions_against_one_long_device_run(amd, dev):
    """opv_txb_set_state puts streams far into a run: one inside the flat-top bit zone (frame 1560: its 4 frames straddle
    symbols whose flat bit differs from a neighbour's), one across the end of the build-time checkpoint table (frame 4094) into
    the host continuation, one at frame 5. Each modulates 4 frames and == the matching slice of ONE opv_tx_modulate_device run
    of the whole length (existing code, held to `opv-mod` by tests/test_gpu_parity.py; 1.4 GB); the one at frame 5 also == the
    host modulator, so that the long run is not the only yardstick."""
    import torch
    total = 4098
    fr = stream_frames(amd, 9, total)
    par = np.concatenate([[0], np.cumsum(M.frame_parities(amd, fr)) & 1])    # sign parity in front of frame k
    # a start at or behind frame 1560 whose 4 frames hold a symbol whose flat bit differs from its neighbour's, on this libm
    zone = None
    for start in range(1560, 2000, 4):
        bits = M.flat_bits(M.symbol_phases(amd, start * M.FSYMS, 4 * M.FSYMS))
        if (bits[1:] != bits[:-1]).any():
            zone = start
            break
    assert zone is not None, "no flat-bit change found behind frame 1560"
    print("flat-bit zone start:", zone, "changes:", int((bits[1:] != bits[:-1]).sum()))
    starts = [zone, 4094, 5]
    d = amd.Demod(1, max_samples=1 << 16)
    bank = amd.TxBank(d, 4)
    out = Lanes(dev, 3, 4)
    for k, s in enumerate(starts):
        bank.set_state(k + 1, s * M.FSYMS, int(par[s]))
    patched = bank.round([3, 1, 2], [fr[starts[2]:starts[2] + 4], fr[starts[0]:starts[0] + 4], fr[starts[1]:starts[1] + 4]],
                         [out.ptr(2), out.ptr(0), out.ptr(1)])
    print("host-patched samples:", patched)
    for k, s in enumerate(starts):
        assert bank.state(k + 1) == ((s + 4) * M.FSYMS, int(par[s + 4])), s
    assert out.canaries_intact()
    assert np.array_equal(out.lane(2), amd.modulate(fr[:9])[2 * 5 * FS:2 * 9 * FS])
    long_run = torch.empty(2 * amd.lib().opv_tx_modulated_samples(total), dtype=torch.int16, device=dev)
    d.modulate_device(fr, long_run.data_ptr())
    for k, s in enumerate(starts):
        assert torch.equal(out.buf[GAP + k * (out.per + GAP):][:out.per], long_run[2 * s * FS:2 * (s + 4) * FS]), s
    del long_run
    bank.close()
    d.close()


def test_device_resident_frames_end_to_end(amd, dev):
    """A repeater: three clean 3-frame captures are demodulated in one context, slices of opv_device_frames go straight into
    the bank (frames_on_device), and what it writes == the host modulation of the popped frames; with the 4000 zero samples of
    the run's end behind it, a second context decodes the same 3 x 134 bytes per stream with metric 0."""
    import torch
    tx = [stream_frames(amd, 20 + k, 3) for k in range(3)]
    rx = amd.Demod(3, max_samples=1 << 19)
    for k in range(3):
        rx.push(k, amd.modulate(tx[k]))
        rx.flush(k)
    rx.process()
    rx.sync()
    assert [rx.state(k).frames_released for k in range(3)] == [3, 3, 3]
    d_frames, _, _, cap = rx.device_frames()
    n_out = 3 * FS + 4000
    out = torch.zeros((3, 2 * n_out), dtype=torch.int16, device=dev)
    bank = amd.TxBank(rx, 3)
    assert bank.round([2, 0, 1], [(d_frames + (s * cap) * 134, 3) for s in (2, 0, 1)], [out[s].data_ptr() for s in (2, 0, 1)],
                      on_device=True) >= 0
    popped = [rx.pop_frames(k)[0] for k in range(3)]
    for k in range(3):
        assert np.array_equal(popped[k], tx[k])
        assert np.array_equal(out[k].cpu().numpy(), amd.modulate(popped[k])), k     # (tail included: the zeros were there)
    bank.close()
    again = amd.Demod(3, max_samples=1 << 19)
    for k in range(3):
        again.attach(k, out[k].data_ptr(), n_out, eof=True)
    again.process()
    again.sync()
    for k in range(3):
        got, meta = again.pop_frames(k)
        assert np.array_equal(got, tx[k]) and meta["viterbi_metric"].tolist() == [0, 0, 0], k
    again.close()
    rx.close()


def test_misuse_leaves_everything_usable(amd, dev):
    """Every refusal between two good rounds: the good rounds' outputs == the host's, the state after a refused round is the
    state before it, nothing was written; a round against a bank whose context is gone answers OPV_ESTATE, and the bank can
    still be destroyed."""
    import ctypes as C
    fr = [stream_frames(amd, 30 + k, 2) for k in range(3)]
    d = amd.Demod(1, max_samples=1 << 16)
    bank = amd.TxBank(d, 3)
    out = Lanes(dev, 3, 2)
    assert bank.round([1, 0], [fr[1][:1], fr[0][:1]], [out.ptr(1), out.ptr(0)]) >= 0
    bank.set_state(2, (65536 - 1) * M.FSYMS, 1)
    before = [bank.state(s) for s in range(3)]
    snapshot = out.buf.clone()
    p0, p1, p2 = out.ptr(0, 1), out.ptr(1, 1), out.ptr(2)
    one = [fr[0][1:], fr[1][1:]]
    refused = [
        (EINVAL, lambda: bank.round([0, 3], one, [p0, p1])),                                 # stream out of range
        (EINVAL, lambda: bank.round([0, -1], one, [p0, p1])),
        (EINVAL, lambda: bank.round([0, 0], one, [p0, p1])),                                 # named twice
        (EINVAL, lambda: bank.round([0, 1], one, [p0 + 8, p1])),                             # misaligned
        (EINVAL, lambda: bank.round([0, 1], one, [p0, 0])),                                  # null output
        (EINVAL, lambda: bank.round([0, 1], [fr[0], fr[1][1:]], [out.ptr(0), out.ptr(0, 1)])),   # overlap
        (EINVAL, lambda: bank.round([0, 1], [(0, 1), (p1, 1)], [p0, p1], on_device=True)),   # null frames
        (ECAPACITY, lambda: bank.round([0, 2], [fr[0][1:], fr[2]], [p0, p2])),               # stream 2 would pass the run limit
    ]
    L = amd.lib()
    ids, nf = (C.c_int * 2)(0, 1), (C.c_size_t * 2)(1, 1)
    fp = (C.c_void_p * 2)(one[0].ctypes.data, one[1].ctypes.data)
    op = (C.c_void_p * 2)(p0, p1)
    raw = [(EINVAL, lambda: L.opv_txb_round(bank.h, -1, ids, fp, nf, op, 0)), (EINVAL, lambda: L.opv_txb_round(None, 2, ids, fp, nf, op, 0)),
           (EINVAL, lambda: L.opv_txb_round(bank.h, 2, None, fp, nf, op, 0)), (EINVAL, lambda: L.opv_txb_round(bank.h, 2, ids, None, nf, op, 0)),
           (EINVAL, lambda: L.opv_txb_round(bank.h, 2, ids, fp, None, op, 0)), (EINVAL, lambda: L.opv_txb_round(bank.h, 2, ids, fp, nf, None, 0))]
    for k, (want, call) in enumerate(refused):
        assert code_raised_by(amd, call) == want, k
        assert [bank.state(s) for s in range(3)] == before, k
    for k, (want, call) in enumerate(raw):
        assert call() == want, k
        assert [bank.state(s) for s in range(3)] == before, k
    import torch
    assert torch.equal(out.buf, snapshot)
    assert bank.round([], [], []) == 0 and bank.round([2, 1], [fr[2][:0], fr[1][:0]], [0, 0]) == 0   # nothing to do is not misuse
    assert [bank.state(s) for s in range(3)] == before and torch.equal(out.buf, snapshot)
    # the second good round
    assert bank.round([0, 1], one, [p0, p1]) >= 0
    for s in (0, 1):
        assert np.array_equal(out.lane(s), amd.modulate(fr[s])[:4 * FS]), s
    assert out.canaries_intact() and (out.lane(2) == CANARY).all()
    # the context goes first: the bank is detached
    after = [bank.state(s) for s in range(3)]
    d.close()
    assert code_raised_by(amd, lambda: bank.round([0], [fr[0][:1]], [p0])) == ESTATE
    assert code_raised_by(amd, lambda: bank.reset()) == ESTATE and code_raised_by(amd, lambda: bank.set_state(0, 0, 0)) == ESTATE
    assert [bank.state(s) for s in range(3)] == after
    bank.close()
