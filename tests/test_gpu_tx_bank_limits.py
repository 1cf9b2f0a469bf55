"""GPU: the transmit bank (csrc/k_tx_bank.hip, csrc/opv_tx_bank.hip) at the launch shapes tests/test_gpu_tx_bank.py never
leaves the smallest of, held the same way: `==` on int16 samples against the host modulator (runs from symbol 0) or
tests/tx_bank_model.py's samples() (streams put elsewhere; pinned by tests/test_tx_bank_host.py), the state after every round
`==` the model's, every canary intact.

  a. 261 entries in one round (65 full scan workgroups of four waves and one of a single wave, owner searches over 261 rows,
     stream indices above 255), between a round of 5 - so the bank's scratch grows - and rounds of 4 and 1 that continue its
     streams, one from frames that lie in device memory at byte offsets that are no multiple of 4
  b. entries of 129, 65, 64 and 1 frames: the scan's second and third trip of 64 frames, with the carry changing between them
  c. entries that start and end on, one symbol in front of and one behind a 128-symbol checkpoint, from symbol positions that
     are no frame starts

Frames are drawn bytes: the BERT frames of one stream of the other module all have the same on-air parity
(tx_bank_runs.drawn_frames), so only here do the parities within an entry differ. Every test first asserts from the model or
the plan, on the CPU, that its inputs reach the edge it is named after. The ambiguous-sample path is not here: no sample of a
run of 65 536 frames comes nearer than 1.9e-3 to a non-zero integer without being a flat top
(scripts/experiments/tx_find_ambiguous.py; NOTEBOOK.md, transmit chain), so no input reaches it and every round answers 0."""
import numpy as np
import pytest

import tx_bank_model as M
from fixtures_built import amd  # noqa: F401
from tx_bank_runs import FS, Lanes, drawn_frames
from tx_bank_runs import dev  # noqa: F401

pytestmark = pytest.mark.gpu


def parity_of(bits):
    return int(np.sum(bits) & 1)


def intervals(first_symbol, n_symbols):
    """txb_intervals (csrc/opv_txb_rules.h), restated: 128-symbol checkpoint intervals that the symbols touch"""
    first_symbol, n_symbols = np.asarray(first_symbol, np.int64), np.asarray(n_symbols, np.int64)
    return (first_symbol + n_symbols - 1) // M.CKPT_SYMS - first_symbol // M.CKPT_SYMS + 1


# ------------------------------------------------------------------------------------------------ a. many entries per round
def test_261_entries_in_one_round_on_a_scratch_that_grows(amd, dev):
    """A bank of 300 streams, eight of them put at frames below 64 with both parities, four rounds on one scratch: 5 entries;
    261 non-empty ones in shuffled stream order (ten of two frames) with zero-frame entries first, last and in the middle;
    4 entries from device-resident frames at odd multiples of 134 bytes; 1 entry. Rounds 3 and 4 continue streams of round 2,
    with carried parities 0 and 1, the 1 in a stream above 255."""
    import torch
    N = 300
    order = np.random.default_rng(300).permutation(N).tolist()
    call2 = order[:264]
    counts2 = [0 if i in (0, 130, 263) else 2 if i % 26 == 7 else 1 for i in range(264)]
    call1 = [call2[1], call2[200], order[264], call2[100], order[265]]
    start = {call2[i]: (f, k & 1) for k, (i, f) in enumerate(zip([3, 7, 50, 100, 150, 200, 250, 262], [1, 3, 16, 31, 40, 47, 58, 63]))}
    frames = [drawn_frames(1000 + s, 5) for s in range(N)]
    fp = [M.frame_parities(amd, f) for f in frames]

    def model_state(s, done):
        f0, p0 = start.get(s, (0, 0))
        return (f0 + done) * M.FSYMS, (p0 + parity_of(fp[s][:done])) & 1

    # rounds 3 and 4 are chosen by what the model says the streams of round 2 carry behind it
    after2 = {s: model_state(s, n + (s in call1))[1] for s, n in zip(call2, counts2) if n}
    plain = [s for s in after2 if s not in start and s not in call1]
    high1 = [s for s in plain if s > 255 and after2[s] == 1]
    low0 = [s for s in plain if s < 256 and after2[s] == 0]
    call3, counts3 = [high1[0], low0[0], call2[50], call2[33]], [1, 1, 1, 2]
    call4, counts4 = [high1[1]], [1]
    rounds = [(call1, [1] * 5, False), (call2, counts2, False), (call3, counts3, True), (call4, counts4, False)]
    # ---- what the test is named after, from the plan and the model
    assert [sum(n > 0 for n in c) for _, c, _ in rounds] == [5, 261, 4, 1] and 261 == 65 * 4 + 1
    assert counts2[0] == counts2[130] == counts2[-1] == 0 and counts2.count(2) == 10 and counts2.count(1) == 251
    assert call2 != sorted(call2) and sum(s > 255 for s, n in zip(call2, counts2) if n) >= 30
    assert len(start) == 8 and {p for _, p in start.values()} == {0, 1} and all(0 < f < 64 for f, _ in start.values())
    assert set(call3 + call4) <= set(after2) and counts2[33] == 2 and call2[50] in start
    assert {after2[s] for s in call3 + call4} == {0, 1} and call3[0] > 255 and call4[0] > 255 and after2[call3[0]] == after2[call4[0]] == 1
    assert {int(v) for s in range(N) for v in fp[s]} == {0, 1}
    total = [0] * N
    for streams, counts, _ in rounds:
        for s, n in zip(streams, counts):
            total[s] += n
    assert max(total) <= 5 and sum(total) == 5 + 271 + 5 + 1
    d = amd.Demod(1, max_samples=1 << 16)
    bank = amd.TxBank(d, N)
    out = Lanes(dev, N, total)
    for s, (f0, p0) in start.items():
        bank.set_state(s, f0 * M.FSYMS, p0)
    done = [0] * N
    for r, (streams, counts, on_device) in enumerate(rounds):
        ptrs = [out.ptr(s, done[s]) if n or i == 130 else 0 for i, (s, n) in enumerate(zip(streams, counts))]
        if r == 1:                                                           # the grid of the large round, as the host plans it
            fb, fs = amd.txb_plan_round([model_state(s, done[s]) for s in range(N)], streams, counts, ptrs)
            assert fb[-1] == 34 * sum(counts) == 34 * 271 and fs.tolist() == [model_state(s, done[s])[0] for s in streams]
        chunks = [frames[s][done[s]:done[s] + n] for s, n in zip(streams, counts)]
        if on_device:
            # one device tensor, every entry's frames at an odd multiple of 134 bytes: a multiple of 2 and never of 4
            at, offs = 1, []
            for c in chunks:
                offs.append(134 * at)
                at += len(c)
                at += 1 - at % 2
            assert all(o % 134 == 0 and o % 4 == 2 for o in offs)
            host = np.full(134 * at, 0xEE, np.uint8)
            for o, c in zip(offs, chunks):
                host[o:o + c.size] = c.reshape(-1)
            d_frames = torch.from_numpy(host).to(dev)
            assert d_frames.data_ptr() % 4 == 0
            chunks = [(d_frames.data_ptr() + o, len(c)) for o, c in zip(offs, chunks)]
        assert bank.round(streams, chunks, ptrs, on_device=on_device) == 0, r
        for s, n in zip(streams, counts):
            done[s] += n
        for s in range(N):                                                   # streams not named stand still
            assert bank.state(s) == model_state(s, done[s]), (r, s)
    assert done == total
    for s in range(N):
        if s in start:
            want = M.samples(amd, frames[s][:total[s]], start[s][0] * M.FSYMS, start[s][1])
        else:
            want = amd.modulate(frames[s][:total[s]])[:2 * total[s] * FS]
        assert np.array_equal(out.lane(s), want), s
    assert out.canaries_intact()
    bank.close()
    d.close()


# ------------------------------------------------------------------------------------------------ b. long entries
LONG_SEED, SEED_65, SEED_64, SEED_1 = 2, 5, 6, 7                             # drawn_frames seeds whose parities the test asserts


def test_entries_of_129_65_64_and_1_frames(amd, dev):
    """One round with entries of 65, 129, 1 and 64 frames. The 129 go into a stream that a round of one frame left at parity 1;
    their first 64 and their next 64 frames are both of odd parity, so the scan's carry is 0 at base 64 and 1 again at base 128,
    where frame 128 sits alone in a third trip. The 65 frames start at parity 0 and have carry 1 at base 64: the last frame's
    sign hangs on it. (Seeds, not callsigns and tokens: a BERT stream's frames all have one parity, and 64 of them are even.) The single frame goes
    into a stream put at frame 40 with parity 1 and is held to the model, the runs from symbol 0 to the host modulator."""
    long, f65, f64, one = drawn_frames(LONG_SEED, 130), drawn_frames(SEED_65, 65), drawn_frames(SEED_64, 64), drawn_frames(SEED_1, 1)
    pl, p65 = M.frame_parities(amd, long), M.frame_parities(amd, f65)
    carried = int(pl[0])
    at64 = carried ^ parity_of(pl[1:65])
    at128 = at64 ^ parity_of(pl[65:129])
    assert (carried, at64, at128) == (1, 0, 1)                               # every `carry ^=` of the long entry changes the carry
    assert parity_of(p65[:64]) == 1                                          # the 65 frames: carry 1 at base 64, carried 0
    d = amd.Demod(1, max_samples=1 << 16)
    bank = amd.TxBank(d, 6)
    out = Lanes(dev, 4, [130, 65, 64, 1])
    assert out.buf.numel() * 2 < 100e6
    bank.set_state(5, 40 * M.FSYMS, 1)
    assert bank.round([4], [long[:1]], [out.ptr(0)]) == 0
    assert bank.state(4) == (M.FSYMS, 1) and bank.state(5) == (40 * M.FSYMS, 1)
    assert bank.round([0, 4, 5, 2], [f65, long[1:], one, f64], [out.ptr(1), out.ptr(0, 1), out.ptr(3), out.ptr(2)]) == 0
    assert bank.state(4) == (130 * M.FSYMS, M.sign_parity(amd, long)) and bank.state(0) == (65 * M.FSYMS, M.sign_parity(amd, f65))
    assert bank.state(2) == (64 * M.FSYMS, M.sign_parity(amd, f64)) and bank.state(5) == (41 * M.FSYMS, M.sign_parity(amd, one, 1))
    assert bank.state(1) == bank.state(3) == (0, 0)
    for lane, fr in enumerate((long, f65, f64)):
        assert np.array_equal(out.lane(lane), amd.modulate(fr)[:2 * len(fr) * FS]), lane
    assert np.array_equal(out.lane(3), M.samples(amd, one, 40 * M.FSYMS, 1))
    assert out.canaries_intact()
    bank.close()
    d.close()


# ------------------------------------------------------------------------------------------------ c. checkpoint-interval edges
def test_entries_on_and_beside_checkpoints(amd, dev):
    """One round of eleven streams put by opv_txb_set_state at symbols 16 x 2168 = 271 x 128 (on a checkpoint; with either
    parity), one in front of and one behind it, 15 x 2168 (the frame ends on a checkpoint), 16 x 2168 - 119 (the first position
    from which a frame reaches into an 18th interval: 2168 = 16 x 128 + 120, so it touches 18 exactly when it starts 9 or more
    symbols into one), 8 x 2168 with 8 frames (starts half-way through an interval, ends on a checkpoint; 271 workgroups of
    k_txb_modulate and no partial one), 127, 128, 129, and 1 (right behind the silent symbol). The frame-aligned ones also ==
    the slice of one 17-frame run of the host modulator."""
    F = M.FSYMS
    run = drawn_frames(17, 17)
    before = np.concatenate([[0], np.cumsum(M.frame_parities(amd, run)) & 1]).astype(int)   # sign parity in front of frame k
    assert set(before[[8, 15, 16]].tolist()) == {0, 1}
    # (stream, first symbol, sign parity, frames, frame of `run` it continues or None)
    cases = [(3, 16 * F, before[16], run[16:], 16), (9, 16 * F - 1, 1, drawn_frames(31, 1), None), (0, 16 * F + 1, 0, drawn_frames(32, 1), None),
             (7, 15 * F, before[15], run[15:16], 15), (1, 8 * F, before[8], run[8:16], 8), (10, 127, 1, drawn_frames(33, 1), None),
             (4, 128, 0, drawn_frames(34, 1), None), (2, 129, 1, drawn_frames(35, 1), None), (8, 1, 0, drawn_frames(36, 1), None),
             (5, 16 * F - 119, 0, drawn_frames(37, 1), None), (6, 16 * F, 1 - before[16], run[16:], None)]
    firsts, counts = [c[1] for c in cases], [len(c[3]) for c in cases]
    assert 16 * F == 271 * 128 and (15 * F + F) % 128 == 0 and (16 * F - 119) % 128 == 9 and 8 * F == 271 * 64 and 8 * F % 128 == 64
    ivl = intervals(firsts, np.array(counts) * F).tolist()
    assert ivl == [17, 18, 17, 17, 136, 18, 17, 17, 17, 18, 17]
    assert [v for f, n, v in zip(firsts, counts, ivl) if n == 1 and f % 128 == 0] == [17, 17, 17]
    pairs = set(zip(ivl, ivl[1:]))
    assert (17, 18) in pairs and (18, 17) in pairs and sum(ivl) == 4 * 64 + 53   # both next to each other in the grid; four workgroups and a partial one
    streams = [c[0] for c in cases]
    assert sorted(streams) == list(range(11)) and streams != sorted(streams)
    d = amd.Demod(1, max_samples=1 << 16)
    bank = amd.TxBank(d, 12)
    out = Lanes(dev, 11, counts)
    for s, first, par, _, _ in cases:
        bank.set_state(s, first, int(par))
    fb, fs = amd.txb_plan_round([bank.state(s) for s in range(12)], streams, counts, [out.ptr(k) for k in range(11)])
    assert fs.tolist() == firsts and fb[5] - fb[4] == 271 and fb[-1] == 34 * 10 + 271
    assert bank.round(streams, [c[3] for c in cases], [out.ptr(k) for k in range(11)]) == 0
    host = amd.modulate(run)[:2 * 17 * FS]
    for k, (s, first, par, fr, at) in enumerate(cases):
        assert bank.state(s) == (first + len(fr) * F, M.sign_parity(amd, fr, int(par))), k
        got = out.lane(k)
        assert np.array_equal(got, M.samples(amd, fr, first, int(par))), k
        if at is not None:
            assert np.array_equal(got, host[2 * at * FS:2 * (at + len(fr)) * FS]), k
    assert bank.state(11) == (0, 0) and out.canaries_intact()
    bank.close()
    d.close()
