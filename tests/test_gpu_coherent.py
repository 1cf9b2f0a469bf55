"""k_coherent_frontend (csrc/k_coherent.hip, batch `-c`) held to the oracle beyond its 2000-symbol prefix, and the host code around
it (csrc/opv_capi.hip) held to its contract. The cases, the gain rule that says how far each can be followed and the envelope E that
says how closely are tests/coherent_inputs.py's, derived there from the oracle and the number formats alone;
tests/test_coherent_host.py asserts every case's condition on the CPU and pins the oracle to the compiled reference on all of them.

Per case, one batch context of one stream:
  state      est_offset_hz, total_symbols, total_samples, one chunk line with its remainder and symbol count: ==
  soft       |soft - oracle's| <= E(s) for every s < P (the whole capture in the tame regimes); beyond P the place where the
             trajectories part is printed, nothing asserted
  chunk line where P is the whole capture: fo within max(1, g) 1e-9 Hz, carrier and loop_freq within E(nsym) / M rad; == where the
             oracle's value sits on a clamp (+/-2000.0 Hz, +/-0.1)
  silence    soft == +0.0 exactly where the oracle's is
  tie        equal tone energies with signal in them (tie-dc): the upper tone drives the loop, as `en1 > en2` says
  back half  frames, metrics, release symbols, events == Oracle.track(the device's own soft log); in the tame regimes also the
             oracle's own frames, except those with a payload symbol within E of a quantiser boundary (at most one in four)
Context level: several streams per context (blockIdx.x > 0) bit-identical to each alone; three ways of delivery; process() before
flush and after the round; reset and reuse; `-s -c` takes the non-coherent path; every stream carries its own offset estimate.

What the module notices, tried on scratch builds of the library with one edit each to csrc/k_coherent.hip (never committed):
  AFC from `sym > 1` instead of `sym > 0`        29 tests: every case with afc_alpha != 0 and >= 2 symbols (edge-80 by its chunk
                                                 line alone), the three several-stream tests
  dominant tone by `en1 >= en2`                  tie-dc alone: on silence both correlations are +0.0 and the choice cannot be
                                                 seen; symbol 0 of a real constant at an estimate of exactly 0 Hz has
                                                 en1 == en2 != 0 (tests/test_coherent_host.py)
  loop_freq clamped in front of its update       loop-clamp and test_clamps_show_in_the_chunk_line
  `streams[0]` for `streams[blockIdx.x]`         test_six_streams_of_six_cases, test_seventy_streams,
                                                 test_every_stream_carries_its_own_offset_estimate
  carrier advanced by 39 loop_freq, not 40       42 tests: every case of two symbols or more with signal in it

The largest err / E per case is printed; OPV_COHERENT_PARITY_OUT=<file> writes the same lines there (profiles/coherent_parity.txt
is such a run's record)."""
import os

import numpy as np
import pytest

import coherent_inputs as CI
from fixtures import amd, torch_dev  # noqa: F401
from oracle_lib import format_events
from stream_runs import assert_same, new_acc, feed, result, state_tuple

pytestmark = pytest.mark.gpu

KERNEL = "k_coherent_frontend"
TAME = ("tame_frozen", "tame_afc", "tame_afc_clamped")
RECORD = []


@pytest.fixture(scope="module", autouse=True)
def record_file():
    yield
    out = os.environ.get("OPV_COHERENT_PARITY_OUT")
    if out and RECORD:
        with open(out, "w") as f:
            f.write("\n".join(RECORD) + "\n")


# ------------------------------------------------------------------ running streams
def context(amd, n_streams, setting, max_samples, **kw):
    return amd.Demod(n_streams, max_samples=max_samples + 64, streaming=False, coherent=True, afc_alpha=setting[0], pll_bw=setting[1], **kw)


def collect(d, s):
    fr, meta = d.pop_frames(s)
    st = d.state(s)
    return dict(frames=fr, meta=meta, events=d.pop_events(s), soft=d.soft(s), st=st, state=state_tuple(st), chunks=d.chunks(s))


def run_together(amd, xs, setting):
    """the captures xs as the streams of ONE batch context -> per-stream results, and the kernel's name"""
    d = context(amd, len(xs), setting, max(x.size // 2 for x in xs))
    for s, x in enumerate(xs):
        d.push(s, x)
        d.flush(s)
    d.process()
    d.sync()
    got = [collect(d, s) for s in range(len(xs))]
    kernel = d.frontend_kernel()
    d.close()
    return got, kernel


_ALONE = {}


def alone(amd, name):
    """the case's capture alone in a one-stream context (run once per module)"""
    if name not in _ALONE:
        c = CI.case(name)
        got, kernel = run_together(amd, [c["x"]], c["setting"])
        assert kernel == KERNEL
        _ALONE[name] = got[0]
    return _ALONE[name]


# ------------------------------------------------------------------ one stream against the oracle
def held_to_the_oracle(amd, c, got, tag, tame_name=None):
    """c: a case of coherent_inputs (case() / make()); got: collect()'s result. tame_name: the case's name where the oracle's own
    frames are asserted too."""
    st, n, nsym, P, E, M = got["st"], c["n"], c["nsym"], c["P"], c["E"], c["M"]
    soft = got["soft"]
    # state fields
    assert st.stalled == 0, (tag, st.stalled)
    assert st.est_offset_hz == c["est"], (tag, st.est_offset_hz, c["est"])
    assert st.total_symbols == n // 40 == len(soft) == nsym, (tag, st.total_symbols, len(soft), nsym)
    assert st.total_samples == n, (tag, st.total_samples, n)
    ch = got["chunks"]
    assert st.n_chunks == 1 and ch.shape == (1, 5), (tag, st.n_chunks, ch.shape)
    assert ch[0, 3] == n - 40 * nsym and ch[0, 4] == nsym, (tag, ch[0])
    # soft log inside the prefix
    err = np.abs(soft - c["soft"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(err == 0.0, 0.0, err / E[:nsym])
    at = int(np.argmax(ratio[:P])) if P else -1
    worst = float(ratio[at]) if P else 0.0
    scale = float(np.mean(np.abs(c["soft"]))) if nsym else 0.0
    part = np.nonzero(err > 1e-6 * scale)[0] if scale else np.zeros(0, int)
    line = (f"{tag}: afc_alpha {c['setting'][0]} pll_bw {c['setting'][1]}: {nsym} symbols, P {P}, gain at P {float(c['g'][P - 1]) if P else 0.0:.3g}; "
            f"max err/E over s < P {worst:.3f} at symbol {at}")
    if P:
        line += f" (err {err[at]:.3e} = {err[at] / scale:.2e} of mean |soft|)" if scale else ""
    if P < nsym:
        line += f"; beyond P: over 1e-6 of mean |soft| from symbol {int(part[0]) if part.size else None}"
    # chunk line
    fo, lf, ca = c["fin"]
    if c["whole"]:
        g_end = max(1.0, float(c["g"][-1])) if nsym else 1.0
        tol_fo, tol_ph = g_end * 1e-9, (E[nsym] / M if M else 0.0)
        d_fo, d_lf, d_ca = abs(ch[0, 0] - fo), abs(ch[0, 1] - lf), abs(ch[0, 2] - ca)
        line += f"; chunk line: fo off by {d_fo:.2e} Hz (allowed {tol_fo:.1e}), loop_freq {d_lf:.2e}, carrier {d_ca:.2e} rad (allowed {tol_ph:.1e})"
    print(line)
    RECORD.append(line)
    assert worst <= 1.0, line
    if c["whole"]:
        assert d_fo <= tol_fo and d_lf <= tol_ph and d_ca <= tol_ph, line
        if abs(fo) == CI.FO_CLAMP:
            assert ch[0, 0] == fo, (tag, ch[0, 0], fo)
        if abs(lf) == CI.LOOP_FREQ_CLAMP:
            assert ch[0, 1] == lf, (tag, ch[0, 1], lf)
        assert st.freq_offset_hz == ch[0, 0], (tag, st.freq_offset_hz, ch[0, 0])
    # silence: +0.0 exactly where the oracle has it (inside the prefix, where the two logs are the same trajectory)
    zero = c["soft"][:P] == 0.0
    assert np.array_equal(soft[:P] == 0.0, zero) and not np.any(np.signbit(soft[:P][zero])), tag
    # the back half over the device's own soft log
    t = CI.oracle().track(soft)
    keep = t["metrics"] >= 0
    assert np.array_equal(got["frames"], t["frames"][keep]), f"{tag}: decoded bytes differ from the tracker and decoder over the device's soft log"
    assert np.array_equal(got["meta"]["viterbi_metric"], t["metrics"][keep]), tag
    assert np.array_equal(got["meta"]["release_symbol"], t["frame_sym"][keep]), tag
    assert st.frames_released == len(t["metrics"]) and st.sync_state == t["final_state"], (tag, st.frames_released, st.sync_state)
    ev = got["events"]
    assert len(ev) == len(t["events"]), (tag, len(ev), len(t["events"]))
    for k in ("kind", "count", "sym_idx", "corr", "raw"):
        assert np.array_equal(ev[k], t["events"][k], equal_nan=(k in ("corr", "raw"))), (tag, k)
    assert amd.format_events(ev) == format_events(t["events"]), tag
    if tame_name is not None:
        T, fragile = CI.tracked(tame_name), CI.fragile_frames(tame_name)
        assert np.array_equal(t["frame_sym"], T["frame_sym"]), f"{tag}: released at {t['frame_sym']}, the oracle at {T['frame_sym']}"
        assert 4 * int(fragile.sum()) <= len(fragile), f"{tag}: {int(fragile.sum())} of {len(fragile)} frames sit on a quantiser boundary"
        sure = ~fragile
        assert np.array_equal(t["metrics"][sure], T["metrics"][sure]) and np.array_equal(t["frames"][sure], T["frames"][sure]), tag
        if not fragile.any():
            assert np.array_equal(got["frames"], c["exp"]["frames"]) and np.array_equal(got["meta"]["viterbi_metric"], c["exp"]["metrics"]), tag
        print(f"{tag}: {len(fragile)} frames released, {int(keep.sum())} decoded, {int(fragile.sum())} excluded by the boundary rule")
    return worst


@pytest.mark.parametrize("name", CI.CASES)
def test_case_against_the_oracle(amd, name):
    c = CI.case(name)
    held_to_the_oracle(amd, c, alone(amd, name), name, tame_name=name if CI.GROUP[name] in TAME else None)


def test_the_tame_cases_release_frames_on_the_device(amd):
    """what the frame comparison above compared: not empty lists"""
    per = {n: len(alone(amd, n)["frames"]) for g in TAME for n in CI.in_group(g)}
    assert max(per[n] for n in CI.in_group("tame_frozen")) >= 3 and sum(per[n] >= 2 for n in CI.in_group("tame_afc")) >= 2, per


def test_clamps_show_in_the_chunk_line(amd):
    """fo == +2000.0 and == -2000.0, loop_freq == +/-0.1: the exact values, from the device"""
    hi, lo, lc = alone(amd, "clamped-cut-hi"), alone(amd, "clamped-cut-lo"), alone(amd, "loop-clamp")
    assert hi["chunks"][0, 0] == 2000.0 and lo["chunks"][0, 0] == -2000.0, (hi["chunks"], lo["chunks"])
    assert abs(lc["chunks"][0, 1]) == 0.1 and lc["chunks"][0, 1] == CI.case("loop-clamp")["fin"][1], lc["chunks"]
    assert lc["chunks"][0, 3] == 17.0


def test_all_zero_capture(amd):
    c, got = CI.case("silence-zeros"), alone(amd, "silence-zeros")
    assert np.array_equal(got["soft"], np.zeros(300)) and not np.any(np.signbit(got["soft"]))
    assert len(got["frames"]) == 0 and len(got["events"]) == 0
    assert got["chunks"].tolist() == [[c["est"], 0.0, 0.0, 22.0, 300.0]], got["chunks"]


@pytest.mark.parametrize("cut", [0, 39])
def test_captures_below_one_symbol(amd, cut):
    got = alone(amd, f"edge-{cut}")
    assert got["st"].total_symbols == 0 and len(got["soft"]) == 0 and got["st"].stalled == 0
    assert got["chunks"].shape == (1, 5) and got["chunks"][0, 4] == 0.0 and got["chunks"][0, 3] == float(cut), got["chunks"]
    assert len(got["frames"]) == 0 and len(got["events"]) == 0


# ------------------------------------------------------------------ several streams per context
SIX = ["silence-gaps", "silence-zeros", "edge-0", "edge-41", "edge-86719", "f0+1440"]    # all at the tame-AFC setting


def test_six_streams_of_six_cases(amd):
    cases = [CI.case(n) for n in SIX]
    assert len(set(c["n"] for c in cases)) == 6 and cases[2]["n"] == 0 and all(c["setting"] == CI.AFC for c in cases)
    got, kernel = run_together(amd, [c["x"] for c in cases], CI.AFC)
    assert kernel == KERNEL
    for s, name in enumerate(SIX):
        assert_same(got[s], alone(amd, name), f"stream {s} ({name}) of six vs alone")
        held_to_the_oracle(amd, cases[s], got[s], f"six[{s}] {name}")


def test_seventy_streams(amd):
    """70 cuts of 100 .. 169 symbols of one tame capture, cut j starting 40 j samples in: more streams than one wave has lanes, every
    block index with a capture of its own"""
    x = CI.captures()["n300"]
    xs = [np.ascontiguousarray(x[2 * 40 * j: 2 * 40 * (j + 100 + j)]) for j in range(70)]
    assert [v.size // 80 for v in xs] == list(range(100, 170))
    cases = [CI.make(v, CI.AFC) for v in xs]
    assert all(c["whole"] for c in cases)
    got, kernel = run_together(amd, xs, CI.AFC)
    assert kernel == KERNEL
    worst = 0.0
    n = len(RECORD)
    for j in range(70):
        one, k1 = run_together(amd, [xs[j]], CI.AFC)
        assert k1 == KERNEL
        assert_same(got[j], one[0], f"stream {j} of seventy vs alone")
        worst = max(worst, held_to_the_oracle(amd, cases[j], got[j], f"seventy[{j}]"))
    del RECORD[n:]
    RECORD.append(f"seventy streams of 100 .. 169 symbols: largest err/E {worst:.3f}")
    assert len(set(g["soft"][:100].tobytes() for g in got)) == 70


def test_every_stream_carries_its_own_offset_estimate(amd):
    cases = [CI.case(n) for n in CI.OFFSETS]
    got, kernel = run_together(amd, [c["x"] for c in cases], CI.AFC)
    assert kernel == KERNEL
    est = [g["st"].est_offset_hz for g in got]
    assert est == [c["est"] for c in cases] and len(set(est)) == 4, est
    for s, name in enumerate(CI.OFFSETS):
        assert_same(got[s], alone(amd, name), f"stream {s} ({name}) of four vs alone")
        held_to_the_oracle(amd, cases[s], got[s], f"offsets[{s}] {name}")
    assert len(set(g["chunks"][0, 0] for g in got)) >= 2, [g["chunks"][0] for g in got]


# ------------------------------------------------------------------ delivery, a second process(), reset
DELIVERED = "afc-n300"
PIECES = [1, 39, 40, 4097, 100003, 41, 86720]


def test_three_ways_of_delivery(amd, torch_dev):
    torch, dev = torch_dev
    c, whole = CI.case(DELIVERED), alone(amd, DELIVERED)
    x, n = c["x"], c["n"]
    d = context(amd, 1, c["setting"], n)
    at, k = 0, 0
    while at < n:
        m = min(PIECES[k % len(PIECES)], n - at)
        d.push(0, x[2 * at: 2 * (at + m)])
        at, k = at + m, k + 1
    d.flush(0)
    d.process()
    d.sync()
    assert d.frontend_kernel() == KERNEL and k > 30
    assert_same(collect(d, 0), whole, "pushed in pieces, then flush vs pushed whole")
    d.close()
    d = context(amd, 1, c["setting"], n)
    t = torch.from_numpy(x.copy()).to(dev)
    torch.cuda.synchronize()
    d.attach(0, t.data_ptr(), n, eof=True)
    d.process()
    d.sync()
    assert d.frontend_kernel() == KERNEL
    assert_same(collect(d, 0), whole, "attach_device_iq(eof=1) vs pushed whole")
    d.close()


def test_process_before_flush_after_the_round_and_after_reset(amd):
    c, whole, other = CI.case(DELIVERED), alone(amd, DELIVERED), alone(amd, "silence-gaps")
    x, n = c["x"], c["n"]
    d = context(amd, 1, c["setting"], n)
    # not yet eof: nothing comes out - no symbols, no chunk line, no estimate taken from a part of the capture
    d.push(0, x[: 2 * 1000])
    d.process()
    d.sync()
    st = d.state(0)
    assert st.total_symbols == 0 and st.n_chunks == 0 and len(d.soft(0)) == 0 and len(d.pop_frames(0)[0]) == 0 and len(d.pop_events(0)) == 0
    d.push(0, x[2 * 1000:])
    d.process()
    d.sync()
    st = d.state(0)
    assert st.total_symbols == 0 and st.n_chunks == 0 and len(d.soft(0)) == 0 and len(d.pop_frames(0)[0]) == 0
    d.flush(0)
    d.process()
    d.sync()
    first = collect(d, 0)
    assert_same(first, whole, "process() twice before flush, then the round vs pushed whole")
    # after the round nothing changes
    for _ in range(2):
        d.process()
        d.sync()
        again = collect(d, 0)
        assert again["state"] == first["state"] and again["st"].n_chunks == 1
        assert again["soft"].tobytes() == first["soft"].tobytes() and again["chunks"].tobytes() == first["chunks"].tobytes()
        assert len(again["frames"]) == 0 and len(again["events"]) == 0            # (all popped above; none made again)
    # reset, the same capture: the same bits; reset, another capture: that capture's own
    for y, exp, what in ((x, whole, "the same capture after reset"), (CI.case("silence-gaps")["x"], other, "another capture after reset"),
                         (x, whole, "the first capture again")):
        d.reset(0)
        d.push(0, y)
        d.flush(0)
        d.process()
        d.sync()
        assert d.frontend_kernel() == KERNEL
        assert_same(collect(d, 0), exp, what)
    d.close()


def test_streaming_with_the_coherent_flag_takes_the_noncoherent_path(amd):
    """-s -c (tests/golden/c1_stream_coherent_flag_stderr.txt pins the CLI side): the flag is ignored, bit for bit"""
    x = CI.captures()["n300"][: 2 * (3 * 86720 + 12345)]
    n = x.size // 2
    res = []
    for coherent in (True, False):
        d = amd.Demod(1, max_samples=n + 64, streaming=True, coherent=coherent, pll_bw=35.0, afc_alpha=0.002)
        acc, names = new_acc(), set()
        for lo in range(0, n, 50021):
            feed(d, 0, x, lo, min(lo + 50021, n), acc, piece=50021)
            names.add(d.frontend_kernel())
        d.flush(0)
        d.process()
        d.sync()
        names.add(d.frontend_kernel())
        r = result(amd, d, 0, acc)
        r["state"] = state_tuple(r["state"])
        res.append(r)
        assert KERNEL not in names and all(k.startswith("k_msk_frontend") for k in names), names
        d.close()
    assert len(res[0]["soft"]) > 6000 and len(res[0]["chunks"]) >= 3
    assert_same(res[0], res[1], "-s -c vs -s")
