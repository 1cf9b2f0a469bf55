"""GPU: which lane of k_msk_frontend_rb's helper wave writes which fp64 ring entry (csrc/k_frontend.hip, f64_ring_helper: lane l
converts samples fill + l + 64 k of a chunk) must not show in any result. Every case below runs on the fp64 ring (this process,
the automatic shape while a context has no more streams than the device has CUs), on the int16 ring (OPV_FRONTEND_INT16_RING=1 is
read by opv_create: ONE child process started with it runs all cases once, module fixture) and through the CPU oracle:

  fp64 ring == int16 ring   bit for bit, per round: soft symbols, the per-call carry {fo, tf, mu, leftover, nsym}, the stream
                            state, frames, Viterbi metrics, tracker events (stream_runs.assert_same)
  fp64 ring vs the oracle   stream_checks.check_stream in full (frames, metrics, sync positions, events, symbol count, every
                            soft symbol < SOFT_TIGHT, carry), nothing stalled
  overflow == 0             opv_get_state / opv_pop_frames fail on a stream whose hand-over timed out (overflow = 2)

Shapes, chosen for where a wrong lane-to-sample mapping, zero fill or last difference shows:
  lengths   L0 + r samples, L0 = 391 x 256 (one whole 86 720-sample call, then an EOF tail), r in R: n mod 4 takes 0, 1, 2, 3 and
            n mod 128 / n mod 256 take 0, 1, 127, 129, 255 (and 128, 2, 130): the capture ends on a chunk boundary, one sample
            past it, one before it, and the same around the half chunk. One stream per context, and three streams of three
            different lengths per context.
  six       three 6-frame captures (524 320 samples: the 2048-entry ring wraps 256 times), whole
  pieces    the same three captures pushed 100 003 samples at a time with opv_process in between: a launch starts at an origin
            that is no multiple of the chunk, and the helper's first chunk starts below origin - 11
  tails     whole calls followed by an EOF tail shorter than one 256-sample chunk (37, 100, 200 samples), a 60-sample capture
            (the first symbol of a call and nothing else) and a 50-sample one (no symbol at all)"""
import os
import pickle
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

from amd_lib import load
from fixtures import amd  # noqa: F401
from stream_checks import check_stream
from stream_runs import CHUNK, assert_same, base_capture, collect_unstalled

pytestmark = pytest.mark.gpu
L0 = 391 * 256
R = (0, 1, 2, 127, 128, 129, 130, 255)
PIECE = 100003
ENV = "OPV_FRONTEND_INT16_RING"


def make_cases(amd):
    """name -> (captures, samples per push or None for the whole capture at once)"""
    two = [base_capture(amd, frames=2, seed=50 + s, sigma=250.0 + 25.0 * s) for s in range(3)]
    six = [base_capture(amd, frames=6, seed=60 + s, sigma=250.0 + 25.0 * s) for s in range(3)]
    assert all(c.size // 2 >= L0 + 256 for c in two) and all(c.size // 2 >= 6 * CHUNK for c in six)
    cases = {}
    for r in R:
        cases[f"len1_{r}"] = ([two[0][: 2 * (L0 + r)]], None)
    for i in range(0, len(R), 3):                           # (0, 1, 2) (127, 128, 129) (130, 255, 0)
        rs = [R[(i + j) % len(R)] for j in range(3)]
        cases["len3_" + "_".join(map(str, rs))] = ([two[j][: 2 * (L0 + rs[j])] for j in range(3)], None)
    cases["six"] = (six, None)
    cases["pieces"] = (six, PIECE)
    cases["tails"] = ([two[0][: 2 * (CHUNK + 37)], two[1][: 2 * (2 * CHUNK + 100)], two[2][: 2 * (CHUNK + 200)]], None)
    cases["sixty"] = ([two[0][: 2 * 60]], None)
    cases["fifty"] = ([two[0][: 2 * 50]], None)
    return cases


def run_case(amd, captures, piece):
    """one context; per round (one opv_process) the results of every stream"""
    S = len(captures)
    caps = [c.reshape(-1, 2) for c in captures]
    n = [c.shape[0] for c in caps]
    d = amd.Demod(S, max_samples=max(n) + 64, streaming=True)
    try:
        rounds, at = [], 0
        while True:
            m = max(n) - at if piece is None else min(piece, max(n) - at)
            for s in range(S):
                if at < n[s]:
                    d.push(s, caps[s][at: min(at + m, n[s])])
                    if at + m >= n[s]:
                        d.flush(s)
            at += m
            d.process()
            d.sync()
            assert d.frontend_kernel() == "k_msk_frontend_rb"
            rounds.append([collect_unstalled(d, s) for s in range(S)])
            if at >= max(n):
                return rounds
    finally:
        d.close()


def run_all(amd, cases):
    return {name: run_case(amd, caps, piece) for name, (caps, piece) in cases.items()}


@pytest.fixture(scope="module")
def rings(amd, tmp_path_factory):
    """every case on the fp64 ring (here) and on the int16 ring (one child process for all of them)"""
    assert ENV not in os.environ
    cases = make_cases(amd)
    tmp = tmp_path_factory.mktemp("ring_layout")
    with open(tmp / "cases.pkl", "wb") as f:
        pickle.dump(cases, f)
    p = subprocess.Popen([sys.executable, str(Path(__file__).resolve()), str(tmp / "cases.pkl"), str(tmp / "int16.pkl")],
                         env={**os.environ, ENV: "1"}, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    f64 = run_all(amd, cases)                              # (while the child runs)
    out, _ = p.communicate(timeout=300)
    assert p.returncode == 0, out[-2000:]
    with open(tmp / "int16.pkl", "rb") as f:
        i16 = pickle.load(f)
    return dict(cases=cases, f64=f64, i16=i16)


_ORACLE = {}


def oracle_of(capture):
    from oracle_lib import Oracle
    key = capture.tobytes()
    if key not in _ORACLE:
        if "o" not in _ORACLE:
            _ORACLE["o"] = Oracle()
        _ORACLE[key] = _ORACLE["o"].receive(capture, streaming=True, want_soft=True)
    return _ORACLE[key]


class State:
    def __init__(self, amd, values):
        for (f, _), v in zip(amd.StreamState._fields_, values):
            setattr(self, f, v)


def check_case(amd, rings, name):
    captures, _piece = rings["cases"][name]
    a, b = rings["f64"][name], rings["i16"][name]
    assert len(a) == len(b)
    for r, (ra, rb) in enumerate(zip(a, b)):
        for s in range(len(captures)):
            assert_same(ra[s], rb[s], f"{name}: round {r} stream {s}")
    for s, cap in enumerate(captures):
        exp = oracle_of(cap)
        last = a[-1][s]
        got = dict(frames=np.concatenate([ro[s]["frames"] for ro in a]), meta=np.concatenate([ro[s]["meta"] for ro in a]),
                   events=np.concatenate([ro[s]["events"] for ro in a]), soft=last["soft"], chunks=last["chunks"],
                   state=State(amd, last["st"]))
        tag = f"{name}: stream {s} ({cap.size // 2} samples)"
        if exp["n_soft"] == 0:                             # nothing to scale a soft error by
            assert last["total_symbols"] == 0 and len(got["soft"]) == 0 and len(got["frames"]) == 0 and len(exp["frames"]) == 0, tag
            assert len(got["events"]) == len(exp["events"]) and len(got["chunks"]) == len(exp["chunks"]), tag
            assert np.array_equal(got["chunks"][:, 3:], exp["chunks"][:, 3:]), tag
            continue
        check_stream(amd, got, exp, tag, edge_ties=0, offset_ties=None)
    return a


@pytest.mark.parametrize("streams", [1, 3])
def test_capture_lengths_around_the_chunk(amd, rings, streams):
    names = [k for k in rings["cases"] if k.startswith(f"len{streams}_")]
    assert len(names) == (len(R) if streams == 1 else 3)
    seen = set()
    for name in names:
        got = check_case(amd, rings, name)
        seen |= {c.size // 2 for c in rings["cases"][name][0]}
        assert all(len(st["chunks"]) == 2 and st["total_symbols"] > 2400 for st in got[-1]), name   # one whole call + the EOF tail
    assert {n % 4 for n in seen} == {0, 1, 2, 3} and {0, 1, 127, 129, 255} <= {n % 256 for n in seen}
    assert {0, 1, 127} <= {n % 128 for n in seen}


def test_six_frames_the_ring_wraps_250_times(amd, rings):
    got = check_case(amd, rings, "six")
    assert all(c.size // 2 // 2048 >= 250 for c in rings["cases"]["six"][0])
    assert sum(len(st["frames"]) for st in got[-1]) >= 12


def test_six_frames_in_pieces_of_100003(amd, rings):
    """... and the pushed run's final soft log and carry are the whole run's, bit for bit"""
    got = check_case(amd, rings, "pieces")
    assert len(got) == 6 and PIECE % 256 != 0
    whole = rings["f64"]["six"][-1]
    for s in range(3):
        assert got[-1][s]["soft"].tobytes() == whole[s]["soft"].tobytes(), s
        assert got[-1][s]["chunks"].tobytes() == whole[s]["chunks"].tobytes(), s


def test_short_eof_tails_and_no_symbol(amd, rings):
    got = check_case(amd, rings, "tails")
    assert [len(st["chunks"]) for st in got[-1]] == [2, 3, 2]
    got = check_case(amd, rings, "sixty")
    assert got[-1][0]["total_symbols"] == 1                 # (the reference's loop runs while pos + 50 < n: the first symbol alone)
    got = check_case(amd, rings, "fifty")
    assert got[-1][0]["total_symbols"] == 0 and len(got[-1][0]["chunks"]) == 1


if __name__ == "__main__":                                 # the int16-ring child of the `rings` fixture
    assert os.environ.get(ENV) == "1"
    _amd = load()
    _amd.lib()
    with open(sys.argv[1], "rb") as _f:
        _cases = pickle.load(_f)
    _res = run_all(_amd, _cases)
    with open(sys.argv[2], "wb") as _f:
        pickle.dump(_res, _f)
