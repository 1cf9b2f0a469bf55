"""CPU-only: oracle/opv_oracle.c held to the COMPILED REFERENCE, live (oracle/_ref/libopv_ref.so), on every input class the GPU
parity tests are built on. Those tests compare the kernels with the oracle; on the classes below the oracle used to be the only
witness, so a misstatement of the reference there would have been tuned into the product with the suite green. The classes: the
hostile set of tests/test_gpu_mapping_matrix.py (tests/hostile_inputs.py: pathological inputs, slipping clocks, channel accidents,
silence gaps with and without one-tap windows, the AFC clamp, 3-4 LSB signals, a sub-sync-word capture), -s and batch; the
offset-search generators of tests/soak_inputs.py and the constructed ties of test_gpu_parity.py; the extreme -o / -a flag values;
the fuzz recipe; one slot of the 10 MS/s wideband plan's model output, whose zero tail shows one-tap windows; the decoder soak's
payloads; coherent mode on two hostile captures.

Every comparison is == : floats through their bits (.view(np.uint64)), est_offset NaN-aware; the tracker's lines as text against
the reference's own stderr. Nothing here is a tolerance, and nothing is compared with the product."""
import functools

import numpy as np
import pytest

from amd_lib import load
from hostile_inputs import (AFC_ALPHA_FLAG, EXTREME_FLAGS, ambiguous, assert_same_receive, assert_set_is_hostile, extreme_flags_capture,
                            fuzz_captures, hostile_captures, near_tie_captures, receive_pairs, staged_ties_capture)
from oracle_lib import Reference
from soak_inputs import decoder_payloads, offset_openings, symmetric_openings, weak_correlation_openings

pytestmark = pytest.mark.skipif(not Reference.available(), reason="oracle/_ref/libopv_ref.so not built")

SEED = 20261003
HOSTILE_NAMES = [f"patho{k}" for k in range(8)] + ["slip-25000", "slip-3000", "slip+3000", "slip+25000"] + \
    [f"accident{k}" for k in (0, 5, 6, 7)] + ["gaps_nudged", "gaps_as_drawn", "clamp+2600", "edge-1990", "lsb_2_chunks", "short"] + \
    [f"ord{k}_{F}f" for k, F in enumerate((1, 5, 3, 5, 8, 12, 4, 7, 2, 9))]


@pytest.fixture(scope="module")
def ref():
    return Reference()


# ------------------------------------------------------------------ 1. the hostile set
@pytest.fixture(scope="module")
def hostile(oracle):
    built = hostile_captures(oracle)
    return dict(names=[b[0] for b in built], classes=[b[1] for b in built], caps=[np.ascontiguousarray(b[2]) for b in built], exp={})


def hostile_pairs(hostile, keys):
    """(oracle's, reference's) result for every (capture, streaming) of keys: computed once each, what is missing over worker
    processes at one go"""
    missing = [k for k in keys if k not in hostile["exp"]]
    if missing:
        hostile["exp"].update(zip(missing, receive_pairs([(hostile["caps"][j], dict(streaming=s)) for j, s in missing])))
    return [hostile["exp"][k] for k in keys]


def test_the_hostile_set_is_what_it_claims(hostile):
    """test_gpu_mapping_matrix's non-vacuity conditions, from the oracle's output alone: the oracle that the captures below pin is
    the one that says what the set is for. (Both receivers run over the whole set here, -s and batch; the tests below compare.)"""
    assert hostile["names"] == HOSTILE_NAMES
    n = len(hostile["caps"])
    mine = [a for a, _ in hostile_pairs(hostile, [(j, s) for s in (True, False) for j in range(n)])]
    assert_set_is_hostile(hostile["names"], hostile["classes"], hostile["caps"], mine[:n], mine[n:])


@pytest.mark.parametrize("streaming", [True, False], ids=["stream", "batch"])
@pytest.mark.parametrize("j", range(len(HOSTILE_NAMES)), ids=HOSTILE_NAMES)
def test_hostile_capture(hostile, j, streaming):
    assert hostile["names"][j] == HOSTILE_NAMES[j]
    a, b = hostile_pairs(hostile, [(j, streaming)])[0]
    assert_same_receive(a, b, f"{HOSTILE_NAMES[j]} streaming={streaming}")


@pytest.mark.parametrize("name", ["patho0", "slip+3000"])
def test_hostile_capture_coherent_mode(hostile, oracle, ref, name):
    """-c on two of them, as test_oracle_golden.test_coherent_live_against_reference_class: the Costas loop is chaotic, so only the
    reference's own arithmetic, libm results included, follows it"""
    x = hostile["caps"][HOSTILE_NAMES.index(name)]
    a = oracle.receive(x, streaming=False, coherent=True, pll_bw=35.0, afc_alpha=0.002)
    b = ref.receive(x, streaming=False, coherent=True, pll_bw=35.0, afc_alpha=0.002)
    assert len(a["soft"]) == x.size // 2 // 40
    assert_same_receive(a, b, f"-c {name}")


# ------------------------------------------------------------------ 2. the offset search
GENERATORS = {"offset": (offset_openings, 32), "symmetric": (symmetric_openings, 32), "weak": (weak_correlation_openings, 24)}


@functools.lru_cache(maxsize=None)
def openings(kind):
    """the generator's first openings (its captures are drawn one after the other, so a shorter run is a prefix of a longer one):
    the first eight kinds by index are in, mirror ties and digital silence among them"""
    gen, n = GENERATORS[kind]
    return gen(SEED, n)


@pytest.mark.parametrize("kind,first", [(k, f) for k, (_, n) in GENERATORS.items() for f in range(0, n, 8)])
def test_offset_search_on_the_soak_generators(oracle, ref, kind, first):
    caps = openings(kind)[first: first + 8]
    assert len(caps) == 8
    got = [(oracle.estimate_offset(x), ref.estimate_offset(x)) for x in caps]
    assert all(a == b for a, b in got), (kind, first, got)
    if kind == "symmetric" and first == 0:
        assert any(abs(a) == 1530.0 for a, _ in got), got                       # (an exact mirror tie drags the fine pass to an edge)


def test_offset_search_on_the_constructed_ties(oracle, ref, iq10):
    """the captures of test_offset_search_near_tie_guard and of test_more_ties_in_one_round_than_the_host_passes_stage"""
    got = [(oracle.estimate_offset(x), ref.estimate_offset(x)) for x in near_tie_captures(iq10) + [staged_ties_capture()]]
    assert all(a == b for a, b in got), got
    assert sum(abs(a) == 1530.0 for a, _ in got) >= 5, got


# ------------------------------------------------------------------ 3. flags, fuzz, the wideband model's output, the decoder
@pytest.mark.parametrize("off,alpha", EXTREME_FLAGS)
def test_extreme_flag_values(oracle, ref, iq10, off, alpha):
    x = extreme_flags_capture(iq10)
    a = oracle.receive(x, streaming=True, init_offset=off, afc_alpha=alpha)
    assert_same_receive(a, ref.receive(x, streaming=True, init_offset=off, afc_alpha=alpha), f"-o {off} -a {alpha}")


def test_afc_alpha_flag(oracle, ref, iq10):
    a = oracle.receive(iq10, streaming=True, afc_alpha=AFC_ALPHA_FLAG)
    assert_same_receive(a, ref.receive(iq10, streaming=True, afc_alpha=AFC_ALPHA_FLAG), f"-a {AFC_ALPHA_FLAG}")


@pytest.mark.parametrize("seed", [SEED + s for s in range(4)])
def test_fuzz_recipe(iq10, iq100, seed):
    """test_clock_rate_error_and_random_channels_fuzz's 24 captures of one seed, -s and batch (both receivers over worker
    processes: 48 runs of each)"""
    caps = fuzz_captures(seed, iq10, iq100)
    assert len(caps) == 24
    keys = [(k, s) for k in range(24) for s in (True, False)]
    leftovers = set()
    for (k, s), (a, b) in zip(keys, receive_pairs([(caps[k], dict(streaming=s)) for k, s in keys])):
        assert_same_receive(a, b, f"fuzz seed {seed} capture {k} streaming={s}")
        if s:
            leftovers.update(int(v) for v in a["chunks"][:-1, 3])
    assert len(leftovers) >= 8, leftovers                  # (as in the GPU test: the clock errors really moved the chunk grid)


@pytest.fixture(scope="module")
def wideband_slot():
    """slot 0 of the 10 MS/s plan (wideband_device.PLAN_10M) as the numpy model (wideband_models.wbr_model) says the door
    delivers it: a clean channel that is digitally silent behind its two frames"""
    from wideband_device import PLAN_10M, make_plan_wide_10m, plan_taps_10m
    from wideband_models import wbr_model, wbr_model_inc
    amd = load()
    amd.build()
    wide, _tx = make_plan_wide_10m(amd, 2)
    inc = wbr_model_inc(PLAN_10M["down"], PLAN_10M["up"], PLAN_10M["centres"][:1])
    return wbr_model(amd.wb_lo_table(), wide, PLAN_10M["down"], PLAN_10M["up"], inc, plan_taps_10m(), PLAN_10M["out_shift"])[0]


@pytest.mark.parametrize("streaming", [True, False], ids=["stream", "batch"])
def test_wideband_model_output_with_one_tap_windows(oracle, ref, wideband_slot, streaming):
    """the class where the product deviates by design (edge_ties) and the oracle alone says what is right"""
    a = oracle.receive(wideband_slot, streaming=streaming)
    amb = ambiguous(a["soft"])
    assert len(a["frames"]) == 2 and (not streaming or (amb.size >= 1 and amb[0] >= 2 * 2168)), (len(a["frames"]), amb)
    assert_same_receive(a, ref.receive(wideband_slot, streaming=streaming), f"wideband slot 0 streaming={streaming}")


def test_decoder_payloads_of_all_eight_kinds(oracle, ref):
    soft = decoder_payloads(400, SEED)
    dropped = 0
    for k, s in enumerate(soft):
        a = oracle.frame_decode(s)
        m, frame = ref.frame_decode(s)
        assert a["metric"] == m and np.array_equal(a["frame"], frame), (k, k % 8, a["metric"], m)
        dropped += m < 0
    assert 0 < dropped < len(soft) // 8, dropped            # (only some of the payloads around the 1e-10 threshold are dropped)
