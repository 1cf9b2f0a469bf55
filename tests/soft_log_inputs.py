"""Made soft-symbol logs for the back half of the receive chain (tracker, scale pre-pass, in-context decoder).

A test INPUT generator, like soak_inputs.py: nothing here is a reference. A "frame" is the 24 sync symbols `pattern * a`
followed by oracle.encode_frame(payload) mapped to +/-a (coded bit 0 -> +a), with optional Gaussian noise. The edge cases come
as PAIRS, one log on each side of a tracker decision; every value that decides an edge is a small integer, so every window sum is
exact in fp64 whatever the order of additions, and the two sides differ by ONE in one symbol.

    logs = all_logs(oracle)          # {name: Log}; names of a pair end in ".yes" / ".no"
    decoder_edge_payloads(oracle)    # (names, [n, 2144] payloads) for the decoder alone

Log.soft is the log, Log.cuts the symbol counts at which a caller should also cut it into calls (first-sync alignments),
Log.note says what the log is for."""
from dataclasses import dataclass, field

import numpy as np

SYNC_WORD = 0x02B8DB
SYNC_BITS = 24
CODED = 2144
FSYMS = 2168
PATTERN = np.array([-1.0 if (SYNC_WORD >> (SYNC_BITS - 1 - i)) & 1 else 1.0 for i in range(SYNC_BITS)])
A = 500.0                                       # amplitude of an ordinary frame: raw = 12 000, norm = 1


@dataclass
class Log:
    soft: np.ndarray
    note: str = ""
    cuts: list = field(default_factory=list)
    marks: dict = field(default_factory=dict)   # named symbol positions a test wants to know


def sync(mags=A, flip=()):
    """24 sync symbols of the given magnitude(s); positions in `flip` carry the wrong sign"""
    m = np.broadcast_to(np.asarray(mags, np.float64), (SYNC_BITS,)).copy()
    s = PATTERN * m
    for i in flip:
        s[i] = -s[i]
    return s


def mags_of(groups):
    """[(count, value), ...] -> 24 magnitudes"""
    m = np.concatenate([np.full(c, float(v)) for c, v in groups])
    assert m.size == SYNC_BITS, m.size
    return m


_PAYLOADS = {}


def payload(oracle, k, a=A, sigma=0.0, rng=None):
    """the 2144 coded symbols of BERT frame k at amplitude a"""
    if k not in _PAYLOADS:
        _PAYLOADS[k] = oracle.encode_frame(oracle.bert_frames(1, first=k)[0]).astype(np.float64)
    s = (1.0 - 2.0 * _PAYLOADS[k]) * a
    if sigma:
        s = s + sigma * rng.standard_normal(CODED)
    return s


def frame(oracle, k, a=A, sync_syms=None, sigma=0.0, rng=None):
    s = sync(a) if sync_syms is None else np.asarray(sync_syms, np.float64)
    if sigma:
        s = s + sigma * rng.standard_normal(SYNC_BITS)
    return np.concatenate([s, payload(oracle, k, a, sigma, rng)])


def cat(*parts):
    return np.ascontiguousarray(np.concatenate([np.atleast_1d(np.asarray(p, np.float64)) for p in parts]))


def zeros(n):
    return np.zeros(n, np.float64)


def pair(logs, name, yes, no, note, cuts=()):
    logs[name + ".yes"] = Log(yes, note, list(cuts))
    logs[name + ".no"] = Log(no, note, list(cuts))


# ------------------------------------------------------------------------------------------------ (a) HUNTING acceptance
def hunting_logs(o):
    logs = {}
    lead = 40

    def one(sync_syms, a):
        return cat(zeros(lead), sync_syms, payload(o, 0, a), frame(o, 1, a, sync_syms=sync(a)), zeros(30))
    # raw 5000 / 4999 with norm = 1: 23 x 208 + 216 = 5000. The payload (24 x 208 = 4992 of energy per window) can never pass
    # raw >= 5000 by itself, and neither can the second frame's clean sync word: the .no side stays HUNTING to its end.
    pair(logs, "a.raw5000", one(sync(mags_of([(23, 208), (1, 216)])), 208.0), one(sync(mags_of([(23, 208), (1, 215)])), 208.0),
         "HUNTING: raw == 5000.0 is accepted, 4999.0 is not (norm = 1)")
    # norm 6800/8000 / 6798/8000, raw well above 5000: one symbol of 600 / 601 with the wrong sign, the other 23 add up to 7400 / 7399
    pair(logs, "a.norm085", one(sync(mags_of([(1, 600), (17, 322), (6, 321)]), flip=(0,)), 322.0),
         one(sync(mags_of([(1, 601), (17, 322), (5, 321), (1, 320)]), flip=(0,)), 322.0),
         "HUNTING: norm 6800/8000 == 0.85 is accepted, 6798/8000 is not")
    # the same ten times larger: raw = 67 980, an order above its threshold, and norm still just below 0.85
    # (the wrong-signed symbol sits in the middle of the word: at these amplitudes a window that holds nothing but one or two
    # symbols of the right sign has raw >= 5000 and norm = 1 - see a.lone_symbol)
    pair(logs, "a.rawhigh", one(sync(np.roll(mags_of([(1, 6000), (17, 3220), (6, 3210)]), 11), flip=(11,)), 3220.0),
         one(sync(np.roll(mags_of([(1, 6010), (17, 3220), (5, 3210), (1, 3200)]), 11), flip=(11,)), 3220.0),
         "HUNTING: raw = 67 980 does not make up for norm 67980/80000 < 0.85")
    # one strong symbol in silence IS a sync word to SyncTracker: the window that ends on it has raw = 6000 = energy. The next 23
    # windows would pass too: the first wins.
    logs["a.lone_symbol"] = Log(cat(zeros(40), [6000.0 * PATTERN[23]], zeros(2200), frame(o, 0), frame(o, 1), zeros(30)),
                                "HUNTING: a single symbol of 6000 in silence is accepted (24 windows in a row pass, the first wins)")
    return logs


# ------------------------------------------------------------------------------------------------ (b) LOCKED check
def locked_logs(o):
    logs = {}

    def one(slot):
        return cat(zeros(7), frame(o, 0), slot, payload(o, 1), frame(o, 2), frame(o, 3), zeros(30))
    pair(logs, "b.norm070", one(sync(mags_of([(3, 500), (16, 405), (5, 404)]), flip=(0, 1, 2))),
         one(sync(mags_of([(2, 500), (1, 501), (15, 405), (6, 404)]), flip=(0, 1, 2))),
         "LOCKED: 7000/10000 == 0.70 passes the check, 6998/10000 is a miss")
    pair(logs, "b.energy100", one(sync(mags_of([(20, 4), (4, 5)]))), one(sync(mags_of([(21, 4), (3, 5)]))),
         "LOCKED: energy == 100.0 passes the gate (norm = 1), 99.0 gives norm = 0, a miss")
    pair(logs, "b.silent", one(sync(mags_of([(20, 4), (4, 5)]))), one(zeros(SYNC_BITS)),
         "LOCKED: a silent sync slot (energy 0) is a miss with corr = 0")
    return logs


# ------------------------------------------------------------------------------------------------ (c) miss counter
def miss_logs(o):
    logs = {}
    inverted = -sync(A)                                                     # norm = -1
    half = sync(mags_of([(24, 100)]), flip=tuple(range(6)))                 # 1200 / 2400 = 0.5
    bad = [zeros(SYNC_BITS), inverted, half, zeros(SYNC_BITS), inverted]    # norms 0, -1, 0.5, 0, -1

    def run(n_bad, after):
        parts = [zeros(3), frame(o, 0)]
        for k in range(n_bad):
            parts += [bad[k], payload(o, 1 + k)]
        return cat(*parts, *after)
    good = [frame(o, 7), frame(o, 8), zeros(30)]
    pair(logs, "c.four_five", run(4, good), run(5, good),
         "four misses then a good sync word: the counter starts again, the flywheel frames carry sync_ok = 0 and the miss's norm "
         "(0, -1, 0.5, 0); a fifth miss: LOST_LOCK, nothing pending is released")
    # after LOST_LOCK at symbol c: a clean word ending at c + 1 (its first 23 symbols ARE the fifth slot, one symbol late) ...
    late1 = cat(zeros(3), frame(o, 0), *[p for k in range(4) for p in (bad[k], payload(o, 1 + k))],
                payload(o, 9)[:1], frame(o, 7), frame(o, 8), zeros(30))
    # ... and one ending at c + 23: its first symbol is the slot's last
    late23 = cat(zeros(3), frame(o, 0), *[p for k in range(4) for p in (bad[k], payload(o, 1 + k))],
                 zeros(23), frame(o, 7), frame(o, 8), zeros(30))
    pair(logs, "c.relock_next", late1, run(5, [zeros(40)]),
         "a clean sync word ending on the very next symbol after LOST_LOCK is taken at once")
    pair(logs, "c.relock_23", late23, run(5, [zeros(40)]),
         "a clean sync word ending 23 symbols after LOST_LOCK (its window starts at the LOST_LOCK symbol)")
    return logs


# ------------------------------------------------------------------------------------------------ (d) first sync position
def first_sync_logs(o):
    logs = {}
    body = cat(payload(o, 0), frame(o, 1), frame(o, 2), zeros(30))
    for end in (22, 23, 24, 86, 87):
        s = cat(zeros(max(0, end - 23)), sync(A)[max(0, 23 - end):], body)
        # cuts: the accepted window's last symbol is the last of a call / the first of the next; the window over two and three calls
        logs["d.first%d" % end] = Log(s, "the first sync word ends at symbol %d" % end, [end + 1, end, max(1, end - 11), max(2, end - 5)])
    pair(logs, "d.lane63_64", logs["d.first86"].soft, logs["d.first87"].soft,
         "the hit in lane 63 of the first scan step (symbol 23 + 63) and in lane 0 of the second (23 + 64)", [64, 86, 87, 88])
    both = cat(zeros(17), sync(A), zeros(6), sync(A), body)                 # words ending at 40 and 70: one 64-wide step sees both
    second = cat(zeros(17 + SYNC_BITS), zeros(6), sync(A), body)
    pair(logs, "d.two_in_step", both, second, "two accepted windows inside one 64-symbol span: the first wins", [41, 71])
    return logs


# ------------------------------------------------------------------------------------------------ (e) embedded sync words
def embedded_logs(o):
    logs = {}

    def one(embed_verifying, embed_locked):
        p0, p1 = payload(o, 0).copy(), payload(o, 1).copy()
        if embed_verifying:
            p0[1000:1000 + SYNC_BITS] = sync(A)
        if embed_locked:
            p1[700:700 + SYNC_BITS] = sync(A)
        return cat(zeros(5), sync(A), p0, sync(A), p1, frame(o, 2), zeros(30))
    pair(logs, "e.embedded", one(True, True), one(False, False),
         "a full-strength sync word inside the payload while VERIFYING and while LOCKED is ignored: same events either way")
    # last symbols of the two embedded words, and a cut behind the sync word in front of each (from where a HUNTING tracker sees it)
    logs["e.embedded.yes"].marks = dict(verifying_end=5 + 24 + 1000 + 23, verifying_from=100,
                                        locked_end=5 + FSYMS + 24 + 700 + 23, locked_from=5 + FSYMS + 24 + 100)
    # a stray word at symbol 50 is a false anchor: the tracker then looks 2168 symbols later, where the .yes side has a word
    # embedded in the (off-grid) real frame's payload - and keeps following the false grid
    def false_anchor(embed):
        real = cat(frame(o, 0), frame(o, 1), frame(o, 2), frame(o, 3), frame(o, 4), frame(o, 5), frame(o, 6), frame(o, 7), frame(o, 8))
        s = cat(zeros(27), sync(A), zeros(700), real, zeros(30))
        if embed:
            at = 50 + FSYMS - 23
            s[at:at + SYNC_BITS] = sync(A)
        return s
    pair(logs, "e.false_anchor", false_anchor(True), false_anchor(False),
         "a sync word embedded 2168 symbols after a false anchor passes the LOCKED check there")
    return logs


# ------------------------------------------------------------------------------------------------ (f) non-finite values
def nonfinite_logs(o):
    logs = {}
    for name, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
        w = sync(A)
        w[11] = v
        p = payload(o, 1).copy()
        p[[0, 1, 777, 2143]] = v
        # frame 0's word is spoilt (HUNTING passes over it), frame 1 is taken, frame 2's word is spoilt (LOCKED: a miss whose
        # corr is NaN), frame 3's payload holds the value
        s = cat(zeros(9), w, payload(o, 0), frame(o, 1), w, payload(o, 2), sync(A), p, frame(o, 4), zeros(30))
        logs["f." + name] = Log(s, "%s inside a sync window in HUNTING and in LOCKED, and inside a payload" % name)
    return logs


# ------------------------------------------------------------------------------------------------ (g) decoder edge values
def decoder_edge_payloads(o, seed=7):
    """(names, [n, 2144]) real coded frames and noise carrying the values the front-end never produces"""
    rng = np.random.default_rng(seed)
    clean = payload(o, 3)
    noisy = payload(o, 4, sigma=400.0, rng=rng)
    noise = 300.0 * rng.standard_normal(CODED)
    sparse = rng.choice(CODED, 9, replace=False)
    names, rows = [], []

    def add(name, p):
        names.append(name)
        rows.append(np.asarray(p, np.float64))
    for base_name, base in (("clean", clean), ("noisy", noisy), ("noise", noise)):
        for vname, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
            p = base.copy()
            p[sparse] = v
            add("%s+%s" % (base_name, vname), p)
        p = base.copy()
        p[sparse[:4]] = np.inf
        p[sparse[4:]] = -np.inf
        add(base_name + "+both_inf", p)
        add(base_name + "*1.7e308", base / np.max(np.abs(base)) * 1.7e308)           # the running sum overflows
        add(base_name + "*denormal", np.sign(base) * 5e-324 * np.rint(np.abs(base) / 100.0 + 1.0))   # all denormal: dropped
        p = base.copy()
        p[0::2] = -0.0
        add(base_name + "+negzero", p)
    for at, v in ((0, 1.0), (1071, -3.0e300), (2143, 1e-7)):                      # |soft / scale| = 2144, the stated bound
        p = zeros(CODED)
        p[at] = v
        add("single@%d" % at, p)
    add("equal+", np.full(CODED, 123.0))                                           # every value on a quantiser boundary
    add("equal-", np.full(CODED, -7.0e-3))
    add("equal_signed", np.sign(clean) * 0.1)
    # two levels 6 u and 8 u, half and half: scale = 7 u, so 3.5 soft / scale is +/-3 or +/-4 and EVERY value sits on a
    # quantiser boundary (the kernel's guard band); u = 0.1 is not a dyadic number, so the quotient is rounded
    lv = np.where(np.arange(CODED) % 2 == 0, 6.0, 8.0)
    add("boundary*1", np.sign(clean) * lv)
    add("boundary*0.1", np.sign(clean) * lv * 0.1)
    add("boundary_noise*3e-5", np.sign(noise) * lv[::-1] * 3e-5)
    add("clean", clean)                                                            # (the ordinary case, for the branch census)
    add("zeros", zeros(CODED))
    return names, np.ascontiguousarray(np.stack(rows))


def decoder_edge_log(o):
    """the same payloads as frames of one log (clean sync words, so that the tracker releases every one of them)"""
    names, pl = decoder_edge_payloads(o)
    return names, Log(cat(zeros(11), *[cat(sync(A), p) for p in pl], zeros(30)), "decoder edge values as payloads of a tapped log")


# ------------------------------------------------------------------------------------------------ (h) a seeded walk
def walk_log(o, seed=2026):
    """40 frames, 86 720 symbols: noise per frame, erased and inverted sync words placed so that all five event kinds occur
    (four misses in a row and a recovery; five in a row, LOST_LOCK and a new hunt), the rest at random"""
    rng = np.random.default_rng(seed)
    parts = []
    for k in range(40):
        sigma = float(rng.choice([0.0, 60.0, 150.0, 300.0, 450.0]))
        w = sync(A)
        if 8 <= k < 12 or rng.random() < 0.08:
            w = zeros(SYNC_BITS) if rng.random() < 0.5 else 0.2 * w
        if 20 <= k < 25:
            w = -w
        parts.append(frame(o, k, sync_syms=w, sigma=sigma, rng=rng))
    return Log(cat(*parts), "seeded 40-frame walk through all five event kinds")


def long_log(o, n_frames=130, seed=99):
    """n_frames noisy frames with every seventh sync word erased: more tracker lines than a context's event ring holds"""
    rng = np.random.default_rng(seed)
    parts = [zeros(10)]
    for k in range(n_frames):
        parts.append(frame(o, k % 50, sync_syms=zeros(SYNC_BITS) if k % 7 == 5 else None, sigma=120.0, rng=rng))
    return Log(cat(*parts), "a long run for back-pressure and the lossy event ring")


def counted_log(o, n_release, seed):
    """a log that ends on the release symbol of its n_release-th frame (n_release = 0: noise too weak to be a sync word)"""
    rng = np.random.default_rng(seed)
    if n_release == 0:
        return Log(3.0 * rng.standard_normal(3001), "releases nothing")
    lead = int(rng.integers(1, 200))
    s = cat(zeros(lead), *[frame(o, int(rng.integers(0, 50)), sigma=200.0, rng=rng) for _ in range(n_release)])
    return Log(s, "releases %d frames" % n_release)


def all_logs(o):
    logs = {}
    for make in (hunting_logs, locked_logs, miss_logs, first_sync_logs, embedded_logs, nonfinite_logs):
        logs.update(make(o))
    logs["h.walk"] = walk_log(o)
    return logs
