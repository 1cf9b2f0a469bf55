"""Inputs the scan's tests share (tests/test_scan_host.py, tests/test_gpu_scan.py): the made rows opv_scan_carriers is held to
carriers_model on, and the end-to-end plan - three BERT channels of the D = 4 plan (wideband_device.PLAN_D4) whose carriers sit
kHz off their nominal centres, under wideband noise - with its CPU half. numpy and the oracle only: importing needs no device."""
import numpy as np

from oracle_lib import impair
from scan_model import carriers_model, hann_window, scan_model
from wideband_device import PLAN_D4, plan_taps_d4
from wideband_models import WIDE_RATE, wb_model, wb_model_inc, wbr_model_inc


# ------------------------------------------------------------------ rows for opv_scan_carriers
def carrier_cases():
    """-> [(name, row uint64, f0_hz, step_hz, half_width_hz, ratio_q8, cap)]"""
    rng = np.random.default_rng(2024)
    cases = []

    def noise(P, scale=1000):
        return rng.integers(scale, 2 * scale, P).astype(np.uint64)
    # two equal peaks far apart: a tie in box, the lower index first
    row = np.full(101, 500, np.uint64)
    row[20:23] = [7000, 90000, 7000]
    row[70:73] = [7000, 90000, 7000]
    cases.append(("tie_in_box", row, -1e6, 20000.0, 40000.0, 512, 4))
    # peaks at both ends of the row: boxes with fewer terms
    row = noise(64)
    row[0], row[1], row[63], row[62] = 10 ** 7, 3 * 10 ** 6, 2 * 10 ** 7, 10 ** 6
    cases.append(("both_ends", row, -4.336e6, 16937.5, 60000.0, 1024, 3))
    # a flat row: floor = every value, no excess anywhere
    cases.append(("flat_strict", np.full(33, 12345, np.uint64), 0.0, 1000.0, 2500.0, 256, 5))       # box x 256 == ratio x n x floor: no candidate
    cases.append(("flat_loose", np.full(33, 12345, np.uint64), 0.0, 1000.0, 2500.0, 255, 5))        # every probe ties: index order, den = 0
    # floor = 0: a noise-free capture, every probe with power is a candidate and cap bounds the list
    row = np.zeros(200, np.uint64)
    row[[10, 11, 12]] = [5, 900, 40]
    row[[150, 151]] = [300, 300]
    row[199] = 1
    cases.append(("floor_zero", row, 1e5, 8468.75, 17000.0, 4096, 2))
    cases.append(("floor_zero_all", row, 1e5, 8468.75, 17000.0, 4096, 200))
    # ratio_q8 <= 256: every probe passes wherever its box is above the floor's share
    row = noise(80)
    row[40] = 10 ** 6
    cases.append(("ratio_256", row, -3e5, 5000.0, 10000.0, 256, 8))
    cases.append(("ratio_0", row, -3e5, 5000.0, 10000.0, 0, 80))
    # two peaks closer than 2 W share a box: one carrier between them (the boxes that hold one of them alone lie within 2 W of it and
    # are skipped), and a third peak further out is kept
    row = noise(128)
    row[50], row[55], row[90] = 10 ** 6, 9 * 10 ** 5, 4 * 10 ** 5
    cases.append(("closer_than_2w", row, 0.0, 16937.5, 60000.0, 512, 3))
    # cap smaller than the candidates, and no room at all
    cases.append(("cap_1", row, 0.0, 16937.5, 60000.0, 512, 1))
    cases.append(("cap_0", row, 0.0, 16937.5, 60000.0, 512, 0))
    # rows near 2^61 (one block at its bound) and sums of rows up to 2^64 - 1
    row = (np.uint64(1 << 61) - rng.integers(0, 1 << 40, 96).astype(np.uint64))
    row[30] = np.uint64(1 << 61)
    cases.append(("near_2_61", row, -1e6, 21000.0, 45000.0, 256, 4))
    row = rng.integers(1 << 62, (1 << 63) - 1, 1024).astype(np.uint64) * np.uint64(2) + np.uint64(1)
    row[700] = np.uint64((1 << 64) - 1)
    cases.append(("near_2_64", row, -4.336e6, 8468.75, 60000.0, 256, 6))
    # a half width beyond the row, half width 0, the smallest rows
    row = noise(40)
    row[7] = 10 ** 5
    cases.append(("w_beyond_row", row, 0.0, 100.0, 1e9, 300, 3))
    cases.append(("w_zero", row, 0.0, 100.0, 0.0, 300, 3))
    cases.append(("p_1", np.array([77], np.uint64), 5.0, 1.0, 1.0, 0, 3))
    cases.append(("p_2", np.array([77, 3], np.uint64), 5.0, 1.0, 1.0, 100, 3))
    for k in range(6):                                                       # random rows, random rule
        P = int(rng.integers(3, 1025))
        row = noise(P, int(rng.integers(1, 10 ** 6)))
        for at in rng.integers(0, P, int(rng.integers(0, 6))):
            row[at] *= np.uint64(rng.integers(2, 500))
        cases.append((f"random_{k}", row, float(rng.uniform(-5e6, 5e6)), float(rng.uniform(10.0, 40000.0)), float(rng.uniform(0.0, 200000.0)),
                      int(rng.integers(0, 4096)), int(rng.integers(1, 12))))
    return cases


# ------------------------------------------------------------------ the end-to-end plan
# Slots 0 - 2 of PLAN_D4 (8.672 MS/s; nominal centres -1.1, 0.0 and +1.6 MHz, the door's 321-tap filter and shift), but the carriers sit
# `off_hz` from their nominal centres - outside the reference's -1500 .. +1500 Hz coarse search - at unequal amplitudes, and white
# noise is added to the WIDE capture (not per channel: a channel's own noise, repeated by D, would be a pedestal 2.168 MHz wide under
# its peak and not a floor), so that the median of a row is a noise floor: its density puts the weakest channel, slot 1, at Eb/N0 =
# `ebn0_db` under oracle_lib.impair's definition (variance 80 amp^2 / 10^(Eb/N0 / 10) per 2.168 MHz), the others 6 and 9.5 dB above.
# The scan: 512 probes across Fw (16.94 kHz apart), a 1024-tap integer Hann window, hop 1024, the first `scan_samples` of the
# capture (75.6 ms: ten blocks of 64 segments; over the first 30 ms alone the model's centroids lie up to 1 kHz off, over 75 ms
# within 500 Hz), rows summed; carriers: boxes of +/-60 kHz, a candidate at 2 x the floor, cap 3. The third carrier sits 15 250 Hz
# off: at +11 250 and +13 250 Hz the oracle fed the NOMINAL centre still released (wrong) frames, at +15 250 Hz it releases none.
SCAN_PLAN = dict(frames=2, centres=PLAN_D4["centres"][:3], off_hz=[7300.0, -4100.0, 15250.0], amp=[3000.0, 1000.0, 2000.0],
                 ebn0_db=12.0, seed=91, scan_samples=10 * 64 * 1024,
                 n_probes=512, n_window=1024, hop=1024, n_avg=64, out_shift=22, half_width_hz=60000.0, ratio_q8=512)


def scan_plan_probes():
    fw = PLAN_D4["D"] * WIDE_RATE
    step = fw / SCAN_PLAN["n_probes"]
    return -fw / 2, step, -fw / 2 + step * np.arange(SCAN_PLAN["n_probes"], dtype=np.float64)


def make_scan_capture(amd):
    """-> dict(wide, tx[k], true_hz[k]): the capture, built like wideband_device.make_plan_capture_d4"""
    D, fs = PLAN_D4["D"], PLAN_D4["D"] * WIDE_RATE
    p = SCAN_PLAN
    tx, z = [], None
    for k, nominal in enumerate(p["centres"]):
        tx.append(amd.bert_frames(p["frames"], "SC%d" % k, first=10 * k))
        iq = impair(amd.modulate(tx[k]), amp=p["amp"][k])
        zk = np.repeat(iq[0::2].astype(np.float64) + 1j * iq[1::2].astype(np.float64), D)
        zk = zk * np.exp(2j * np.pi * (nominal + p["off_hz"][k]) / fs * np.arange(zk.size, dtype=np.float64))
        z = zk if z is None else z + zk
    rng = np.random.default_rng(p["seed"])
    sd = np.sqrt(D * 80.0 * min(p["amp"]) ** 2 / 10.0 ** (p["ebn0_db"] / 10.0) / 2.0)
    z = z + sd * (rng.standard_normal(z.size) + 1j * rng.standard_normal(z.size))
    assert max(np.max(np.abs(z.real)), np.max(np.abs(z.imag))) < 32767
    wide = np.empty(2 * z.size, np.int16)
    wide[0::2], wide[1::2] = np.rint(z.real), np.rint(z.imag)
    return dict(wide=wide, tx=tx, true_hz=[c + o for c, o in zip(p["centres"], p["off_hz"])])


def scan_plan_rows_model(amd, wide):
    """scan_model's rows of the plan's scan on the capture's first scan_samples: uint64 [10][512]"""
    p = SCAN_PLAN
    wide = wide[: 2 * p["scan_samples"]]
    _, _, probes = scan_plan_probes()
    inc = wbr_model_inc(PLAN_D4["D"], 1, probes)
    return scan_model(amd.wb_lo_table(), wide, inc, hann_window(p["n_window"]), p["hop"], p["n_avg"], p["out_shift"])


def scan_plan_carriers(rows, carriers=carriers_model):
    """the plan's carrier rule on the sum of `rows`: [(centre_hz, probe, excess)] in ascending centre_hz (slot order)"""
    p = SCAN_PLAN
    f0, step, _ = scan_plan_probes()
    total = rows.sum(axis=0, dtype=np.uint64)
    return sorted(carriers(total, f0, step, p["half_width_hz"], p["ratio_q8"], 3))


def door_streams_on_the_cpu(amd, oracle, wide, centres):
    """wb_model at `centres` and the oracle on each slot: -> (model[k] int16 IQ, exp[k])"""
    D = PLAN_D4["D"]
    model = wb_model(amd.wb_lo_table(), wide, D, wb_model_inc(D, centres), plan_taps_d4(), PLAN_D4["out_shift"])
    return model, [oracle.receive(model[k], streaming=True) for k in range(len(centres))]
