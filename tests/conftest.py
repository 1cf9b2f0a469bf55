import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


# The suite's wall clock against the driver's limits (900 s for `pytest -m gpu`, a few minutes for `-m "not gpu"`): every run
# ends with its total and its ten slowest tests, whatever the flags (the same list `--durations=10` would print; here it cannot be
# forgotten). Nothing is asserted - DESIGN.md section 4 states the current totals.
_T0 = {}
_DUR = {}


def _start_clock():
    import time
    _T0["t"] = time.time()


# Wall-clock guard for `-m gpu`. Tests that start PYTHON child processes (ranks over gloo / RCCL, bench.py under the launcher) cost
# 2 - 20 s each on a box whose image is paged in and 30 - 120 s each on a cold one (measured: the same suite 351 s and 886 s on two boxes
# of the pool, profiles/r06_gpu_suite*.txt) - and the driver kills the suite at 900 s, which would take the parity tests down with
# them. So (1) those rehearsal tests run LAST, in order of what they prove, behind every parity test; (2) one of them is skipped - with
# the reason - once less than 200 s of the limit remain (a cold-box run of one took up to 121 s). On a warm box they start at ~300 s
# and nothing is skipped; on the cold box of the record the last three would have been, and the suite would have ended at ~700 s.
# OPV_SUITE_LIMIT_S overrides the 900 s.
_LATE = ["test_world2_real_pipeline_every_global_stream_vs_oracle", "test_real_pipeline_rank_code_under_nccl_world_1",
         "test_gather_frames_under_nccl_world_1", "test_worldN_real_pipeline_over_rccl_every_global_stream_vs_oracle",
         "test_bench_world2_under_the_drivers_launcher", "test_bench_world2_started_from_a_bare_shell",
         "test_bench_worldN_over_rccl_under_the_drivers_launcher", "test_bench_world2_a_dead_rank_takes_the_job_down",
         "test_bench_plain_run_is_lean_and_dumps_what_it_decoded"]
# (test_bench_rccl_leg_executes_at_world_1 is not one of them: it only reads what the session-start child already did)
_LATE_RESERVE_S = 200.0


def _late_rank(item):
    name = item.name.split("[")[0]
    return _LATE.index(name) if name in _LATE else -1


def pytest_collection_modifyitems(config, items):
    early = [i for i in items if _late_rank(i) < 0]
    late = sorted((i for i in items if _late_rank(i) >= 0), key=lambda i: (_late_rank(i), i.name))     # (stable within a test: [2] before [4])
    items[:] = early + late


def pytest_runtest_setup(item):
    import os
    import time
    if _late_rank(item) < 0 or item.get_closest_marker("gpu") is None:
        return
    limit = float(os.environ.get("OPV_SUITE_LIMIT_S", "900"))
    gone = time.time() - _T0.get("t", time.time())
    if gone > limit - _LATE_RESERVE_S:
        pytest.skip(f"suite wall-clock guard: {gone:.0f} s of the driver's {limit:.0f} s are gone and this rehearsal test starts Python child "
                    f"processes (up to ~125 s on a cold box); the parity tests ran first")


def pytest_runtest_logreport(report):
    _DUR[report.nodeid] = _DUR.get(report.nodeid, 0.0) + report.duration      # setup + call + teardown


def pytest_terminal_summary(terminalreporter, exitstatus, config):
    import time
    if not _DUR:
        return
    total = time.time() - _T0.get("t", time.time())
    expr = config.getoption("markexpr", "") or ""
    limit = 900.0 if ("gpu" in expr and "not gpu" not in expr) else None
    tr = terminalreporter
    tr.write_sep("-", "wall clock")
    tr.write_line(f"session {total:.0f} s" + (f" of the driver's {limit:.0f} s for `-m gpu` ({100.0 * total / limit:.0f} %)" if limit else "") +
                  f"; tests alone {sum(_DUR.values()):.0f} s; the ten slowest:")
    for nodeid, d in sorted(_DUR.items(), key=lambda kv: -kv[1])[:10]:
        tr.write_line(f"  {d:7.1f} s  {nodeid}")


def run_rccl_selftest():
    """BASELINE configs[4]'s RCCL leg on ONE GPU: bench.py with OPV_BENCH_FORCE_DIST=1 takes its N > 1 path
    (init_process_group("nccl", device_id=...), sharding.gather_frames on the library's zero-copy device views,
    all_reduce MAX of the step time) with a world of one rank. Run as a fresh child process; returns what it said."""
    import os
    import socket
    import subprocess
    import time
    root = Path(__file__).resolve().parent.parent
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env.update(OPV_BENCH_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), NCCL_DEBUG="INFO",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    cmd = [sys.executable, str(root / "bench.py"), "--gpus", "1", "--streams", "8", "--frames", "12", "--steps", "1",
           "--warmup", "0", "--full", "--no-extras"]
    t0 = time.time()
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)     # (a hung rendezvous must not eat the suite's time)
    return {"cmd": "OPV_BENCH_FORCE_DIST=1 NCCL_DEBUG=INFO " + " ".join(cmd[1:]), "rc": p.returncode, "stdout": p.stdout,
            "stderr": p.stderr, "seconds": time.time() - t0}


def pytest_sessionstart(session):
    """On a GPU box, under -m gpu: the RCCL self-test child runs FIRST, before this process has touched the GPU
    (tests/test_gpu_multirank.py::test_bench_rccl_leg_executes_at_world_1 reads the result)."""
    import os
    _start_clock()
    expr = session.config.getoption("markexpr", "") or ""
    if "gpu" not in expr or "not gpu" in expr or os.environ.get("OPV_SKIP_RCCL_SELFTEST"):
        return
    try:
        import torch
        if torch.cuda.device_count() < 1:       # (counting devices does not initialise the GPU)
            return
        session.config._opv_rccl_selftest = run_rccl_selftest()
    except Exception as e:                       # reported by the test, not here
        session.config._opv_rccl_selftest = {"cmd": "", "rc": -1, "stdout": "", "stderr": repr(e), "seconds": 0.0}


@pytest.fixture(scope="session")
def golden():
    import json

    import numpy as np

    g = Path(__file__).resolve().parent / "golden"
    arrays = np.load(g / "golden.npz")
    meta = json.loads((g / "golden.json").read_text())
    return arrays, meta


@pytest.fixture(scope="session")
def oracle():
    from oracle_lib import Oracle

    return Oracle()


@pytest.fixture(scope="session")
def iq10(oracle):
    return oracle.modulate(oracle.bert_frames(10))


@pytest.fixture(scope="session")
def iq100(oracle):
    return oracle.modulate(oracle.bert_frames(100))
