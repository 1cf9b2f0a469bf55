"""CPU-only: the shape of bench.py's ONE JSON line (the driver's contract), checked on the line recorded on MI355X by
profiles/collect.sh (the newest profiles/rNN_bench.json; made with an extras budget that holds every extra): metric / config as
BASELINE.json names them, whole-job value, the roofline and cpu_baseline objects with every field the contract lists,
internally consistent numbers."""
import json
import re
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_recorded_bench_line_has_the_contract_shape():
    line = json.loads(sorted((ROOT / "profiles").glob("r[0-9][0-9]_bench.json"))[-1].read_text())
    base = json.loads((ROOT / "BASELINE.json").read_text())
    assert line["metric"] == base["metric"] and line["unit"] == "Msamples/s"
    for k in ("value", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in line, k
    assert line["higher_is_better"] is True and line["scaling"] == "weak" and line["vs_baseline"] is None and line["dtype"] == "f64"
    assert line["data"] == "synthetic" and "workload" in line["config"] and "model" not in line["config"]
    assert line["config"]["workload"].startswith("configs[3]: 64 concurrent IQ streams")
    assert "f0 -2000..+2000 Hz" in line["config"]["workload"]            # SURVEY.md 8(d) C4 as written: the edge streams on the AFC clamp
    # the contract's figures are total-time ones; the median of the (>= 5) timed steps stands next to them
    m = line["median"]
    assert line["steps"] >= 5 and len(m["step_ms"]) == line["steps"]
    assert abs(m["ms_per_step"] - sorted(m["step_ms"])[len(m["step_ms"]) // 2]) < 1e-6
    assert abs(m["value"] - line["value"]) < 0.02 * line["value"]
    # value = samples of all streams x steps / time
    n = line["config"]["samples_per_stream"] * line["config"]["streams_per_gpu"] * line["n_gpus"]
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3) / 1e6) < 0.01 * line["value"]
    r = line["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["kernel"].startswith("k_msk_frontend")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-6
    algo = n / line["n_gpus"] * (4.0 + 134.0 / 86720)                   # 4 B in + 134 B per frame out
    assert abs(r["achieved"] - algo / (r["kernel_ms"] * 1e-3) / 1e9) < 0.01 * r["achieved"]
    assert r["traffic"] is None or r["traffic"] >= 0.99 * r["achieved"]    # measured HBM bytes are never below the algorithmic ones
    assert r["issue"]["wave_cycles_per_symbol"] > 600 and 2.0 < r["issue"]["clock_GHz"] < 2.5
    # the bound that BINDS is named in the object (64 waves on 1024 SIMDs: a lone wave's issue port), HBM stays the contract's figure
    b = r["binding"]
    assert b["bound"] == "wave-issue" and b["waves"] == 64 and b["simds"] == 1024
    assert 0.5 < b["frac"] <= 1.0 and abs(b["frac"] - b["achieved"] / b["peak"]) < 2e-3 and b["frac"] == r["issue"]["wave_issue_frac"]
    assert b["frac"] > 100 * r["frac"]                                   # (what the HBM fraction alone would hide)
    # ... and it is the FIRST thing the note says: a record that keeps the note's first hundred characters keeps the binding bound
    m_ = re.match(r"binding=wave-issue (0\.\d{3}) \((\d+) instr x 4 / ([\d.]+) cyc\); ", r["note"])
    assert m_, r["note"][:120]
    assert float(m_.group(1)) == round(b["frac"], 3) and abs(float(m_.group(3)) - b["peak"]) < 0.05 and abs(4 * int(m_.group(2)) - b["achieved"]) <= 2.0
    assert r["fp64_valu"]["peak"] == 78.6 and r["fp64_valu"]["unit"] == "TFLOP/s"
    c = line["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] == 1 and 1.0 < c["value"] < 200.0
    assert line["check"]["edge_ties"] == 0 and line["check"]["frames_exact"] >= 0.99 * line["check"]["frames_total"]
    ac = line["extras"]["all_clean_variant"]                              # C4's "all-clean variant": every frame exact and perfect
    assert ac["frames_exact"] == ac["frames_total"] == ac["frames_perfect"] == 64000 and ac["steps"] >= 5
    # the extras share one wall-clock budget; the recorded line was made with one that holds them all
    assert line["extras"]["skipped_for_budget"] == [] and line["extras"]["budget"]["spent_total_s"] <= line["extras"]["budget"]["seconds"]
    lc = line["extras"]["live_capacity"]
    assert lc["streams"] >= 4096 and lc["round_ms_p99"] < 40.0 and all(p.get("frames_wrong", 0) == 0 for p in lc["probes"])
    assert lc["pipelined"]["streams"] >= lc["streams"] and lc["cut_short"] is None
    # the boundary's host-buffer entry points: the batched asynchronous push releases what the attached run releases, faster than one copy per stream
    pi = line["extras"]["pcie_inclusive"]
    assert pi["host_pushed_batched"]["frames_released"] == pi["host_pushed"]["frames_released"] == pi["hbm_attached"]["frames_released"]
    assert pi["host_pushed_batched"]["ms"] < 1.1 * pi["host_pushed"]["ms"]      # (both sit on the PCIe link's rate: 2.2 GB in ~75 ms beside the kernels)
    # the regimes beside the contract configuration, as recorded: a host-side step that grows with the stream count shows here first
    # (round 5: deciding EVERY guarded offset search on the host took the 32 768-stream figure from 412 to 264 GS/s)
    ex = line["extras"]
    assert ex["many_streams_unique_captures"]["Msamples/s"] > 350000.0 and ex["many_streams_unique_captures"]["frontend_kernel"] == "k_msk_frontend_x16_wg8"
    assert ex["stream_sweep"]["16384x3"]["16_per_wave"]["Msamples/s"] > 240000.0
    assert ex["configs4_workload_on_one_gpu"]["Msamples/s"] > 55000.0 and ex["stream_sweep"]["1024x60"]["1_per_wave"]["Msamples/s"] > 100000.0


# ----------------------------------------------------------------------------------------------------------------------
# bench.py's world > 1 branch, EXECUTED (on the one GPU of the test box): two ranks share cuda:0
# (OPV_BENCH_SHARE_DEVICE=1) and rendezvous / gather over gloo (OPV_BENCH_BACKEND=gloo; RCCL refuses two ranks on one
# device). Rank spawning, the per-rank shard, the cross-rank expectation, the MAX of the step time and the N > 1
# cpu_baseline leg are the lines an 8-GPU node runs; only the transport differs (RCCL's leg: test_gpu_multirank.py).
import os
import subprocess
import sys
import time

import pytest

WORLD2_ARGS = ["--gpus", "2", "--streams", "8", "--frames", "12", "--steps", "2", "--warmup", "1", "--full"]     # (--full: the checks below)


def _world2_env():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE",
                                                            "MASTER_ADDR", "MASTER_PORT", "OPV_BENCH_FORCE_DIST")}
    env.update(OPV_BENCH_BACKEND="gloo", OPV_BENCH_SHARE_DEVICE="1",
               HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return env


def _check_world2_line(p, how, world=2, backend="gloo"):
    out = ROOT / "gpurun_out"
    out.mkdir(exist_ok=True)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
    with open(out / "bench_world2.txt", "a") as f:
        f.write(("$ OPV_BENCH_BACKEND=gloo OPV_BENCH_SHARE_DEVICE=1 " if backend == "gloo" else "$ ") + f"{how}\nexit {p.returncode}\n" + "\n".join(lines) + "\n"
                + ("--- stderr tail\n" + p.stderr[-3000:] + "\n" if p.returncode else "") + "\n")
    assert p.returncode == 0, p.stderr[-3000:]
    assert len(lines) == 1, p.stdout[-2000:]          # ONE line, from rank 0 only
    line = json.loads(lines[0])
    S, F = 8, 12
    W = world
    assert line["n_gpus"] == W and line["steps"] == 2 and line["warmup"] == 1 and line["scaling"] == "weak"
    c = line["collective"]
    assert c["backend"] == backend and c["world"] == W
    assert c["gathered_shape"][0] == W and c["gathered_shape"][1] == S and c["gathered_shape"][3] == 134
    # rank r owns the global streams 8 r .. 8 r + 7 - not a second copy of 0..7: said by the ranks, and read back from the bytes
    assert c["rank_shards"] == [[r * S, (r + 1) * S] for r in range(W)]
    assert c["gathered_callsigns"] == [f"S{g}" for g in range(W * S)]
    assert c["rank_frames_released"] == [S * F] * W
    chk = line["check"]
    assert chk["gathered_frames_total"] == W * S * F
    assert chk["gathered_frames_exact"] >= W * S * F - W          # 16 dB: at most a stray channel error per rank
    assert chk["gathered_equals_local_view"] is True and chk["edge_ties"] == 0
    # whole-job value: the samples of ALL ranks over the max-over-ranks time
    n = line["config"]["samples_per_stream"] * S * W
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3) / 1e6) < 0.01 * line["value"]
    r = line["roofline"]
    assert r["bound"] == "hbm" and r["kernel"].startswith("k_msk_frontend") and r["achieved"] > 0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-6
    cb = line["cpu_baseline"]
    assert cb["kind"] in ("reference", "port") and cb["cores"] == 1 and cb["value"] > 0.5
    return line


@pytest.mark.gpu
def test_bench_world2_started_from_a_bare_shell():
    """`python bench.py --gpus 2`: spawn_ranks starts both ranks itself and relays rank 0's line"""
    cmd = [sys.executable, str(ROOT / "bench.py")] + WORLD2_ARGS
    p = subprocess.run(cmd, env=_world2_env(), capture_output=True, text=True, timeout=420)
    _check_world2_line(p, "python bench.py " + " ".join(WORLD2_ARGS))


@pytest.mark.gpu
@pytest.mark.parametrize("world", [2, 4])
def test_bench_world2_under_the_drivers_launcher(world):
    """the driver's own command for N > 1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N
    (RANK / LOCAL_RANK / WORLD_SIZE / MASTER_* come from the launcher), with two and with four ranks on the one GPU"""
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    args = ["--gpus", str(world)] + WORLD2_ARGS[2:]
    launch = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
              "--master-port", str(port), str(ROOT / "bench.py")] + args
    p = subprocess.run([sys.executable] + launch, env=_world2_env(), capture_output=True, text=True, timeout=420)
    _check_world2_line(p, "python " + " ".join(launch[:-len(args) - 1]) + " bench.py " + " ".join(args), world=world)


def _n_gpus():
    try:
        import torch
        return torch.cuda.device_count()           # (does not initialise a GPU on this image)
    except Exception:
        return 0


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 4])
def test_bench_worldN_over_rccl_under_the_drivers_launcher(world):
    """ARMED FOR AN N-GPU BOX (worlds 2 and 4 are skipped on the 1-GPU pool; world 1 runs there, so that only the other ranks
    are new on a bigger box): the driver's own launcher command with NO rehearsal switch - rank r on cuda:r,
    init_process_group("nccl") = RCCL over xGMI, the frame gather and the MAX of the step time on device tensors. Same checks as
    the gloo rehearsal: rank shards, callsigns read back from the gathered bytes, whole-job value."""
    import socket
    if _n_gpus() < world:
        pytest.skip(f"needs >= {world} GPUs, {_n_gpus()} visible: RCCL refuses two ranks on one device (armed for an N-GPU box)")
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        port = sk.getsockname()[1]
    env = {k: v for k, v in _world2_env().items() if k not in ("OPV_BENCH_BACKEND", "OPV_BENCH_SHARE_DEVICE")}
    args = ["--gpus", str(world)] + WORLD2_ARGS[2:]
    if world == 1:
        env["OPV_BENCH_FORCE_DIST"] = "1"                  # (one rank takes bench.py's N > 1 path only when told to)
        args.append("--no-big")                            # (and a one-rank line carries extras: not the minutes-long ones)
    launch = ["-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(world), "--master-addr", "127.0.0.1",
              "--master-port", str(port), str(ROOT / "bench.py")] + args
    p = subprocess.run([sys.executable] + launch, env=env, capture_output=True, text=True, timeout=420)
    _check_world2_line(p, "python " + " ".join(launch[:-len(args) - 1]) + " bench.py " + " ".join(args), world=world, backend="nccl")


@pytest.mark.gpu
def test_bench_world2_a_dead_rank_takes_the_job_down():
    """rank 1 is killed while the job runs: the parent ends rank 0 too and exits non-zero within seconds (a surviving
    rank would otherwise sit in the gather until the rendezvous timeout, half an hour)"""
    import psutil
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "2", "--streams", "8", "--frames", "100", "--steps", "2000", "--warmup", "1"]
    parent = subprocess.Popen(cmd, env=_world2_env(), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    try:
        victim = None
        t0 = time.time()
        while victim is None and time.time() - t0 < 120:
            for ch in psutil.Process(parent.pid).children():
                try:
                    if ch.environ().get("RANK") == "1":
                        victim = ch
                except psutil.Error:
                    pass
            time.sleep(0.1)
        assert victim is not None, "rank 1 never appeared"
        time.sleep(20.0)                                   # both ranks are up and inside their steps by now
        assert parent.poll() is None, parent.communicate()[1][-2000:]
        victim.kill()
        t1 = time.time()
        out, err = parent.communicate(timeout=60)
        took = time.time() - t1
    finally:
        if parent.poll() is None:
            for ch in psutil.Process(parent.pid).children(recursive=True):
                ch.kill()
            parent.kill()
    assert parent.returncode != 0
    assert took < 15.0, took
    assert not [ln for ln in out.splitlines() if ln.startswith('{"metric"')]     # and no bench line from a broken job
    with open(ROOT / "gpurun_out" / "bench_world2.txt", "a") as f:
        f.write(f"$ bench.py --gpus 2 ... with rank 1 killed (SIGKILL) 20 s in: parent exit {parent.returncode} after {took:.2f} s, no bench line\n\n")


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_what_it_decoded(tmp_path):
    """the plain command (no --full): one line with the headline fields and nothing measured beside them, --steps timed steps;
    --dump-outputs writes what the last timed step decoded - every stream's frames equal what it was sent (16 dB: at most a
    stray channel error), counts and Viterbi metrics beside them - and two runs with the same arguments write the same arrays"""
    import numpy as np
    from __graft_entry__ import load_opv_amd, load_pkg_module
    amd, workload = load_opv_amd(), load_pkg_module("workload")
    S, F, K = 8, 12, 3
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "LOCAL_WORLD_SIZE", "OPV_BENCH_FORCE_DIST")}
    dumps = []
    for run in range(2):
        d = tmp_path / f"run{run}"
        cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--streams", str(S), "--frames", str(F), "--steps", str(K),
               "--warmup", "1", "--dump-outputs", str(d)]
        p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr[-3000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{"metric"')]
        assert len(lines) == 1, p.stdout[-2000:]
        line = json.loads(lines[0])
        assert line["steps"] == K and len(line["median"]["step_ms"]) == K and line["warmup"] == 1
        assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
        n = line["config"]["samples_per_stream"] * S
        assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3) / 1e6) < 0.01 * line["value"]
        for k in ("roofline", "kernel_ms", "check", "cpu_baseline", "extras"):
            assert k not in line, k                                  # (what --full adds)
        dumps.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    a, b = dumps
    assert sorted(a) == ["counts", "frames", "viterbi_metric"] and sorted(b) == sorted(a)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and np.array_equal(a[k], b[k]), k
    assert a["frames"].shape == (S, F, 134) and a["viterbi_metric"].shape == (S, F) and np.array_equal(a["counts"], np.full(S, F))
    sent = np.stack([workload.tx_frames(amd, g, F) for g in range(S)])
    assert int((a["frames"] == sent).all(axis=2).sum()) >= S * F - 1
    m = a["viterbi_metric"]
    assert np.array_equal(m, np.round(m)) and m.min() >= -1                # int32 metrics (-1: a frame the decoder dropped)
