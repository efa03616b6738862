"""GN_MLSL with its default local optimiser (LN_COBYLA) on a USER-SUPPLIED device objective (tests/userobj/zoo_extra.hip `myrastrigin`,
bound WITHOUT a host twin): the searches batched on the device as coroutines (hip/cobyla_ext.hip) against the same run with
"amd_cobyla_host" = 1 (every sample and every COBYLA evaluation a single-point launch of the user's kernel) — same process, same seed,
results asserted identical, wall time of each.  -> profiles/r08_cobyla_ext.txt
usage: python tools/cobyla_ext_bench.py [out-file]            the table
       python tools/cobyla_ext_bench.py steps N POP MAXEVAL   one device-path run (for a kernel trace: the launches of
                                                              cobyla_batch_ext_kernel are the run's coroutine steps)
NLOPT_AMD_LIB=<another build's libnlopt_amd.so> runs the same table on that build (the parent commit: both columns the host path)."""
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nlopt_amd          # noqa: E402

SRC = os.path.join(ROOT, "tests", "userobj", "zoo_extra.hip")
CO = os.path.join(ROOT, "tests", "userobj", "zoo_extra.hsaco")


def code_object():
    if not os.path.exists(CO) or os.path.getmtime(CO) < os.path.getmtime(SRC):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"), SRC, "-o", CO], check=True)
    return CO


def run(n, pop, maxeval, host, seed=5, xtol=1e-4):
    o = nlopt_amd.Opt(nlopt_amd.GN_MLSL, n)
    o.set_lower_bounds(-5.12); o.set_upper_bounds(5.12)
    assert o.set_min_device_objective(code_object(), "myrastrigin", None) > 0, o.get_errmsg()
    o.set_xtol_rel(xtol); o.set_population(pop); o.set_maxeval(maxeval)
    if host:
        o.set_param("amd_cobyla_host", 1)
    nlopt_amd.srand(seed)
    x0 = -5.12 + 10.24 * np.modf(np.arange(1, n + 1) * 0.6180339887498949)[0]
    t0 = time.perf_counter()
    x, minf, ret = o.optimize_raw(x0)
    dt = time.perf_counter() - t0
    st = o.stats()
    return dict(x=x, minf=minf, ret=ret, nev=o.get_numevals(), s=dt, launches=st["lbfgs_launches"], searches=st["accepted"], t_local_ms=st["t_lbfgs_ms"],
                iters=st["generations"])


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "steps":
        n, pop, maxeval = (int(v) for v in sys.argv[2:5])
        run(n, pop, min(maxeval, 2000), False)                 # (module load, first launches)
        d = run(n, pop, maxeval, False)
        print("steps-run n=%d pop=%d maxeval=%d: %.3f s, %d launches of the batch (nla_local_ctx_run), %d searches committed, %.1f ms inside them"
              % (n, pop, maxeval, d["s"], d["launches"], d["searches"], d["t_local_ms"]))
        return 0
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r08_cobyla_ext.txt")
    lines = ["# python tools/cobyla_ext_bench.py   (library: %s)" % os.path.relpath(nlopt_amd.LIB_PATH, ROOT),
             "# GN_MLSL, myrastrigin as a user kernel without a host twin, xtol_rel 1e-4, seed 5; device = batched coroutine searches,",
             "# host = amd_cobyla_host 1; wall seconds of nlopt_optimize, one run each behind a warm-up; results asserted bit-identical",
             "# n pop maxeval | device_s host_s host/device | batch launches, searches committed, committed per launch, ms inside the launches | evals ret"]
    run(8, 16, 1500, False); run(8, 16, 1500, True)           # warm-up: module load, first launches
    #          n   pop  maxeval: pop ~ 220 / 1070 -> up to ceil(0.3 (pop + 1)) = 67 / 322 candidates per local phase; pop 1: one search at a time.
    # (The budgets at n = 64 are small: a batch lasts as many steps as its longest search has evaluations, ~2 ms each there.)
    for n, pop, maxeval in ((8, 220, 40000), (8, 1070, 120000), (64, 220, 6000), (64, 1070, 8000), (8, 1, 6000), (64, 1, 3000)):
        d = run(n, pop, maxeval, False)
        h = run(n, pop, maxeval, True)
        same = (d["ret"], d["nev"], d["minf"]) == (h["ret"], h["nev"], h["minf"]) and np.array_equal(d["x"], h["x"])
        assert same, (n, pop, d, h)
        lines.append("%3d %5d %7d | %8.3f %8.3f %6.2f | %5d %6d %7.1f %9.1f | %d %d"
                     % (n, pop, maxeval, d["s"], h["s"], h["s"] / d["s"], d["launches"], d["searches"], d["searches"] / max(d["launches"], 1), d["t_local_ms"], d["nev"], d["ret"]))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
