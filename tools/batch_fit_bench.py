"""Many small fits in one call: nlopt_amd_optimize_batch with a row-data objective (tests/batch/fit_rows.hip: expfit_rows, one decay
curve of m = 64 points per search, LD_LBFGS) against the only path the library had before it — a loop of lone nlopt_optimize calls with
expfit2 and nlopt_amd_set_device_objective_data per curve — and, per batch size, the waiting list of a coroutine step built on the device
(nla_k_local_waiting_list) against the host loop ("amd_batch_host_list" = 1), the two alternating.

Wall time around the call (time.perf_counter), warm (one untimed call of each kind first), `--repeats` timed calls per setting; reported
slowest .. fastest.  Steps per call = the longest search's evaluations (one coroutine step per evaluation of the slowest search).
usage: python tools/batch_fit_bench.py [--counts 1,64,4096,65536] [--repeats 5] [--sample 256] [--out profiles/r11_batch_fit.txt]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nlopt_amd  # noqa: E402

SRC = os.path.join(ROOT, "tests", "batch", "fit_rows.hip")
CO = os.path.join(ROOT, "tests", "batch", "fit_rows.hsaco")
M = 64
T = np.linspace(0.0, 4.0, M)
LB, UB = np.array([0.1, 0.1, -1.0]), np.array([5.0, 5.0, 2.0])


def curves(count, seed=1):
    rng = np.random.default_rng(seed)
    a, b, c = rng.uniform(1.5, 3.5, count), rng.uniform(0.6, 2.0, count), rng.uniform(0.0, 1.0, count)
    Y = a[:, None] * np.exp(-b[:, None] * T[None, :]) + c[:, None] + 0.01 * rng.standard_normal((count, M))
    X0 = np.stack([rng.uniform(0.8, 1.6, count), rng.uniform(0.8, 1.4, count), rng.uniform(-0.2, 0.4, count)], axis=1)
    return Y, X0


def make(name, mf):
    o = nlopt_amd.Opt(nlopt_amd.LD_LBFGS, 3)
    o.set_lower_bounds(LB)
    o.set_upper_bounds(UB)
    assert o.set_min_device_objective(CO, name) > 0, o.get_errmsg()
    o.set_ftol_rel(1e-10)
    o.set_maxeval(200)
    o._L.nlopt_set_vector_storage(o._h, mf)
    return o


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,64,4096,65536")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--mf", type=int, default=10, help="L-BFGS history pairs (vector_storage), the same on both sides")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(CO) or os.path.getmtime(CO) < os.path.getmtime(SRC):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"),
                        SRC, "-o", CO], check=True)
    lines = ["LD_LBFGS, expfit_rows (tests/batch/fit_rows.hip: y = a exp(-b t) + c, n = 3, m = %d points per curve), ftol_rel 1e-10, vector_storage %d;"
             % (M, a.mf),
             "batch: nlopt_amd_optimize_batch, %d timed calls per setting after one warm call, device list (D) and host loop (H) alternating;" % a.repeats,
             "baseline: lone nlopt_optimize calls with expfit2 + set_device_objective_data over a sample of <= %d of the same curves, per fit" % a.sample,
             "   count   batch fits/s D (slowest .. fastest)        baseline fits/s   ratio   steps  ms/step D   ms/step H   H/D time  searches without a positive result"]
    for count in [int(c) for c in a.counts.split(",")]:
        Y, X0 = curves(count)
        rows = np.concatenate([np.tile(T, (count, 1)), Y], axis=1)
        o = make("expfit_rows", a.mf)
        assert o.set_device_objective_row_data(rows) > 0, o.get_errmsg()
        times = {0: [], 1: []}
        steps = 0
        for rep in range(a.repeats + 1):
            for host in (0, 1):
                o.set_param("amd_batch_host_list", host)
                t0 = time.perf_counter()
                X, minf, res, nev = o.optimize_batch(X0)
                dt = time.perf_counter() - t0
                failed = int(np.sum(res <= 0))           # (a search the algorithm itself gives up on, alone or batched alike)
                if rep:
                    times[host].append(dt)
                steps = int(nev.max())
        # the baseline: the same curves one by one
        k = min(count, a.sample)
        b = make("expfit2", a.mf)
        base = []
        for rep in range(2):
            t0 = time.perf_counter()
            for i in range(k):
                b.set_device_objective_data(np.concatenate([T, Y[i]]))
                x, f, r = b.optimize_raw(X0[i])
                assert r == res[i] and np.array_equal(x, X[i]) and f == minf[i], (i, r)   # the same fits, bit for bit
            base.append((time.perf_counter() - t0) / k)
        per_fit = min(base)
        d, h = np.array(times[0]), np.array(times[1])
        lines.append("%8d   %10.4g (%10.4g .. %10.4g)        %10.4g   %7.2fx  %5d  %9.4f   %9.4f   %6.3f   %d"
                     % (count, count / np.median(d), count / d.max(), count / d.min(), 1.0 / per_fit, (count / np.median(d)) * per_fit,
                        steps, 1e3 * np.median(d) / steps, 1e3 * np.median(h) / steps, np.median(h) / np.median(d), failed))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
