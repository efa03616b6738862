"""What batches of truncated-Newton searches cost (one MI355X): NLOPT_LD_TNEWTON, _RESTART, _PRECOND, _PRECOND_RESTART through
nlopt_amd_optimize_batch on the compiled-in Rosenbrock and Rastrigin objectives — COUNT searches of dimension N from starts drawn in the
objective's golden box, maxeval MAXEVAL, no other tolerance set — in tree-sum mode (the default) and with amd_exact_dot = 1, beside
  LD_LBFGS   batches of the same shape on the same box in the same run, and
  reference  the REAL reference (oracle/_ref/libnlopt_ref.so) on one host core: its nlopt_optimize in a loop over a sample of the starts with
             the oracle's sequential C objective, scaled to COUNT.
Wall time around the call (time.perf_counter): one untimed warm call, then the median (least .. greatest) of --repeats timed ones.
Figures: evaluations/s (all searches' evaluations over the call's time) and ms per search (the call's time over COUNT).
usage: python tools/tnewton_bench.py [--counts 1,64,2048] [--dims 64,1024,4096] [--objs rosenbrock,rastrigin] [--algs 15,16,17,18]
                                     [--maxeval 200] [--repeats 3] [--sample 4] [--out FILE] [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nlopt_amd                                  # noqa: E402
import _oracle as O                               # noqa: E402

NAMES = {11: "LD_LBFGS", 15: "LD_TNEWTON", 16: "LD_TNEWTON_RESTART", 17: "LD_TNEWTON_PRECOND", 18: "LD_TNEWTON_PRECOND_RESTART"}


def make(alg, obj, n, maxeval, exact):
    _, lo, hi = O.golden_x0(obj, n)
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(lo)
    o.set_upper_bounds(hi)
    o.set_min_objective(nlopt_amd.objective(obj))
    o.set_maxeval(maxeval)
    o.set_param("amd_exact_dot", 1 if exact else 0)
    return o


def timed_batches(o, X0, repeats):
    times = []
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        out = o.optimize_batch(X0)
        if rep:
            times.append(time.perf_counter() - t0)
    return times, out


def reference_loop(alg, obj, n, X0, maxeval):
    """seconds and evaluations of the real reference's loop over the rows of X0, one host core, the oracle's C objective"""
    secs, evals = 0.0, 0
    for x0 in X0:
        t0 = time.perf_counter()
        r = O.run_ref(alg, obj, n, 0, 0, maxeval=maxeval, x0=x0, cap=maxeval + 2 * n + 64)
        secs += time.perf_counter() - t0
        evals += r["nevals"]
    return secs, evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,64,2048")
    ap.add_argument("--dims", default="64,1024,4096")
    ap.add_argument("--objs", default="rosenbrock,rastrigin")
    ap.add_argument("--algs", default="15,16,17,18")
    ap.add_argument("--maxeval", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    counts, dims = [int(v) for v in a.counts.split(",")], [int(v) for v in a.dims.split(",")]
    objs, algs = a.objs.split(","), [int(v) for v in a.algs.split(",")]
    lines = ["# python tools/tnewton_bench.py --counts %s --dims %s --objs %s --algs %s --maxeval %d --repeats %d --sample %d   (library: %s, %s)"
             % (a.counts, a.dims, a.objs, a.algs, a.maxeval, a.repeats, a.sample, os.path.relpath(nlopt_amd.LIB_PATH, ROOT), time.strftime("%Y-%m-%d")),
             "# starts drawn in the golden box, maxeval %d per search; time: median (least .. greatest) of %d calls after one warm call" % (a.maxeval, a.repeats),
             "%-11s %5s %6s %-27s %-5s %31s %12s %12s %11s %9s" % ("objective", "n", "count", "algorithm", "sums", "time [ms]", "evals/s", "ms/search", "evaluations", "positive")]
    print("\n".join(lines), flush=True)
    records = []

    def row(obj, n, count, what, sums, times, evals, positive):
        med = float(np.median(times))
        lines.append("%-11s %5d %6d %-27s %-5s %10.2f (%8.2f .. %8.2f) %12.4g %12.4g %11d %9s" %
                     (obj, n, count, what, sums, 1e3 * med, 1e3 * min(times), 1e3 * max(times), evals / med, 1e3 * med / count, evals, positive))
        records.append(dict(objective=obj, n=n, count=count, algorithm=what, sums=sums, seconds=[float(t) for t in times], evaluations=int(evals),
                            positive=positive))
        print(lines[-1], flush=True)
    for obj in objs:
        for n in dims:
            _, lo, hi = O.golden_x0(obj, n)
            for count in counts:
                X0 = np.random.default_rng(7 * n + count).uniform(lo, hi, (count, n))
                for alg in [11] + algs:
                    for exact in (False, True):
                        o = make(alg, obj, n, a.maxeval, exact)
                        times, (_, _, res, nev) = timed_batches(o, X0, a.repeats)
                        row(obj, n, count, NAMES[alg], "exact" if exact else "tree", times, int(nev.sum()), "%d/%d" % (int(np.sum(res > 0)), count))
            if O.have_ref():
                k = min(a.sample, max(counts))
                Xs = np.random.default_rng(7 * n + max(counts)).uniform(lo, hi, (max(counts), n))[:k]
                for alg in [11] + algs:
                    secs, evals = reference_loop(alg, obj, n, Xs, a.maxeval)
                    row(obj, n, k, "reference " + NAMES[alg], "seq", [secs], evals, "")
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(command=lines[0][2:], rows=records), fh, indent=1)


if __name__ == "__main__":
    main()
