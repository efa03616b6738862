"""What a constrained COBYLA batch costs (one MI355X): nlopt_amd_optimize_batch with NLOPT_LN_COBYLA, a user device objective and a
user's device constraint blocks (tests/batchcon/con_models.hip: n = 5, inequality blocks of 3 and 1 values, an equality block of 2)
against the only way to do this without it — a loop of lone nlopt_optimize calls on the same optimiser (the host algorithm, every
evaluation a handful of single-point launches).  Results asserted identical where both ran.
usage: python tools/batch_con_bench.py [out-file]        the table for count = 1, 64, 4096 (the loop is timed over at most 256 searches
                                                         and scaled: it is linear in the count)
       python tools/batch_con_bench.py steps COUNT       one batch of COUNT searches and nothing else — for a kernel trace
                                                         (rocprofv3 --kernel-trace --stats -- python tools/batch_con_bench.py steps 4096):
                                                         the share of the <block>_coneval kernels in the batch's device time"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import nlopt_amd          # noqa: E402

CO = os.path.join(ROOT, "tests", "batchcon", "con_models.hsaco")
C5, W5 = np.array([1.0, -0.5, 0.75, 1.5, -1.0]), np.array([1.0, 2.0, 0.5, 1.5, 1.0])
LOOP_MAX = 256


def optimiser():
    o = nlopt_amd.Opt(nlopt_amd.LN_COBYLA, 5)
    o.set_lower_bounds(-2.0)
    o.set_upper_bounds(2.0)
    assert o.set_min_device_objective(CO, "wsq2") > 0, o.get_errmsg()
    assert o.set_device_objective_data(np.concatenate([C5, W5])) > 0
    assert o.add_inequality_device_constraints(CO, "prod3", 3, tol=1e-8) > 0, o.get_errmsg()
    assert o.add_inequality_device_constraints(CO, "ball", 1, tol=1e-8, data=np.array([4.0])) > 0
    assert o.add_equality_device_constraints(CO, "heq2", 2, tol=1e-8) > 0
    o.set_xtol_rel(1e-6)
    o.set_maxeval(400)
    return o


def starts(count):
    return np.random.default_rng(2025).uniform(-1.9, 1.9, (count, 5))


def main():
    if not os.path.exists(CO):
        raise SystemExit("build tests/batchcon/con_models.hsaco first (__graft_entry__.build() does)")
    if len(sys.argv) > 2 and sys.argv[1] == "steps":
        o = optimiser()
        X, minf, res, nev = o.optimize_batch(starts(int(sys.argv[2])))
        print("batch of %s: %d evaluations, %d constraint launches" % (sys.argv[2], o.get_numevals(), o.batch_constraint_launches()))
        return
    o = optimiser()
    o.optimize_batch(starts(2))                                       # (first launches: code objects loaded, kernels resolved)
    lines = ["# python tools/batch_con_bench.py   (library: %s, %s)" % (os.path.relpath(nlopt_amd.LIB_PATH, ROOT), time.strftime("%Y-%m-%d")),
             "# n = 5, mi = 4, me = 2 (mc = 8 user rows + 10 bound rows), xtol_rel 1e-6, maxeval 400",
             "%6s %12s %12s %14s %14s %10s %12s" % ("count", "evaluations", "steps", "batch [ms]", "loop [ms]", "loop/batch", "con launches")]
    for count in (1, 64, 4096):
        X0 = starts(count)
        t0 = time.perf_counter()
        X, minf, res, nev = o.optimize_batch(X0)
        tb = time.perf_counter() - t0
        launches, evals = o.batch_constraint_launches(), int(nev.sum())
        k = min(count, LOOP_MAX)
        t0 = time.perf_counter()
        ones = [o.optimize_raw(x) for x in X0[:k]]
        tl = (time.perf_counter() - t0) * count / k
        for i, (x, f, r) in enumerate(ones):
            assert r == res[i] and np.array_equal(x, X[i]) and f == minf[i], (count, i)
        lines.append("%6d %12d %12d %14.2f %14.2f %10.1f %12d%s" % (count, evals, launches // 3, tb * 1e3, tl * 1e3, tl / tb, launches,
                                                                "   (loop: %d searches timed, scaled)" % k if k < count else ""))
        print(lines[-1], flush=True)
    out = sys.argv[1] if len(sys.argv) > 1 else None
    text = "\n".join(lines) + "\n"
    if out:
        with open(out, "w") as fh:
            fh.write(text)
    print(text)


if __name__ == "__main__":
    main()
