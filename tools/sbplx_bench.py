"""What a batch of Subplex searches costs (one MI355X), NLOPT_LN_SBPLX, xtol_rel 1e-8, maxeval 400, COUNT searches:
  compiled-in   the n = 8 Rosenbrock objective of the library: every search is a wavefront of hip/sbplx_kernels.hip, one launch from start to end;
  user kernel   the exponential decay of tests/batch/fit_rows.hip (y = a exp(-b t) + c: n = 3, m = 64 points per curve; tools/nldrmd_bench.py's
                fit), one curve per search as an ABI-3 data row: the coroutine, one step per evaluation of the slowest search.
Each against
  lone loop     the same searches one by one through nlopt_optimize on the same library (asserted bit-identical to the batch; timed over
                --sample of them and scaled — the loop is linear in the count);
  reference     the REAL reference's nlopt_optimize(NLOPT_LN_SBPLX) in a loop on one CPU thread over the same sample, scaled: the oracle's C
                twin of the Rosenbrock objective / tools/userdata_fit_twin.c (sequential sums: compared by value only).
Wall time around the calls (time.perf_counter), one untimed warm call of each batch first, then --repeats timed ones: the median, the
least and the greatest.
usage: python tools/sbplx_bench.py [--count 4096] [--repeats 3] [--sample 256] [--out FILE] [--json FILE]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import nlopt_amd                                  # noqa: E402
import nldrmd_bench as NB                         # noqa: E402
from batch_fit_bench import CO, LB, SRC, T, UB, curves      # noqa: E402

LN_SBPLX = 29


def timed(fn, repeats):
    """one warm call, then `repeats` timed ones: (median, least, greatest) seconds and the last result"""
    times, out = [], None
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        out = fn()
        if rep:
            times.append(time.perf_counter() - t0)
    return (float(np.median(times)), float(min(times)), float(max(times))), out


def rosen_opt():
    o = nlopt_amd.Opt(LN_SBPLX, 8)
    o.set_lower_bounds(-2.0)
    o.set_upper_bounds(2.0)
    o.set_min_objective(nlopt_amd.objective("rosenbrock"))
    o.set_xtol_rel(1e-8)
    o.set_maxeval(400)
    return o


def rosen_reference(X0):
    """seconds per search of the real reference on the oracle's C twin, its minima and evaluations"""
    import _oracle as O
    import nldrmd_emu_check as E
    R, L = E.ref_bind(O.ref()), O.port()
    f = L.orc_objective(O.OBJ["rosenbrock"])
    lb, ub = np.full(8, -2.0), np.full(8, 2.0)
    best, fs, evals = None, np.zeros(len(X0)), 0
    for rep in range(2):
        total = 0.0
        for i, s in enumerate(X0):
            opt = R.nlopt_create(LN_SBPLX, 8)
            R.nlopt_set_lower_bounds(opt, O.dptr(lb)); R.nlopt_set_upper_bounds(opt, O.dptr(ub))
            R.nlopt_set_min_objective(opt, f, None)
            R.nlopt_set_xtol_rel(opt, 1e-8); R.nlopt_set_maxeval(opt, 400)
            x, minf = np.array(s), C.c_double(0)
            t0 = time.perf_counter()
            R.nlopt_optimize(opt, O.dptr(x), C.byref(minf))
            total += time.perf_counter() - t0
            fs[i] = minf.value
            evals += R.nlopt_get_numevals(opt) if rep == 0 else 0
            R.nlopt_destroy(opt)
        best = total / len(X0) if best is None else min(best, total / len(X0))
    return best, fs, evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--out", default=None)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not os.path.exists(CO) or os.path.getmtime(CO) < os.path.getmtime(SRC):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"),
                        SRC, "-o", CO], check=True)
    count, k = a.count, min(a.count, a.sample)
    have_ref = os.path.exists(NB.REF)
    lines = ["# python tools/sbplx_bench.py --count %d --repeats %d --sample %d   (library: %s, %s)"
             % (count, a.repeats, a.sample, os.path.relpath(nlopt_amd.LIB_PATH, ROOT), time.strftime("%Y-%m-%d")),
             "# NLOPT_LN_SBPLX, xtol_rel 1e-8, maxeval 400, %d searches; loops timed over %d searches and scaled; time: median (least .. greatest) of %d"
             % (count, k, a.repeats),
             "%-44s %30s %12s %12s %14s" % ("", "time [ms]", "searches/s", "evaluations", "steps (max ev)")]
    rec = []

    def row(what, t, evals, steps):
        med, lo, hi = t
        lines.append("%-44s %10.2f (%8.2f .. %8.2f) %12.4g %12d %14s" % (what, 1e3 * med, 1e3 * lo, 1e3 * hi, count / med, evals, steps))
        rec.append(dict(what=what, count=count, ms_median=1e3 * med, ms_min=1e3 * lo, ms_max=1e3 * hi, evaluations=int(evals), steps=str(steps)))
        print(lines[-1], flush=True)

    def scaled(ts):
        return tuple(t * count / k for t in ts)

    # ---- the compiled-in objective ----
    r = rosen_opt()
    XR = np.random.default_rng(3).uniform(-1.8, 1.8, (count, 8))
    tr, (X, minf, res, nev) = timed(lambda: r.optimize_batch(XR), a.repeats)
    row("Rosenbrock n = 8 compiled in, one batch", tr, int(nev.sum()), "1 launch")

    def lone_rosen():
        for i in range(k):
            x, f, rr = r.optimize_raw(XR[i])
            assert rr == res[i] and np.array_equal(x, X[i]) and f == minf[i] and r.get_numevals() == nev[i], (i, rr)
    tl, _ = timed(lone_rosen, a.repeats)
    row("  loop of lone calls", scaled(tl), int(nev[:k].sum() * count / k), "")
    if have_ref:
        per, fs, evals = rosen_reference(XR[:k])
        row("  reference, 1 CPU thread, C twin", (per * count,) * 3, int(evals * count / k), "")
        lines.append("#   (median |minf - reference's| over the sample: %.3g; the device sums the objective as a tree)" % float(np.median(np.abs(fs - minf[:k]))))
    lines.append("#   searches without a positive result: %d" % int(np.sum(res <= 0)))

    # ---- the user's device objective on per-search data rows ----
    Y, X0 = curves(count)
    rows = np.concatenate([np.tile(T, (count, 1)), Y], axis=1)
    o = NB.make(LN_SBPLX, "expfit_rows")
    assert o.set_device_objective_row_data(rows) > 0, o.get_errmsg()
    tb, (X, minf, res, nev) = timed(lambda: o.optimize_batch(X0), a.repeats)
    row("exponential fit n = 3 user kernel, one batch", tb, int(nev.sum()), int(nev.max()))
    o.set_param("amd_batch_host_list", 0)                 # the waiting list of every step built on the device instead of by the host loop
    td, (Xd, minfd, _, nevd) = timed(lambda: o.optimize_batch(X0), a.repeats)
    assert np.array_equal(Xd, X) and np.array_equal(minfd, minf) and np.array_equal(nevd, nev)
    row("  ... with the device-built list", td, int(nevd.sum()), int(nevd.max()))
    b = NB.make(LN_SBPLX, "expfit2")

    def lone_fit():
        for i in range(k):
            b.set_device_objective_data(np.concatenate([T, Y[i]]))
            x, f, rr = b.optimize_raw(X0[i])
            assert rr == res[i] and np.array_equal(x, X[i]) and f == minf[i] and b.get_numevals() == nev[i], (i, rr)
    tl, _ = timed(lone_fit, a.repeats)
    row("  loop of lone calls", scaled(tl), int(nev[:k].sum() * count / k), "")
    if have_ref:
        with tempfile.TemporaryDirectory() as tmp:
            per, fs, evals = NB.reference_loop(Y, X0, k, tmp, alg=LN_SBPLX)
        row("  reference, 1 CPU thread, C twin", (per * count,) * 3, int(evals * count / k), "")
        lines.append("#   (median |minf - reference's| over the sample: %.3g; the twin sums in another order)" % float(np.median(np.abs(fs - minf[:k]))))
    lines.append("#   searches without a positive result: %d" % int(np.sum(res <= 0)))
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(dict(tool="tools/sbplx_bench.py", count=count, repeats=a.repeats, sample=k, rows=rec), fh, indent=1)


if __name__ == "__main__":
    main()
