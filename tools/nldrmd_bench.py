"""What a batch of small Nelder-Mead fits costs (one MI355X): COUNT fits of the exponential decay of tests/batch/fit_rows.hip (y = a exp(-b t)
+ c: n = 3 parameters, m = 64 points per curve), one curve per search as an ABI-3 data row, NLOPT_LN_NELDERMEAD, xtol_rel 1e-8, maxeval 400:
  batch      nlopt_amd_optimize_batch: every search a wavefront of hip/nldrmd_kernels.hip, one coroutine step per evaluation of the slowest;
  lone loop  the same fits one by one: nlopt_optimize with expfit2 + nlopt_amd_set_device_objective_data per curve (asserted bit-identical
             to the batch; timed over a sample and scaled — the loop is linear in the count);
  reference  the REAL reference's nlopt_optimize(NLOPT_LN_NELDERMEAD) in a loop on one CPU thread, the objective the sequential C twin
             tools/userdata_fit_twin.c (its sums are ordered differently from the device kernel's, so its fits are compared by value only);
  COBYLA     the same batch with NLOPT_LN_COBYLA, for scale.
Wall time around the calls (time.perf_counter), one untimed warm call of each kind first, the median of --repeats timed ones.
usage: python tools/nldrmd_bench.py [--count 4096] [--repeats 3] [--sample 256] [--out FILE]"""
import argparse
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import nlopt_amd                                  # noqa: E402
from batch_fit_bench import CO, LB, M, SRC, T, UB, curves      # noqa: E402

REF = os.path.join(ROOT, "oracle", "_ref", "libnlopt_ref.so")


class FitData(C.Structure):
    """fit_data of tools/userdata_fit_twin.c"""
    _fields_ = [("m", C.c_long), ("t", C.c_void_p), ("y", C.c_void_p)]


def make(alg, name):
    o = nlopt_amd.Opt(alg, 3)
    o.set_lower_bounds(LB)
    o.set_upper_bounds(UB)
    assert o.set_min_device_objective(CO, name) > 0, o.get_errmsg()
    o.set_xtol_rel(1e-8)
    o.set_maxeval(400)
    return o


def timed_batches(o, X0, repeats):
    times = []
    for rep in range(repeats + 1):
        t0 = time.perf_counter()
        out = o.optimize_batch(X0)
        if rep:
            times.append(time.perf_counter() - t0)
    return float(np.median(times)), out


def reference_loop(Y, X0, k, tmp, alg=None):
    """seconds per fit of the real reference on the C twin, its minima and its evaluations over the k fits (alg: the reference's
    algorithm, NLOPT_LN_NELDERMEAD unless given — tools/sbplx_bench.py)"""
    import nldrmd_emu_check as E
    twin = os.path.join(tmp, "libfittwin.so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-fPIC", "-shared", os.path.join(ROOT, "tools", "userdata_fit_twin.c"), "-o", twin, "-lm"], check=True)
    W, R = C.CDLL(twin), E.ref_bind(C.CDLL(REF))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    best, fs, evals = None, np.zeros(k), 0
    for rep in range(2):
        total = 0.0
        for i in range(k):
            y = np.ascontiguousarray(Y[i])
            fd = FitData(M, T.ctypes.data, y.ctypes.data)
            opt = R.nlopt_create(E.LN_NELDERMEAD if alg is None else alg, 3)
            R.nlopt_set_lower_bounds(opt, dp(LB)); R.nlopt_set_upper_bounds(opt, dp(UB))
            R.nlopt_set_min_objective(opt, C.cast(W.expfit_twin, C.c_void_p), C.addressof(fd))
            R.nlopt_set_xtol_rel(opt, 1e-8); R.nlopt_set_maxeval(opt, 400)
            x, minf = np.array(X0[i]), C.c_double(0)
            t0 = time.perf_counter()
            R.nlopt_optimize(opt, dp(x), C.byref(minf))
            total += time.perf_counter() - t0
            fs[i] = minf.value
            evals += R.nlopt_get_numevals(opt) if rep == 0 else 0
            R.nlopt_destroy(opt)
        best = total / k if best is None else min(best, total / k)
    return best, fs, evals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=4096)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--sample", type=int, default=256)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not os.path.exists(CO) or os.path.getmtime(CO) < os.path.getmtime(SRC):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"),
                        SRC, "-o", CO], check=True)
    count, k = a.count, min(a.count, a.sample)
    Y, X0 = curves(count)
    rows = np.concatenate([np.tile(T, (count, 1)), Y], axis=1)
    lines = ["# python tools/nldrmd_bench.py --count %d --repeats %d --sample %d   (library: %s, %s)"
             % (count, a.repeats, a.sample, os.path.relpath(nlopt_amd.LIB_PATH, ROOT), time.strftime("%Y-%m-%d")),
             "# %d fits of y = a exp(-b t) + c (tests/batch/fit_rows.hip: n = 3, m = %d points), xtol_rel 1e-8, maxeval 400; loops timed over %d fits and scaled"
             % (count, M, k),
             "%-34s %12s %12s %12s %14s" % ("", "time [ms]", "fits/s", "evaluations", "steps (max ev)")]

    def row(what, seconds, evals, steps):
        lines.append("%-34s %12.2f %12.4g %12d %14s" % (what, 1e3 * seconds, count / seconds, evals, steps))
        print(lines[-1], flush=True)
    o = make(nlopt_amd.LN_NELDERMEAD, "expfit_rows")
    assert o.set_device_objective_row_data(rows) > 0, o.get_errmsg()
    tb, (X, minf, res, nev) = timed_batches(o, X0, a.repeats)
    row("LN_NELDERMEAD, one batch", tb, int(nev.sum()), int(nev.max()))
    o.set_param("amd_batch_host_list", 0)                 # the waiting list of every step built on the device instead of by the host loop
    td, (Xd, minfd, _, nevd) = timed_batches(o, X0, a.repeats)
    assert np.array_equal(Xd, X) and np.array_equal(minfd, minf) and np.array_equal(nevd, nev)
    row("  ... with the device-built list", td, int(nevd.sum()), int(nevd.max()))
    b = make(nlopt_amd.LN_NELDERMEAD, "expfit2")
    loop = []
    for rep in range(2):
        t0 = time.perf_counter()
        for i in range(k):
            b.set_device_objective_data(np.concatenate([T, Y[i]]))
            x, f, r = b.optimize_raw(X0[i])
            assert r == res[i] and np.array_equal(x, X[i]) and f == minf[i] and b.get_numevals() == nev[i], (i, r)      # the same fits, bit for bit
        loop.append((time.perf_counter() - t0) * count / k)
    row("LN_NELDERMEAD, loop of lone calls", min(loop), int(nev[:k].sum() * count / k), "")
    if os.path.exists(REF):
        with tempfile.TemporaryDirectory() as tmp:
            per_fit, fs, evals = reference_loop(Y, X0, k, tmp)
        row("reference, 1 CPU thread, C twin", per_fit * count, int(evals * count / k), "")
        lines.append("#   (median |minf - reference's| over the sample: %.3g; the twin sums in another order)" % float(np.median(np.abs(fs - minf[:k]))))
    c = make(nlopt_amd.LN_COBYLA, "expfit_rows")
    assert c.set_device_objective_row_data(rows) > 0, c.get_errmsg()
    tc, (_, _, _, nevc) = timed_batches(c, X0, a.repeats)
    row("LN_COBYLA, one batch", tc, int(nevc.sum()), int(nevc.max()))
    lines.append("# searches of the LN_NELDERMEAD batch without a positive result: %d" % int(np.sum(res <= 0)))
    # the kernel without the coroutine's steps: a compiled-in objective, every search one launch from its start to its end
    r = nlopt_amd.Opt(nlopt_amd.LN_NELDERMEAD, 8)
    r.set_lower_bounds(-2.0)
    r.set_upper_bounds(2.0)
    r.set_min_objective(nlopt_amd.objective("rosenbrock"))
    r.set_xtol_rel(1e-8)
    r.set_maxeval(400)
    tr, (_, _, _, nevr) = timed_batches(r, np.random.default_rng(3).uniform(-1.8, 1.8, (count, 8)), a.repeats)
    row("compiled-in Rosenbrock n = 8, batch", tr, int(nevr.sum()), "1 launch")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
