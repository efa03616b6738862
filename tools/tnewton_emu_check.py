"""Development check, CPU only: the batched truncated-Newton kernel (hip/tnewton_kernels.hip, NLOPT_LD_TNEWTON and its three variants, one
workgroup per search) compiled by g++ over tools/simt_emu with workgroups of 64 host threads (-DLB_T=64) and run
  * AS A COROUTINE on Python objectives — this file is the host side of the "External evaluation" contract (include/nlopt_amd.h): launch,
    read req, evaluate every waiting row of EX, write EF and the row of EG, launch again with resume = 1 — against the REAL reference's
    nlopt_optimize(ids 15 .. 18) on the same callback, which records every point it is asked for (the CG probes included).  In
    exact-order mode both are handed identical values, so the result code, the evaluation count, every requested point, minf and x
    must be IDENTICAL;
  * as a WHOLE SEARCH on the compiled-in objectives (run), in tree-sum or exact-order mode.
tests/test_tnewton_emu.py holds the problem list; tests/test_gpu_tnewton.py runs it through libnlopt_amd.so on the device.
       usage: python tools/tnewton_emu_check.py [tree]
`tree`: the tree-sum mode's deviation from the reference on sphere 5, wquad4 65 and rosenbrock 10 (the table of DESIGN.md)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _oracle as O                                       # noqa: E402
from cobyla_emu_check import Ext, HostMem, Result         # noqa: E402  (nla_local_ext, nla_lbfgs_result, run_ext's buffers in host memory)
from lbfgs_emu_check import Params                        # noqa: E402  (nla_lbfgs_params: the launcher takes LD_LBFGS's record)
from nldrmd_emu_check import bits, ref_bind               # noqa: E402

HIP = os.path.join(ROOT, "nlopt_amd", "csrc", "hip")
EMU = os.path.join(ROOT, "tools", "simt_emu")
OUT = os.path.join(ROOT, "tools", "_build", "libtnewton_emu_T%d.so")
LD_TNEWTON, NLA_OBJ_EXTERNAL = 15, -1
IDS = (15, 16, 17, 18)
MEMAVAIL = 1310720


def default_mf(n, vector_storage=0, maxeval=0):
    """nla_lbfgs_default_mf (pnet.c:590-594)"""
    mf = vector_storage
    if mf <= 0:
        mf = max(MEMAVAIL // n, 10)
        if 0 < maxeval <= mf:
            mf = max(maxeval, 1)
    return mf


def build(lb_t=64):
    out = OUT % lb_t
    srcs = [os.path.join(HIP, "tnewton_kernels.hip")]
    deps = srcs + [os.path.join(HIP, h) for h in ("luksan_bounds.h", "local_common.h", "dev_common.h")] + \
           [os.path.join(EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "nlopt_amd", "csrc", "lbfgs_scalar.h"), os.path.join(ROOT, "nlopt_amd", "csrc", "objfuncs.h"),
            os.path.join(ROOT, "include", "nlopt_amd.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.run(["g++", "-O1", "-std=c++17", "-DLB_T=%d" % lb_t, "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++", "-w", "-I", EMU, "-o", tmp] + srcs +
                   ["-lpthread"], check=True)
    os.replace(tmp, out)
    return out


def bind(L):
    vp = C.c_void_p
    for nm in ("nla_tnewton_work_doubles", "nla_tnewton_hist_doubles"):
        getattr(L, nm).restype = C.c_size_t; getattr(L, nm).argtypes = [C.c_int] * 3
    L.nla_tnewton_save_bytes.restype = C.c_size_t; L.nla_tnewton_save_bytes.argtypes = []
    L.nla_k_tnewton_batch.restype = C.c_int
    L.nla_k_tnewton_batch.argtypes = [C.c_int] * 6 + [vp] * 6 + [C.POINTER(Params), vp, C.POINTER(Ext), vp]
    return L


def _mf_of(alg, n, vector_storage, maxeval):
    return default_mf(n, vector_storage, maxeval) if alg >= 17 else 0         # (the ids without preconditioner keep no history)


def run_ext(L, alg, n, starts, lo, hi, evaluate, xtol_rel=0.0, xtol_abs=None, x_weights=None, ftol_rel=0.0, ftol_abs=0.0, maxeval=0,
            minf_max=-np.inf, vector_storage=0, tolg=0.0, exact=1, forced_from=None, timeout_from=None, mem=None, max_steps=100000):
    """the host side of the coroutine nla_k_tnewton_batch(NLA_OBJ_EXTERNAL): launch, read req, evaluate every waiting row of EX with
    `evaluate` (x -> (f, gradient)), or evaluate[i] for search i, launch again with resume = 1 until no search waits.  forced_from /
    timeout_from = k: ext.forced / ext.timeout = 1 from the k-th relaunch on (relaunch k delivers the k-th value).
    `asked`: per search, the points it requested in order; `fseq`: the values delivered."""
    bind(L)
    mem = mem or HostMem()
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, n)
    count, ld, mf = starts.shape[0], (n + 1) & ~1, _mf_of(alg, n, vector_storage, maxeval)
    ev = evaluate if isinstance(evaluate, (list, tuple)) else [evaluate] * count
    X = np.zeros((count, ld)); X[:, :n] = starts
    bX, bl, bu = mem.put(X), mem.put(np.asarray(lo, dtype=np.float64)), mem.put(np.asarray(hi, dtype=np.float64))
    bxa, bxw = [mem.put(np.asarray(a, dtype=np.float64)) if a is not None else None for a in (xtol_abs, x_weights)]
    # 0xff (NaN) everywhere a starting search must not rely on
    bw = mem.alloc(8 * L.nla_tnewton_work_doubles(ld, mf, count), 0xff)
    bh = mem.alloc(8 * L.nla_tnewton_hist_doubles(ld, mf, count), 0xff)
    biw = mem.alloc(4 * ld * count, 0xff)
    bsave, breq = mem.alloc(L.nla_tnewton_save_bytes() * count, 0xff), mem.put(np.zeros((count, 2), dtype=np.int32))
    bEX, bEG, bEF = mem.put(np.full((count, ld), np.nan)), mem.put(np.full((count, ld), np.nan)), mem.put(np.full(count, np.nan))
    bo = mem.alloc(C.sizeof(Result) * count)
    P = Params(minf_max, ftol_rel, ftol_abs, xtol_rel, tolg, maxeval, exact, 1.0, bxa.ptr if bxa else None, bxw.ptr if bxw else None, None, None, 0, None)
    E = Ext(breq.ptr, bEX.ptr, bEG.ptr, bEF.ptr, bsave.ptr, 0, 0, 0, 0)
    asked, fseq, finished_at, seen, step = [[] for _ in range(count)], [[] for _ in range(count)], [None] * count, [], 0
    while True:
        E.forced = 1 if forced_from is not None and step >= forced_from else 0
        E.timeout = 1 if timeout_from is not None and step >= timeout_from else 0
        rc = L.nla_k_tnewton_batch(NLA_OBJ_EXTERNAL, n, ld, mf, alg - LD_TNEWTON, count, bl.ptr, bu.ptr, bX.ptr, bw.ptr, biw.ptr, bh.ptr if mf else None,
                                   C.byref(P), bo.ptr, C.byref(E), None)
        assert rc == 0, rc
        mem.sync()
        req = mem.read(breq, np.int32, 2 * count).reshape(count, 2)
        state = req[:, 0]
        seen.append(state.copy())
        for i in range(count):
            if state[i] == 2 and finished_at[i] is None:
                finished_at[i] = step
        waiting = [i for i in range(count) if state[i] == 1]
        if not waiting:
            break
        assert step < max_steps
        EX, EF = mem.read(bEX, np.float64, count * ld).reshape(count, ld), mem.read(bEF, np.float64, count)
        EG = mem.read(bEG, np.float64, count * ld).reshape(count, ld)
        for i in waiting:
            assert req[i, 1] == 1
            asked[i].append(EX[i, :n].copy())
            f, g = ev[i](EX[i, :n].copy())
            EF[i] = f; EG[i, :n] = g
            fseq[i].append(float(f))
        mem.write(bEF, EF); mem.write(bEG, EG)
        E.resume = 1
        step += 1
    res = (Result * count).from_buffer_copy(mem.read(bo, np.uint8, C.sizeof(Result) * count).tobytes())
    return dict(x=mem.read(bX, np.float64, count * ld).reshape(count, ld)[:, :n].copy(), f=np.array([r.f for r in res]), ret=[r.ret for r in res],
                nevals=[r.nevals for r in res], iterm=[r.iterm for r in res], asked=asked, fseq=fseq, finished_at=finished_at, seen=seen, launches=step + 1)


def run(L, alg, obj, n, starts, lo, hi, exact=0, xtol_rel=0.0, ftol_rel=0.0, ftol_abs=0.0, maxeval=0, minf_max=-np.inf, vector_storage=0, tolg=0.0,
        sign=1.0, trace_cap=2000):
    """nla_k_tnewton_batch on `starts` (count x n) with a compiled-in objective: a whole search per workgroup"""
    bind(L)
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, n)
    count, ld, mf = starts.shape[0], (n + 1) & ~1, _mf_of(alg, n, vector_storage, maxeval)
    X = np.zeros((count, ld)); X[:, :n] = starts
    lb = np.ascontiguousarray(lo, dtype=np.float64); ub = np.ascontiguousarray(hi, dtype=np.float64)
    work = np.full(max(1, L.nla_tnewton_work_doubles(ld, mf, count)), np.nan); hist = np.full(max(1, L.nla_tnewton_hist_doubles(ld, mf, count)), np.nan)
    iwork = np.zeros(count * ld, dtype=np.int32)
    ft = np.full((count, trace_cap), np.nan)
    res = (Result * count)()
    P = Params(minf_max, ftol_rel, ftol_abs, xtol_rel, tolg, maxeval, exact, sign, None, None, None, ft.ctypes.data, trace_cap, None)
    rc = L.nla_k_tnewton_batch(O.OBJ[obj], n, ld, mf, alg - LD_TNEWTON, count, lb.ctypes.data, ub.ctypes.data, X.ctypes.data, work.ctypes.data,
                               iwork.ctypes.data, hist.ctypes.data if mf else None, C.byref(P), C.cast(res, C.c_void_p), None, None)
    assert rc == 0, rc
    return dict(x=X[:, :n].copy(), f=np.array([r.f for r in res]), ret=[r.ret for r in res], nevals=[r.nevals for r in res], iterm=[r.iterm for r in res],
                ftrace=ft)


def reference(alg, n, starts, lo, hi, evaluate, xtol_rel=0.0, xtol_abs=None, x_weights=None, ftol_rel=0.0, ftol_abs=0.0, maxeval=0, minf_max=None,
              vector_storage=0, maxtime=0.0, force_at=None, maximise=False, R=None, setup=None):
    """the starts one after another through nlopt_optimize(alg) of R (default: the real reference); the callback (x -> (f, gradient))
    records every point it is given and (force_at = k) calls nlopt_force_stop inside its k-th call.  setup(R, opt): further settings of
    the optimiser before the run (what it returns is kept alive until the optimiser is destroyed)"""
    R = ref_bind(R or O.ref())
    R.nlopt_set_vector_storage.argtypes = [C.c_void_p, C.c_uint]
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, n)
    ev = evaluate if isinstance(evaluate, (list, tuple)) else [evaluate] * len(starts)
    lo, hi, xtol_abs, x_weights = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (lo, hi, xtol_abs, x_weights)]
    out = dict(x=[], f=[], ret=[], nevals=[], asked=[], fseq=[])
    for s, fn in zip(starts, ev):
        opt = R.nlopt_create(alg, n)
        pts, fs = [], []

        def cb(nn, x, g, d):
            pts.append(np.array(x[:nn], dtype=np.float64))
            if force_at is not None and len(pts) == force_at:
                R.nlopt_force_stop(opt)
            f, grad = fn(pts[-1])
            if g:
                for i in range(nn):
                    g[i] = grad[i]
            fs.append(float(f))
            return fs[-1]
        fcb = O.FUNC(cb)
        R.nlopt_set_lower_bounds(opt, O.dptr(lo)); R.nlopt_set_upper_bounds(opt, O.dptr(hi))
        (R.nlopt_set_max_objective if maximise else R.nlopt_set_min_objective)(opt, C.cast(fcb, C.c_void_p), None)
        if xtol_rel:
            R.nlopt_set_xtol_rel(opt, xtol_rel)
        if xtol_abs is not None:
            R.nlopt_set_xtol_abs(opt, O.dptr(xtol_abs))
        if x_weights is not None:
            R.nlopt_set_x_weights(opt, O.dptr(x_weights))
        if ftol_rel:
            R.nlopt_set_ftol_rel(opt, ftol_rel)
        if ftol_abs:
            R.nlopt_set_ftol_abs(opt, ftol_abs)
        if maxeval:
            R.nlopt_set_maxeval(opt, maxeval)
        if maxtime:
            R.nlopt_set_maxtime(opt, maxtime)
        if minf_max is not None:
            R.nlopt_set_stopval(opt, minf_max)
        if vector_storage:
            R.nlopt_set_vector_storage(opt, vector_storage)
        alive = setup(R, opt) if setup else None
        x, minf = np.array(s, dtype=np.float64), C.c_double(0)
        out["ret"].append(R.nlopt_optimize(opt, O.dptr(x), C.byref(minf)))
        out["f"].append(minf.value); out["x"].append(x); out["nevals"].append(R.nlopt_get_numevals(opt)); out["asked"].append(pts); out["fseq"].append(fs)
        R.nlopt_destroy(opt)
        del alive
    out["x"], out["f"] = np.array(out["x"]), np.array(out["f"])
    return out


def same(a, r):
    """results and, per search, the sequence of requested points and delivered values: the reference's, bit for bit"""
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"], (a["ret"], r["ret"], a["nevals"], r["nevals"])
    for pa, pr in zip(a["asked"], r["asked"]):
        assert len(pa) == len(pr), (len(pa), len(pr))
        for k, (u, v) in enumerate(zip(pa, pr)):
            assert np.array_equal(bits(u), bits(v)), (k, u, v)
    for fa, fr in zip(a["fseq"], r["fseq"]):
        assert np.array_equal(bits(fa), bits(fr))
    assert np.array_equal(bits(a["f"]), bits(r["f"])) and np.array_equal(bits(a["x"]), bits(r["x"])), (a["f"], r["f"], a["x"], r["x"])


# ---- the objectives of the problem list: x -> (f, gradient) ------------------------------------------------------------------------------
def rosen(x):
    n, f, g = len(x), 0.0, np.zeros(len(x))
    for i in range(n - 1):
        a, b = x[i + 1] - x[i] * x[i], 1.0 - x[i]
        f += 100.0 * a * a + b * b
        g[i] += -400.0 * a * x[i] - 2.0 * b
        g[i + 1] += 200.0 * a
    return f, g


def wquad4(x):
    i = np.arange(len(x))
    w, d = 10.0 ** (i % 4), x - 0.1 * (i % 7)
    return float(np.sum(w * d * d)), 2 * w * d


def rastr(x):
    return float(10 * len(x) + np.sum(x * x - 10 * np.cos(2 * np.pi * x))), 2 * x + 20 * np.pi * np.sin(2 * np.pi * x)


def sphere(x):
    f = 0.0
    for v in x:
        f += v * v
    return f, 2 * x


def parabola(x):
    return (x[0] - 0.3) * (x[0] - 0.3), np.array([2.0 * (x[0] - 0.3)])


def tree_problems():
    """the three problems of the tree-sum comparison: (name, compiled-in objective or None, callback, n, x0, lb, ub)"""
    out = []
    for obj, n, fn in (("sphere", 5, sphere), ("rosenbrock", 10, rosen)):
        x0, lo, hi = O.golden_x0(obj, n)
        out.append((obj + str(n), fn, n, np.array(x0, dtype=np.float64), np.full(n, float(lo)), np.full(n, float(hi))))
    out.insert(1, ("wquad4_65", wquad4, 65, np.random.default_rng(65).uniform(-1.5, 1.5, 65), np.full(65, -2.0), np.full(65, 2.0)))
    return out


def tree_deviation(L):
    """tree-sum mode (exact = 0) of the coroutine kernel against the reference: per problem the largest |minf - minf_ref|, the largest
    |x - x_ref|_inf and the largest ratio of evaluation counts over the four ids"""
    rows = []
    for name, fn, n, x0, lo, hi in tree_problems():
        dm = dx = ratio = 0.0
        for alg in IDS:
            r = reference(alg, n, [x0], lo, hi, fn)
            a = run_ext(L, alg, n, [x0], lo, hi, fn, exact=0)
            assert r["ret"][0] > 0
            dm = max(dm, abs(a["f"][0] - r["f"][0])); dx = max(dx, float(np.max(np.abs(a["x"][0] - r["x"][0]))))
            ratio = max(ratio, a["nevals"][0] / r["nevals"][0], r["nevals"][0] / a["nevals"][0])
            print("  %-12s id %d: kernel ret %d nevals %d minf %.17g | reference ret %d nevals %d minf %.17g" %
                  (name, alg, a["ret"][0], a["nevals"][0], a["f"][0], r["ret"][0], r["nevals"][0], r["f"][0]))
        rows.append((name, dm, dx, ratio, float(np.max(np.abs(r["x"][0])))))
    return rows


def main():
    L = C.CDLL(build())
    if len(sys.argv) > 1 and sys.argv[1] == "tree":
        for name, dm, dx, ratio, xr in tree_deviation(L):
            print("%-12s max |minf - ref| %.3e   max |x - ref|_inf %.3e (|x_ref|_inf %.3g)   max evaluation ratio %.3f" % (name, dm, dx, xr, ratio))
        return 0
    bad = 0
    cases = [("rosen2", rosen, 2, [-1.2, 1.0], np.full(2, -np.inf), np.full(2, np.inf)),
             ("rosen10", rosen, 10, np.full(10, -1.0), np.full(10, -1.5), np.full(10, 0.5)),
             ("rastr5", rastr, 5, [2.3, -1.7, 0.6, 3.4, -4.2], np.full(5, -5.12), np.full(5, 5.12)),
             ("wquad65", wquad4, 65, np.random.default_rng(65).uniform(-1.5, 1.5, 65), np.full(65, -2.0), np.full(65, 2.0))]
    for name, fn, n, x0, lo, hi in cases:
        for alg in IDS:
            r = reference(alg, n, [x0], lo, hi, fn)
            a = run_ext(L, alg, n, [x0], lo, hi, fn)
            try:
                same(a, r)
                ok = True
            except AssertionError as e:
                ok = False
                print("   ", str(e)[:300])
            print("%-8s id %d: kernel ret %s nevals %s f %s | reference ret %s nevals %s f %s  %s" %
                  (name, alg, a["ret"], a["nevals"], a["f"], r["ret"], r["nevals"], r["f"], "IDENTICAL" if ok else "DIFFERENT"), flush=True)
            bad += 0 if ok else 1
    print("tnewton emu check:", "ok" if bad == 0 else "%d case(s) differ" % bad)
    return bad


if __name__ == "__main__":
    sys.exit(main())
