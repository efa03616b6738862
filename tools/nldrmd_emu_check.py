"""Development check, CPU only: the batched Nelder-Mead kernel (hip/nldrmd_kernels.hip, one wavefront per search) compiled by g++ over
tools/simt_emu (one std::thread per lane, barriers where the kernel has them) and run AS A COROUTINE — this file is the host side of
the "External evaluation" contract (include/nlopt_amd.h): launch, read req, evaluate every waiting row of EX, write EF, launch again
with resume = 1 — against the REAL reference's nlopt_optimize(NLOPT_LN_NELDERMEAD) on the same Python objective.  Both are handed
identical values, so the result code, the evaluation count, minf, x and the whole sequence of requested points must be IDENTICAL.
tests/test_nldrmd_emu.py holds the problem list; tests/test_gpu_nldrmd.py runs it with device buffers through libnlopt_amd.so.
       usage: python tools/nldrmd_emu_check.py"""
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

HIP = os.path.join(ROOT, "nlopt_amd", "csrc", "hip")
OUT = os.path.join(ROOT, "tools", "_build", "libnldrmd_emu.so")
LN_NELDERMEAD, NLA_OBJ_EXTERNAL = 28, -1


class Params(C.Structure):
    """nla_nldrmd_params (include/nlopt_amd.h)"""
    _fields_ = [("minf_max", C.c_double), ("ftol_rel", C.c_double), ("ftol_abs", C.c_double), ("xtol_rel", C.c_double),
                ("maxeval", C.c_int32), ("exact", C.c_int32), ("sign", C.c_double), ("xtol_abs", C.c_void_p), ("x_weights", C.c_void_p),
                ("abort", C.c_void_p), ("ftrace", C.c_void_p), ("ftrace_cap", C.c_int64), ("done", C.c_void_p)]


def build(alg="nldrmd"):
    """alg: "nldrmd" (hip/nldrmd_kernels.hip) or "sbplx" (hip/sbplx_kernels.hip, tools/sbplx_emu_check.py): the same search body"""
    out = OUT.replace("nldrmd", alg)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    srcs = [os.path.join(HIP, alg + "_kernels.hip")]
    deps = srcs + [os.path.join(HIP, h) for h in ("nm_search.h", "cobyla_search.h", "local_common.h", "dev_common.h")] + [os.path.join(ROOT, "include", "nlopt_amd.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(s) for s in deps):
        return out
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++", "-w", "-I", os.path.join(ROOT, "tools", "simt_emu"),
                    "-o", out] + srcs + ["-lpthread"], check=True)
    return out


def bind(L, alg="nldrmd"):
    vp = C.c_void_p
    serves, work, save, batch = (getattr(L, nm % alg) for nm in ("nla_%s_serves", "nla_%s_work_doubles", "nla_%s_save_bytes", "nla_k_%s_batch"))
    serves.restype = C.c_int; serves.argtypes = [C.c_int]
    work.restype = C.c_size_t; work.argtypes = [C.c_int, C.c_int]
    save.restype = C.c_size_t; save.argtypes = [C.c_int]
    batch.restype = C.c_int
    batch.argtypes = [C.c_int] * 4 + [vp] * 5 + [C.POINTER(Params), vp, C.POINTER(Ext), vp]
    return L


def run_ext(L, n, starts, lo, hi, evaluate, dx=None, xtol_rel=0.0, xtol_abs=None, x_weights=None, ftol_rel=0.0, ftol_abs=0.0, maxeval=0,
            minf_max=-np.inf, forced_from=None, timeout_from=None, mem=None, max_steps=100000, alg="nldrmd"):
    """the host side of the coroutine nla_k_nldrmd_batch(NLA_OBJ_EXTERNAL): launch, read req, evaluate every waiting row of EX — with
    `evaluate`, or with evaluate[i] for search i —, launch again with resume = 1 until no search waits.  forced_from / timeout_from = k:
    ext.forced / ext.timeout = 1 from the k-th relaunch on (the first launch is number 0; relaunch k delivers the k-th value).
    alg = "sbplx": nla_k_sbplx_batch, the same contract.
    `asked`: per search, the points it requested in order; `finished_at`: the launch after which its state was 2; `seen`: the states
    after every launch."""
    bind(L, alg)
    work_doubles, save_bytes, batch = (getattr(L, nm % alg) for nm in ("nla_%s_work_doubles", "nla_%s_save_bytes", "nla_k_%s_batch"))
    mem = mem or HostMem()
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, n)
    count, ld = starts.shape[0], (n + 1) & ~1
    ev = evaluate if isinstance(evaluate, (list, tuple)) else [evaluate] * count
    X = np.zeros((count, ld)); X[:, :n] = starts
    bX, bl, bu = mem.put(X), mem.put(np.asarray(lo, dtype=np.float64)), mem.put(np.asarray(hi, dtype=np.float64))
    opt = [mem.put(np.asarray(a, dtype=np.float64)) if a is not None else None for a in (dx, xtol_abs, x_weights)]
    bd, bxa, bxw = opt
    # 0xff (NaN) everywhere a starting search must not rely on: it writes its slice and its record before it reads them
    bw = mem.alloc(8 * work_doubles(n, count), 0xff)
    bsave, breq = mem.alloc(save_bytes(n) * count, 0xff), mem.put(np.zeros((count, 2), dtype=np.int32))
    bEX, bEG, bEF = mem.put(np.full((count, ld), np.nan)), mem.put(np.full(8, np.nan)), mem.put(np.full(count, np.nan))
    bo = mem.alloc(C.sizeof(Result) * count)
    P = Params(minf_max, ftol_rel, ftol_abs, xtol_rel, maxeval, 0, 1.0, bxa.ptr if bxa else None, bxw.ptr if bxw else None, None, None, 0, None)
    E = Ext(breq.ptr, bEX.ptr, bEG.ptr, bEF.ptr, bsave.ptr, 0, 0, 0, 0)
    asked, fseq, finished_at, seen, step = [[] for _ in range(count)], [[] for _ in range(count)], [None] * count, [], 0
    while True:
        E.forced = 1 if forced_from is not None and step >= forced_from else 0
        E.timeout = 1 if timeout_from is not None and step >= timeout_from else 0
        rc = batch(NLA_OBJ_EXTERNAL, n, ld, count, bl.ptr, bu.ptr, bd.ptr if bd else None, bX.ptr, bw.ptr, C.byref(P), bo.ptr, C.byref(E), None)
        assert rc == 0, rc
        mem.sync()
        state = mem.read(breq, np.int32, 2 * count).reshape(count, 2)[:, 0]
        seen.append(state.copy())
        for i in range(count):
            if state[i] == 2 and finished_at[i] is None:
                finished_at[i] = step
        waiting = [i for i in range(count) if state[i] == 1]
        if not waiting:
            break
        assert step < max_steps
        EX, EF = mem.read(bEX, np.float64, count * ld).reshape(count, ld), mem.read(bEF, np.float64, count)
        for i in waiting:
            asked[i].append(EX[i, :n].copy())
            EF[i] = ev[i](EX[i, :n].copy())
            fseq[i].append(EF[i])
        mem.write(bEF, EF)
        E.resume = 1
        step += 1
    res = (Result * count).from_buffer_copy(mem.read(bo, np.uint8, C.sizeof(Result) * count).tobytes())
    return dict(x=mem.read(bX, np.float64, count * ld).reshape(count, ld)[:, :n].copy(), f=np.array([r.f for r in res]), ret=[r.ret for r in res],
                nevals=[r.nevals for r in res], cols=[r.cols for r in res], asked=asked, fseq=fseq, finished_at=finished_at, seen=seen, launches=step + 1)


def ref_bind(R):
    """the part of the NLopt C API `reference` uses, on any library that has it (the real reference, libnlopt_amd.so)"""
    vp, dp = C.c_void_p, C.POINTER(C.c_double)
    R.nlopt_create.restype = vp; R.nlopt_create.argtypes = [C.c_int, C.c_uint]
    R.nlopt_destroy.argtypes = [vp]
    R.nlopt_optimize.argtypes = [vp, dp, dp]
    R.nlopt_set_min_objective.argtypes = [vp, vp, vp]; R.nlopt_set_max_objective.argtypes = [vp, vp, vp]
    for nm in ("nlopt_set_lower_bounds", "nlopt_set_upper_bounds", "nlopt_set_xtol_abs", "nlopt_set_initial_step", "nlopt_set_x_weights"):
        getattr(R, nm).argtypes = [vp, dp]
    for nm in ("nlopt_set_stopval", "nlopt_set_ftol_rel", "nlopt_set_ftol_abs", "nlopt_set_xtol_rel", "nlopt_set_maxtime"):
        getattr(R, nm).argtypes = [vp, C.c_double]
    R.nlopt_set_maxeval.argtypes = [vp, C.c_int]
    R.nlopt_get_numevals.argtypes = [vp]
    R.nlopt_force_stop.argtypes = [vp]
    R.nlopt_add_inequality_constraint.argtypes = [vp, vp, vp, C.c_double]
    R.nlopt_set_local_optimizer.argtypes = [vp, vp]
    R.nlopt_get_errmsg.restype = C.c_char_p; R.nlopt_get_errmsg.argtypes = [vp]
    return R


def reference(n, starts, lo, hi, evaluate, dx=None, xtol_rel=0.0, xtol_abs=None, x_weights=None, ftol_rel=0.0, ftol_abs=0.0, maxeval=0,
              minf_max=None, force_at=None, maximise=False, R=None, alg=LN_NELDERMEAD, setup=None):
    """the starts one after another through nlopt_optimize(NLOPT_LN_NELDERMEAD) of R (default: the real reference); the callback records
    every point it is given and (force_at = k) calls nlopt_force_stop inside its k-th call.  setup(R, opt): further settings of the
    optimiser before the run (what it returns is kept alive until the optimiser is destroyed)"""
    R = ref_bind(R or O.ref())
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, n)
    ev = evaluate if isinstance(evaluate, (list, tuple)) else [evaluate] * len(starts)
    keep = [np.ascontiguousarray(a, dtype=np.float64) if a is not None else None for a in (lo, hi, dx, xtol_abs, x_weights)]
    lo, hi, dx, xtol_abs, x_weights = keep
    out = dict(x=[], f=[], ret=[], nevals=[], asked=[], fseq=[], errmsg=[])
    for s, fn in zip(starts, ev):
        opt = R.nlopt_create(alg, n)
        pts, fs = [], []

        def cb(nn, x, g, d):
            pts.append(np.array(x[:nn], dtype=np.float64))
            if force_at is not None and len(pts) == force_at:
                R.nlopt_force_stop(opt)
            fs.append(float(fn(pts[-1])))
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
        if minf_max is not None:
            R.nlopt_set_stopval(opt, minf_max)
        if dx is not None:
            R.nlopt_set_initial_step(opt, O.dptr(dx))
        alive = setup(R, opt) if setup else None
        x, minf = np.array(s, dtype=np.float64), C.c_double(0)
        out["ret"].append(R.nlopt_optimize(opt, O.dptr(x), C.byref(minf)))
        out["f"].append(minf.value); out["x"].append(x); out["nevals"].append(R.nlopt_get_numevals(opt)); out["asked"].append(pts); out["fseq"].append(fs)
        out["errmsg"].append(R.nlopt_get_errmsg(opt))
        R.nlopt_destroy(opt)
        del alive
    out["x"], out["f"] = np.array(out["x"]), np.array(out["f"])
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, r):
    """results and, per search, the sequence of requested points: the reference's, bit for bit"""
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"], (a["ret"], r["ret"], a["nevals"], r["nevals"])
    assert np.array_equal(bits(a["f"]), bits(r["f"])) and np.array_equal(bits(a["x"]), bits(r["x"])), (a["f"], r["f"], a["x"], r["x"])
    for pa, pr in zip(a["asked"], r["asked"]):
        assert len(pa) == len(pr) and all(np.array_equal(bits(u), bits(v)) for u, v in zip(pa, pr))


def rosenbrock(x):
    s = 0.0
    for i in range(len(x) - 1):
        a, b = x[i + 1] - x[i] * x[i], 1.0 - x[i]
        s += 100.0 * a * a + b * b
    return s


def main():
    K = C.CDLL(build())
    bad = 0
    for n, maxeval in ((1, 60), (2, 200), (5, 150), (65, 120)):
        lo, hi = np.full(n, -2.0), np.full(n, 2.0)
        starts = np.random.default_rng(100 + n).uniform(-1.5, 1.5, (2, n))
        f = rosenbrock if n > 1 else (lambda x: (x[0] - 0.3) * (x[0] - 0.3))
        a = run_ext(K, n, starts, lo, hi, f, xtol_rel=1e-6, maxeval=maxeval)
        r = reference(n, starts, lo, hi, f, xtol_rel=1e-6, maxeval=maxeval)
        try:
            same(a, r)
            ok = True
        except AssertionError:
            ok = False
        print("n=%-3d kernel ret %s nevals %s f %s | reference ret %s nevals %s f %s  %s"
              % (n, a["ret"], a["nevals"], a["f"], r["ret"], r["nevals"], r["f"], "IDENTICAL" if ok else "DIFFERENT"), flush=True)
        bad += 0 if ok else 1
    print("nldrmd emu check:", "ok" if bad == 0 else "%d case(s) differ" % bad)
    return bad


if __name__ == "__main__":
    sys.exit(main())
