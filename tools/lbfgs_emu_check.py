"""Development check, CPU only: the two batched L-BFGS kernels (hip/lbfgs_kernels.hip = streaming, hip/lbfgs_resident.hip = resident)
compiled by g++ over tools/simt_emu (one std::thread per work-item) and run on the same starts — the resident kernel must
reproduce the streaming kernel's tree-sum mode BIT FOR BIT (f of every evaluation, minimiser, result, counts), and both must
agree with the oracle's sequential-order search (oracle/port_lbfgs.c) to rounding.  The GPU twin of this check is
tests/test_gpu_lbfgs.py::test_resident_kernel_is_the_streaming_kernel; this one exists so that kernel LOGIC can be debugged
without a GPU.       usage: python tools/lbfgs_emu_check.py [quick | wide]
`wide`: workgroups of 64 threads, so that dimensions 1024 < n <= 2048 take the 32-coordinates-per-thread build of the resident kernel
(hip/lbfgs_resident32.hip: 4096 < n <= 8192 on the device) — the same comparison there.
Also a module: tests/test_lbfgs_emu.py and tests/test_mma_emu.py import build / load (one library per workgroup size LB_T under
tools/_build/, hip/mma_kernels.hip included), run, run_mma and the two Params structs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _oracle as O          # noqa: E402

HIP = os.path.join(ROOT, "nlopt_amd", "csrc", "hip")
EMU = os.path.join(ROOT, "tools", "simt_emu")
SRCS = ("lbfgs_kernels.hip", "lbfgs_resident.hip", "lbfgs_resident32.hip", "mma_kernels.hip")
WIDE_LB_T = 64          # workgroups of 64 threads: 1024 < n <= 2048 takes hip/lbfgs_resident32.hip


class Params(C.Structure):
    """nla_lbfgs_params (include/nlopt_amd.h) — the one copy; tests/test_gpu_lbfgs.py imports it"""
    _fields_ = [("minf_max", C.c_double), ("ftol_rel", C.c_double), ("ftol_abs", C.c_double), ("xtol_rel", C.c_double), ("tolg", C.c_double),
                ("maxeval", C.c_int32), ("exact", C.c_int32), ("sign", C.c_double), ("xtol_abs", C.c_void_p), ("x_weights", C.c_void_p),
                ("abort", C.c_void_p), ("ftrace", C.c_void_p), ("ftrace_cap", C.c_int64), ("done", C.c_void_p)]


class MmaParams(C.Structure):
    """nla_mma_params (include/nlopt_amd.h) — the one copy"""
    _fields_ = [("minf_max", C.c_double), ("ftol_rel", C.c_double), ("ftol_abs", C.c_double), ("xtol_rel", C.c_double), ("rho_init", C.c_double),
                ("sigma_min", C.c_double), ("maxeval", C.c_int32), ("inner_maxeval", C.c_int32), ("inner_gradients", C.c_int32),
                ("always_improve", C.c_int32), ("exact", C.c_int32), ("pad", C.c_int32), ("sign", C.c_double), ("xtol_abs", C.c_void_p),
                ("x_weights", C.c_void_p), ("abort", C.c_void_p), ("ftrace", C.c_void_p), ("ftrace_cap", C.c_int64), ("done", C.c_void_p)]


class Result(C.Structure):
    _fields_ = [("f", C.c_double), ("ret", C.c_int32), ("nevals", C.c_int32), ("iterm", C.c_int32), ("cols", C.c_int32)]


RESULT_DT = [("f", "f8"), ("ret", "i4"), ("nevals", "i4"), ("iterm", "i4"), ("cols", "i4")]


def mma_params(params=None, **kw):
    """MmaParams with the dispatcher's defaults (optimize.c:798-803), `params` (rho_init, sigma_min, inner_maxeval, inner_gradients,
    always_improve) and the stopping values / pointers in kw over them"""
    d = dict(minf_max=-np.inf, ftol_rel=0.0, ftol_abs=0.0, xtol_rel=0.0, rho_init=1.0, sigma_min=0.0, maxeval=0, inner_maxeval=0, inner_gradients=1,
             always_improve=1, exact=0, pad=0, sign=1.0, xtol_abs=None, x_weights=None, abort=None, ftrace=None, ftrace_cap=0, done=None)
    d.update(params or {})
    d.update(kw)
    for k in ("inner_maxeval", "inner_gradients", "always_improve"):
        d[k] = int(d[k])
    return MmaParams(*[d[f[0]] for f in MmaParams._fields_])


def lib_path(lb_t):
    return os.path.join(ROOT, "tools", "_build", "liblocal_emu_T%d.so" % int(lb_t))


def build(lb_t=128):
    """the four kernel sources compiled by g++ over tools/simt_emu with workgroups of lb_t threads: one shared library per lb_t under
    tools/_build/, rebuilt when a source, a header of hip/ or the emulator is newer; returns its path"""
    out = lib_path(lb_t)
    deps = [os.path.join(HIP, s) for s in SRCS] + [os.path.join(HIP, h) for h in ("local_common.h", "dev_common.h")] + \
           [os.path.join(EMU, "hip", "hip_runtime.h"), os.path.join(ROOT, "nlopt_amd", "csrc", "lbfgs_scalar.h"), os.path.join(ROOT, "nlopt_amd", "csrc", "objfuncs.h"),
            os.path.join(ROOT, "include", "nlopt_amd.h")]
    if os.path.exists(out) and all(os.path.getmtime(out) > os.path.getmtime(d) for d in deps):
        return out
    os.makedirs(os.path.dirname(out), exist_ok=True)
    tmp = "%s.%d.tmp" % (out, os.getpid())
    subprocess.run(["g++", "-O1", "-std=c++17", "-DLB_T=%d" % int(lb_t), "-ffp-contract=off", "-fPIC", "-shared", "-x", "c++", "-w", "-I", EMU,
                    "-o", tmp] + [os.path.join(HIP, s) for s in SRCS] + ["-lpthread"], check=True)
    os.replace(tmp, out)
    return out


_LIBS = {}


def load(lb_t=128):
    """the library of build(lb_t), loaded once per process"""
    lb_t = int(lb_t)
    if lb_t not in _LIBS:
        L = C.CDLL(build(lb_t))
        vp = C.c_void_p
        L.nla_k_lbfgs_batch.argtypes = [C.c_int] * 5 + [vp] * 6 + [C.POINTER(Params), vp, vp, vp]
        L.nla_k_mma_batch.argtypes = [C.c_int] * 4 + [vp] * 5 + [C.POINTER(MmaParams), vp, vp, vp]
        _LIBS[lb_t] = L
    return _LIBS[lb_t]


def run(L, streaming, obj, n, starts, lo, hi, mf, ftol_rel=1e-8, maxeval=0, sign=1.0, xtol_abs=None, weights=None, trace_cap=1400, exact=False):
    count, ld = starts.shape[0], (n + 1) & ~1
    X = np.zeros((count, ld)); X[:, :n] = starts
    lb = np.ascontiguousarray(lo, dtype=np.float64); ub = np.ascontiguousarray(hi, dtype=np.float64)
    work = np.zeros(count * (4 * ld + 2 * mf)); iwork = np.zeros(count * ld, dtype=np.int32); hist = np.full(count * 2 * mf * ld, np.nan)
    ft = np.full((count, trace_cap), np.nan)
    res = (Result * count)()
    P = Params(-np.inf, ftol_rel, 0.0, 0.0, 0.0, maxeval, (3 if streaming else 1) if exact else (2 if streaming else 0), sign,
               xtol_abs.ctypes.data if xtol_abs is not None else None, weights.ctypes.data if weights is not None else None, None,
               ft.ctypes.data, trace_cap)
    vp = C.c_void_p
    rc = L.nla_k_lbfgs_batch(O.OBJ[obj], n, ld, mf, count, lb.ctypes.data, ub.ctypes.data, X.ctypes.data, work.ctypes.data, iwork.ctypes.data,
                             hist.ctypes.data, C.byref(P), C.cast(res, vp), None, None)
    assert rc == 0, rc
    return dict(x=X[:, :n].copy(), f=np.array([r.f for r in res]), ret=[r.ret for r in res], nevals=[r.nevals for r in res],
                iterm=[r.iterm for r in res], cols=[r.cols for r in res], ftrace=ft)


def run_mma(L, obj, n, starts, lb, ub, maxeval=0, ftol_rel=0.0, ftol_abs=0.0, xtol_rel=0.0, params=None, sigma_init=None, xtol_abs=None,
            weights=None, sign=1.0, exact=True, trace_cap=700, ld=None, pad=np.nan):
    """nla_k_mma_batch on `starts` (count x n) with a compiled-in objective; sigma_init: a scalar (every coordinate) or n values.
    Returns x, the result rows, the ftrace (indexed by objective calls) and X as the kernel left it (count x ld; the columns behind n
    were filled with `pad`)."""
    starts = np.atleast_2d(np.asarray(starts, dtype=np.float64))
    count, ld = starts.shape[0], ld or (n + 1) & ~1
    X = np.full((count, ld), pad); X[:, :n] = starts
    lbv = np.ascontiguousarray(lb, dtype=np.float64); ubv = np.ascontiguousarray(ub, dtype=np.float64)
    work = np.zeros(count * 6 * ld); ft = np.full((count, trace_cap), np.nan)
    res = (Result * count)()
    sg = None if sigma_init is None else np.ascontiguousarray(np.broadcast_to(np.asarray(sigma_init, dtype=np.float64), (n,)))
    ta = None if xtol_abs is None else np.ascontiguousarray(xtol_abs, dtype=np.float64)
    w = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    P = mma_params(params, maxeval=maxeval, ftol_rel=ftol_rel, ftol_abs=ftol_abs, xtol_rel=xtol_rel, exact=1 if exact else 0, sign=sign,
                   xtol_abs=ta.ctypes.data if ta is not None else None, x_weights=w.ctypes.data if w is not None else None,
                   ftrace=ft.ctypes.data, ftrace_cap=trace_cap)
    rc = L.nla_k_mma_batch(O.OBJ[obj], n, ld, count, lbv.ctypes.data, ubv.ctypes.data, sg.ctypes.data if sg is not None else None, X.ctypes.data,
                           work.ctypes.data, C.byref(P), C.cast(res, C.c_void_p), None, None)
    assert rc == 0, rc
    return dict(x=X[:, :n].copy(), X=X, f=np.array([r.f for r in res]), ret=[r.ret for r in res], nevals=[r.nevals for r in res],
                iterm=[r.iterm for r in res], cols=[r.cols for r in res], ftrace=ft)


def main():
    quick = len(sys.argv) > 1 and sys.argv[1] == "quick"
    WIDE = len(sys.argv) > 1 and sys.argv[1] == "wide"
    L = load(WIDE_LB_T if WIDE else int(os.environ.get("EMU_LB_T", "128")))
    rng = np.random.default_rng(7)
    cases = [("ackley", 300, 3, None, 0), ("rastrigin", 40, 2, 5, 0), ("rosenbrock", 10, 2, None, 0), ("griewank", 257, 2, 3, 0), ("levy", 33, 2, None, 0),
             ("sphere", 5, 2, None, 0), ("ackley", 600, 2, None, 25), ("rastrigin", 513, 2, 4, 0)]
    if quick:
        cases = cases[:3]
    if WIDE:
        cases = [("sphere", 1100, 1, 3, 0), ("rastrigin", 1500, 2, 4, 14), ("ackley", 2048, 1, 3, 10), ("griewank", 1025, 1, 2, 8)]
    bad = 0
    for obj, n, count, mf, maxeval in cases:
        _, lo, hi = O.golden_x0(obj, n)
        lov, hiv = np.full(n, lo), np.full(n, hi)
        starts = rng.uniform(lo, hi, (count, n))
        starts[0, : max(1, n // 7)] = hi            # coordinates on a bound from the start: the active-set paths
        if n > 8:
            lov[3] = hiv[3] = 0.5 * (lo + hi)         # a fixed coordinate
            starts[:, 3] = lov[3]
        m = mf or min(max(1310720 // n, 10), 400)
        a = run(L, True, obj, n, starts, lov, hiv, m, maxeval=maxeval)
        b = run(L, False, obj, n, starts, lov, hiv, m, maxeval=maxeval)

        def identical(a, b):
            return (np.array_equal(a["x"], b["x"]) and np.array_equal(a["f"], b["f"]) and a["ret"] == b["ret"] and a["nevals"] == b["nevals"] and
                    a["iterm"] == b["iterm"] and a["cols"] == b["cols"] and np.array_equal(a["ftrace"], b["ftrace"], equal_nan=True))
        same = identical(a, b)
        # the reference's summation order: streaming kernel (exact = 3) against the resident kernel (exact = 1), and — the emulated device's
        # libm being the host's — against the oracle's search evaluation by evaluation, bit for bit
        xa = run(L, True, obj, n, starts, lov, hiv, m, maxeval=maxeval, exact=True)
        xb = run(L, False, obj, n, starts, lov, hiv, m, maxeval=maxeval, exact=True)
        xsame = identical(xa, xb)
        oracle_same = True
        # the oracle's sequential-order search from the same starts (tolerance: the summation order differs)
        orc = []
        for s in range(count):
            p = O.run_port_lbfgs(obj, n, x0=starts[s], ftol_rel=1e-8, maxeval=maxeval, mf=mf or 0, lb=lov, ub=hiv)
            orc.append((p["minf"], p["nevals"], p["ret"]))
            ft = xb["ftrace"][s][: p["nevals"]]
            if not (xb["nevals"][s] == p["nevals"] and np.array_equal(ft, p["fseq"][: len(ft)]) and np.array_equal(xb["x"][s], p["x"])):
                oracle_same = False          # (Levy: the device's gradient expression groups its four terms differently from the host loop's accumulation)
        near = all(abs(orc[s][0] - b["f"][s]) <= 1e-7 * max(1.0, abs(orc[s][0])) or abs(orc[s][1] - b["nevals"][s]) > 4 for s in range(count))
        print("%-10s n=%-4d mf=%-4d: streaming f=%s evals=%s ret=%s | resident identical: %s | exact order: resident == streaming: %s, == the oracle bit for bit: %s | oracle (minf, evals, ret) %s %s" %
              (obj, n, m, np.array2string(a["f"], precision=12), a["nevals"], a["ret"], same, xsame, oracle_same, orc, "" if near else "  <-- differs from the oracle"))
        if not xsame:
            bad += 1
        if not same:
            bad += 1
            for s in range(count):
                fa, fb = a["ftrace"][s], b["ftrace"][s]
                d = np.nonzero(~((fa == fb) | (np.isnan(fa) & np.isnan(fb))))[0]
                if len(d):
                    print("   search %d: first differing evaluation %d: %r vs %r" % (s, d[0], fa[d[0]], fb[d[0]]))
    print("FAILED" if bad else "ok: resident == streaming bit for bit on %d cases" % len(cases))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
