"""Development check, CPU only: the batched Subplex kernel (hip/sbplx_kernels.hip: hip/nm_search.h with psi > 0 under sbplx_minimize's outer
loop, one wavefront per search) compiled by g++ over tools/simt_emu and run AS A COROUTINE against the REAL reference's
nlopt_optimize(NLOPT_LN_SBPLX) on the same Python objective — tools/nldrmd_emu_check.py with alg = "sbplx": the result code, the evaluation
count, minf, x and the whole sequence of requested (full) points must be IDENTICAL.  `reference` also reads the reference's own trace
(its exported int sbplx_verbose: one line per subspace, one per pass) so that a test can assert which subspace sizes and how many passes
a reference run had.  tests/test_sbplx_emu.py holds the problem list; tests/test_gpu_sbplx.py runs it with device buffers.
       usage: python tools/sbplx_emu_check.py"""
import ctypes as C
import os
import re
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import _oracle as O                                       # noqa: E402
import nldrmd_emu_check as NM                             # noqa: E402
from nldrmd_emu_check import Ext, Params, bits, same, ref_bind, rosenbrock, NLA_OBJ_EXTERNAL      # noqa: E402,F401

LN_SBPLX = 29
ALG = "sbplx"


def build():
    return NM.build(ALG)


def bind(L):
    return NM.bind(L, ALG)


def run_ext(L, n, starts, lo, hi, evaluate, **kw):
    """nldrmd_emu_check.run_ext on nla_k_sbplx_batch"""
    return NM.run_ext(L, n, starts, lo, hi, evaluate, alg=ALG, **kw)


def _captured_stdout(fn):
    """fn() with file descriptor 1 redirected into a file: what C code printed meanwhile, and fn's result"""
    sys.stdout.flush()
    keep = os.dup(1)
    with tempfile.TemporaryFile() as tmp:
        os.dup2(tmp.fileno(), 1)
        try:
            out = fn()
        finally:
            C.CDLL(None).fflush(None)                     # (the C library's buffer for stdout, which is a file now: fully buffered)
            os.dup2(keep, 1)
            os.close(keep)
        tmp.seek(0)
        return out, tmp.read().decode()


_SUB = re.compile(r"(\d+) NM iterations for \((\d+),(\d+)\) subspace")


def reference(n, starts, lo, hi, evaluate, R=None, **kw):
    """nldrmd_emu_check.reference with NLOPT_LN_SBPLX.  On the real reference (R None) the runs go with sbplx_verbose = 1 and the result
    has `subspaces` (per run: the (is, ns, evaluations) of every inner search in order) and `passes` (per run: the number of "stepsize
    scale factor" lines, one per completed pass)"""
    if R is not None:
        return NM.reference(n, starts, lo, hi, evaluate, R=R, alg=LN_SBPLX, **kw)
    R = O.ref()
    verbose = C.c_int.in_dll(R, "sbplx_verbose")
    starts = np.asarray(starts, dtype=np.float64).reshape(-1, n)
    ev = evaluate if isinstance(evaluate, (list, tuple)) else [evaluate] * len(starts)
    outs, subs, passes = [], [], []
    for s, fn in zip(starts, ev):
        verbose.value = 1
        try:
            r, text = _captured_stdout(lambda: NM.reference(n, [s], lo, hi, fn, alg=LN_SBPLX, **kw))
        finally:
            verbose.value = 0
        outs.append(r)
        subs.append([(int(m.group(2)), int(m.group(3)), int(m.group(1))) for m in _SUB.finditer(text)])
        passes.append(text.count("stepsize scale factor"))
    out = dict((k, [o[k][0] for o in outs]) for k in outs[0])
    out["x"], out["f"] = np.array(out["x"]), np.array(out["f"])
    out["subspaces"], out["passes"] = subs, passes
    return out


def main():
    K = C.CDLL(build())
    bad = 0
    for n, maxeval in ((1, 60), (2, 200), (5, 300), (7, 600), (65, 900)):
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
        print("n=%-3d kernel ret %s nevals %s f %s | reference ret %s nevals %s f %s passes %s sizes %s  %s"
              % (n, a["ret"], a["nevals"], a["f"], r["ret"], r["nevals"], r["f"], r["passes"], sorted(set(q[1] for q in r["subspaces"][0])),
                 "IDENTICAL" if ok else "DIFFERENT"), flush=True)
        bad += 0 if ok else 1
    print("sbplx emu check:", "ok" if bad == 0 else "%d case(s) differ" % bad)
    return bad


if __name__ == "__main__":
    sys.exit(main())
