"""CPU twin of tests/test_gpu_cobyla_global.py: hip/cobyla_global.hip (the batched LN_COBYLA search of hip/cobyla_search.h with its five
matrices in a global-memory workspace: the dimensions beyond the LDS kernel's 51) compiled by g++ over tools/simt_emu — 64 lockstep
threads, barriers where the kernel has them — against the REAL reference's nlopt_optimize(LN_COBYLA) on the objective's host twin.  In
exact-order mode (sphere / Rosenbrock: no transcendental) the result code, the evaluation count, f and the minimiser are the
reference's bit for bit.  What this cannot see is the device's memory model: the GPU twin runs the same comparison on the MI355X."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

import _oracle as O
import test_cobyla_differential as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GLOBAL = "nla_k_cobyla_batch_global"

pytestmark = pytest.mark.skipif(not shutil.which("g++") or not O.have_ref() or not os.path.exists(T.EMU), reason="no g++ / oracle/_ref / emulated library here")


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import cobyla_emu_check as E
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return E


@pytest.fixture(scope="module")
def kernels():
    E = _tool()
    return E, C.CDLL(E.build_global()), C.CDLL(E.build())


def reference(obj, n, starts, lb, ub, xtol_rel, maxeval, dx=None):
    """the starts one after another through the real reference's LN_COBYLA; the callback is the objective's host twin"""
    R, A = T.more_bind(O.ref()), C.CDLL(T.EMU)
    A.nlopt_amd_objective.restype = C.c_void_p
    fptr = A.nlopt_amd_objective(O.OBJ[obj])
    out = dict(x=[], f=[], ret=[], nevals=[])
    for s in starts:
        opt = R.nlopt_create(T.LN_COBYLA, n)
        R.nlopt_set_lower_bounds(opt, T.dp(lb)); R.nlopt_set_upper_bounds(opt, T.dp(ub))
        R.nlopt_set_min_objective(opt, C.cast(fptr, C.c_void_p), None)
        R.nlopt_set_xtol_rel(opt, xtol_rel)
        if maxeval:
            R.nlopt_set_maxeval(opt, maxeval)
        if dx is not None:
            R.nlopt_set_initial_step.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
            R.nlopt_set_initial_step(opt, T.dp(dx))
        x, minf = np.array(s, dtype=np.float64), C.c_double(0)
        out["ret"].append(R.nlopt_optimize(opt, T.dp(x), C.byref(minf)))
        out["f"].append(minf.value); out["x"].append(x); out["nevals"].append(R.nlopt_get_numevals(opt))
        R.nlopt_destroy(opt)
    out["x"], out["f"] = np.array(out["x"]), np.array(out["f"])
    return out


def same(a, b):
    assert a["ret"] == b["ret"] and a["nevals"] == b["nevals"], (a["ret"], b["ret"], a["nevals"], b["nevals"])
    assert np.array_equal(a["f"], b["f"]) and np.array_equal(a["x"], b["x"]), (a["f"], b["f"])


# n = 52: the first dimension past the LDS kernel (initial simplex + iterations); n = 65: two trips of the 64 lanes over a column, n odd;
# n = 7: small n, where the LDS kernel serves too — same bits; n = 6: infinite bounds (fewer rows than 2n)
@pytest.mark.parametrize("obj,n,count,maxeval,xtol,kind", [("sphere", 52, 1, 120, 1e-6, "plain"), ("rosenbrock", 65, 1, 110, 1e-6, "plain"),
                                                           ("sphere", 7, 2, 0, 1e-6, "plain"), ("rosenbrock", 6, 1, 300, 1e-7, "halfinf")])
def test_global_memory_cobyla_kernel_on_lockstep_cpu_threads_is_the_references_search(kernels, obj, n, count, maxeval, xtol, kind):
    E, K, KL = kernels
    rng = np.random.default_rng(2000 + n)
    _, lo, hi = O.golden_x0(obj, n)
    lb, ub = np.full(n, float(lo)), np.full(n, float(hi))
    starts = rng.uniform(lo, hi, (count, n))
    if kind == "halfinf":
        ub[0] = np.inf; lb[1] = -np.inf; lb[2] = -np.inf; ub[2] = np.inf
    a = E.run(K, obj, n, starts, lb, ub, xtol_rel=xtol, maxeval=maxeval, entry=GLOBAL)
    same(a, reference(obj, n, starts, lb, ub, xtol, maxeval))
    if n == 7:
        same(a, E.run(KL, obj, n, starts, lb, ub, xtol_rel=xtol, maxeval=maxeval))


def test_global_memory_cobyla_launcher_contract_on_the_cpu(kernels):
    """the sizes the launcher serves, and the LDS kernel's limits untouched beside it"""
    E, K, KL = kernels
    K.nla_cobyla_global_work_doubles.restype = C.c_size_t
    assert [K.nla_cobyla_global_fits(n) for n in (0, 1, 51, 52, 256, 257)] == [0, 1, 1, 1, 1, 0]
    assert K.nla_cobyla_global_work_doubles(256, 320) * 8 < 1.3e9 and K.nla_cobyla_global_work_doubles(257, 1) == 0
    assert KL.nla_cobyla_fits(51) == 1 and KL.nla_cobyla_fits(52) == 0
