"""CPU twin of tests/test_gpu_tnewton.py's host-callback part: hip/tnewton_kernels.hip (batched NLOPT_LD_TNEWTON, _RESTART, _PRECOND,
_PRECOND_RESTART; one workgroup per search) compiled by g++ over tools/simt_emu with workgroups of 64 host threads and run AS A COROUTINE
in exact-order mode (tools/tnewton_emu_check.run_ext: launch, read req, evaluate, write EF and EG, launch again with resume = 1).  The
oracle is the REAL reference's nlopt_optimize(ids 15 .. 18) on the same Python objective, its callback recording every point: the result
code, the evaluation count, the whole sequence of points asked for (the CG probes included), the values delivered, minf and x — the best
point SEEN, not the last iterate (memoize_func) — are the reference's bit for bit, no tolerance anywhere.
PROBLEMS is the list the GPU test imports.  The (code, count) figures are asserted on the reference's run first."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

import _oracle as O
from test_lbfgs_emu import BOXES, box, problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = (15, 16, 17, 18)
FORCED_STOP, SUCCESS, MAXTIME_REACHED = -5, 1, 6

pytestmark = pytest.mark.skipif(not shutil.which("g++") or not O.have_ref(), reason="no g++ / oracle/_ref here")


def tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import tnewton_emu_check as E
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return E


E = tool()
rosen, wquad4, rastr, parabola = E.rosen, E.wquad4, E.rastr, E.parabola


@pytest.fixture(scope="module")
def kernel():
    return C.CDLL(E.build())


def _p(name, n, f, x0, lb, ub, expect=None, **kw):
    """expect: per id (result code, evaluation count), or None; kw: the settings of tools/tnewton_emu_check.reference"""
    return dict(name=name, n=n, f=f, x0=np.array(x0, dtype=np.float64), lb=np.array(lb, dtype=np.float64), ub=np.array(ub, dtype=np.float64), expect=expect, kw=kw)


def _full(n, lo, hi):
    return np.full(n, float(lo)), np.full(n, float(hi))


_G65 = np.random.default_rng(65)
W65_FIRST, W65_SECOND = _G65.uniform(-1.5, 1.5, 65), _G65.uniform(-1.5, 1.5, 65)
_R = np.random.default_rng(1518)
ROSEN2 = dict(n=2, f=rosen, x0=[-1.2, 1.0], lb=[-np.inf, -np.inf], ub=[np.inf, np.inf])
ROSEN10_BOX = dict(n=10, f=rosen, x0=np.full(10, -1.0), lb=np.full(10, -1.5), ub=np.full(10, 0.5))

PROBLEMS = [
    _p("rosen2", **ROSEN2, expect=[(1, 182), (1, 89), (1, 234), (1, 74)]),
    _p("rosen2_ftol", **ROSEN2, expect=[(1, 182), (1, 89), (1, 234), (1, 74)], ftol_rel=1e-3),          # (never fires: the same runs)
    _p("rosen2_stopval", **ROSEN2, expect=[(2, 138), (2, 45), (2, 194), (2, 34)], minf_max=1.0),
    _p("rosen2_xtol", **ROSEN2, expect=[(4, 11), (4, 84), (4, 12), (4, 71)], xtol_rel=1e-2),
    _p("rosen2_maxeval1", **ROSEN2, expect=[(5, 1)] * 4, maxeval=1),
    _p("rosen10_box", **ROSEN10_BOX, expect=[(1, 83), (1, 59), (1, 71), (1, 47)]),
    _p("rastr5", 5, rastr, [2.3, -1.7, 0.6, 3.4, -4.2], *_full(5, -5.12, 5.12), expect=[(1, 22), (1, 20), (1, 20), (1, 21)]),
    _p("wquad65", 65, wquad4, W65_FIRST, *_full(65, -2, 2), expect=[(1, 23), (1, 24), (1, 13), (1, 13)]),
    _p("wquad65_maxeval7", 65, wquad4, W65_SECOND, *_full(65, -2, 2), expect=[(5, 10), (5, 7), (5, 7), (5, 8)], maxeval=7),   # id 15: a CG loop overruns
    _p("rosen6_fixed", 6, rosen, [-1.2, 1, 0.3, 1, -1.2, 1], [-2, -2, 0.3, -2, -2, -2], [2, 2, 0.3, 2, 2, 2], expect=[(1, 34), (1, 37), (1, 39), (1, 32)]),
    # the strided loops at a workgroup's edge in the emulator (64 threads)
    _p("n1", 1, parabola, [1.5], *_full(1, -2, 2)),
    _p("wquad63", 63, wquad4, _R.uniform(-1.5, 1.5, 63), *_full(63, -2, 2), maxeval=60),
    _p("wquad64", 64, wquad4, _R.uniform(-1.5, 1.5, 64), *_full(64, -2, 2), maxeval=60),
    _p("wquad65_maxeval60", 65, wquad4, _R.uniform(-1.5, 1.5, 65), *_full(65, -2, 2), maxeval=60),
] + [
    # one-sided and open boxes, a finite side pulled inside the region of the start
    _p("rosen10_" + kind, 10, rosen, problem("rosenbrock", 10, kind, count=1)[0][0], *box("rosenbrock", 10, kind), maxeval=150)
    for kind in BOXES if kind != "closed"
] + [
    _p("xtol_abs", **ROSEN2, xtol_abs=[1e-2, 2e-2], maxeval=400),
    _p("x_weights", **ROSEN2, xtol_rel=1e-2, x_weights=[1.0, 100.0], maxeval=400),
    _p("ring_wraps", **ROSEN10_BOX, vector_storage=3),                    # PRECOND ids: mf = 3 < the iterations, the ring of columns wraps
    _p("forced_at_probe", **ROSEN2, expect=[(FORCED_STOP, None)] * 4, force_at=2),       # evaluation 2 is the first CG probe (ids 15, 17)
    _p("forced9", **ROSEN10_BOX, expect=[(FORCED_STOP, None)] * 4, force_at=9),
    _p("timeout_first", **ROSEN2, expect=[(MAXTIME_REACHED, 1)] * 4, maxtime=1e-9),     # pnet.c:303: the clock has run out behind evaluation 1
]
CASES = [(p, alg) for p in PROBLEMS for alg in IDS]
CASE_IDS = ["%s-%d" % (p["name"], alg) for p, alg in CASES]

_REF = {}


def reference_of(p, alg, R=None):
    """the real reference's run (R: another library with the NLopt C API), computed once per problem and id"""
    key = (p["name"], alg, id(R) if R is not None else None)
    if key not in _REF:
        _REF[key] = E.reference(alg, p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], R=R, **p["kw"])
    return _REF[key]


def kernel_kw(kw):
    """reference settings -> run_ext's: force_at = k is ext.forced from relaunch k on, a clock that has run out is ext.timeout from the start"""
    kw = dict(kw)
    if "force_at" in kw:
        kw["forced_from"] = kw.pop("force_at")
    if "maxtime" in kw:
        kw.pop("maxtime"); kw["timeout_from"] = 0
    return kw


def check_expectations(p, alg, r):
    if p["expect"] is not None:
        ret, nevals = p["expect"][alg - 15]
        assert r["ret"] == [ret], (p["name"], alg, r["ret"], r["nevals"])
        if nevals is not None:
            assert r["nevals"] == [nevals], (p["name"], alg, r["nevals"])
    else:
        assert r["nevals"][0] > 2, (p["name"], alg, r["nevals"])


def best_seen(pts, fs, lb, ub):
    """memoize_func (optimize.c:460-482) replayed on a recorded run"""
    best, bx = np.finfo(np.float64).max, None
    for x, f in zip(pts, fs):
        if np.all(x >= lb) and np.all(x <= ub) and f < best:
            best, bx = f, x
    return best, bx


@pytest.mark.parametrize("p,alg", CASES, ids=CASE_IDS)
def test_coroutine_kernel_asks_for_the_references_points_and_returns_its_result(kernel, p, alg):
    r = reference_of(p, alg)
    check_expectations(p, alg, r)
    a = E.run_ext(kernel, alg, p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], **kernel_kw(p["kw"]))
    E.same(a, r)
    assert a["finished_at"][0] is not None and all(s[0] == 2 for s in a["seen"][a["finished_at"][0]:])


def test_the_table_reaches_a_returned_point_that_is_not_the_last_one_evaluated():
    """so that the best-seen rule is exercised: read from the REFERENCE's trace"""
    hit = 0
    for name in ("rastr5", "rosen10_box", "wquad65"):
        p = next(q for q in PROBLEMS if q["name"] == name)
        for alg in IDS:
            r = reference_of(p, alg)
            f, x = best_seen(r["asked"][0], r["fseq"][0], p["lb"], p["ub"])
            assert E.bits(f) == E.bits(r["f"][0]) and np.array_equal(E.bits(x), E.bits(r["x"][0]))
            hit += not np.array_equal(r["x"][0], r["asked"][0][-1])
    assert hit > 0


@pytest.mark.parametrize("alg", IDS)
def test_a_clock_that_runs_out_at_a_probe_ends_the_search_behind_that_cg_loop(kernel, alg):
    """the reference reads the clock behind the first evaluation, behind PYFUT1 and behind the direction (pnet.c:303,315,507), never inside
    the CG loop; its clock cannot be told to run out at a given evaluation, so this is the kernel alone: ext.timeout from relaunch 2 on
    (evaluation 2: a probe on ids 15 / 17, the first line-search point on 16 / 18) — the points asked for are a proper prefix of the
    untimed run's, the code is MAXTIME_REACHED and the result is the best point of that prefix"""
    p = next(q for q in PROBLEMS if q["name"] == "rosen10_box")
    r = reference_of(p, alg)
    a = E.run_ext(kernel, alg, p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], timeout_from=2)
    k = a["nevals"][0]
    assert a["ret"] == [MAXTIME_REACHED] and 2 <= k < r["nevals"][0] and len(a["asked"][0]) == k
    assert all(np.array_equal(E.bits(u), E.bits(v)) for u, v in zip(a["asked"][0], r["asked"][0][:k]))
    f, x = best_seen(r["asked"][0][:k], r["fseq"][0][:k], p["lb"], p["ub"])
    assert E.bits(a["f"][0]) == E.bits(f) and np.array_equal(E.bits(a["x"][0]), E.bits(x))


@pytest.mark.parametrize("alg", IDS)
def test_searches_of_one_batch_equal_their_lone_runs(kernel, alg):
    """three searches with different objectives in one launch sequence: each is its lone run, and the reference's"""
    n, lb, ub = 10, np.full(10, -1.5), np.full(10, 1.5)
    starts = np.random.default_rng(1600).uniform(-1.4, 1.4, (3, n))
    fs = [rosen, wquad4, rastr]
    a = E.run_ext(kernel, alg, n, starts, lb, ub, fs, maxeval=80)
    r = E.reference(alg, n, starts, lb, ub, fs, maxeval=80)
    E.same(a, r)
    assert len(set(a["finished_at"])) > 1


@pytest.mark.parametrize("obj,n", [("sphere", 5), ("rosenbrock", 10)])
@pytest.mark.parametrize("alg", IDS)
def test_whole_search_on_a_compiled_in_objective_is_the_references(kernel, alg, obj, n):
    """no libm in these two: the device objective in exact-order mode gives the callback's bits, so the f trace (probes included), the
    count, the code, minf and x are the reference's"""
    x0, lo, hi = O.golden_x0(obj, n)
    r = O.run_ref(alg, obj, n, 0, 0, x0=np.array(x0, dtype=np.float64))
    a = E.run(kernel, alg, obj, n, [x0], np.full(n, float(lo)), np.full(n, float(hi)), exact=1)
    assert a["ret"][0] == r["ret"] and a["nevals"][0] == r["nevals"] == len(r["fseq"])
    assert np.array_equal(E.bits(a["ftrace"][0][: r["nevals"]]), E.bits(r["fseq"])) and np.isnan(a["ftrace"][0][r["nevals"]:]).all()
    assert E.bits(a["f"][0]) == E.bits(r["minf"]) and np.array_equal(E.bits(a["x"][0]), E.bits(r["x"]))


def test_launcher_contract_on_the_cpu(kernel):
    E.bind(kernel)
    assert kernel.nla_tnewton_work_doubles(10, 3, 2) == 2 * (10 * 10 + 6) and kernel.nla_tnewton_hist_doubles(10, 3, 2) == 2 * 2 * 3 * 10
    assert kernel.nla_tnewton_hist_doubles(10, 0, 5) == 0 and kernel.nla_tnewton_save_bytes() > 0
    n, ld = 4, 4
    X0 = np.random.default_rng(1700).uniform(-1, 1, (1, ld))
    lb, ub = np.full(n, -2.0), np.full(n, 2.0)

    def call(n=n, ld=ld, mf=0, mos=0, count=1, hist=False, work=True):
        X, out = X0.copy(), np.full(3, -1.0)
        w, iw, h = np.zeros(200), np.zeros(16, dtype=np.int32), np.zeros(200)
        P = E.Params(-np.inf, 0.0, 0.0, 0.0, 0.0, 5, 1, 1.0, None, None, None, None, 0, None)
        rc = kernel.nla_k_tnewton_batch(O.OBJ["sphere"], n, ld, mf, mos, count, lb.ctypes.data, ub.ctypes.data, X.ctypes.data, w.ctypes.data if work else None,
                                        iw.ctypes.data, h.ctypes.data if hist else None, C.byref(P), out.ctypes.data, None, None)
        return rc, np.array_equal(X, X0) and np.all(out == -1.0)
    for kw in (dict(n=0), dict(ld=3), dict(mos=4), dict(mos=-1), dict(mos=2, mf=0, hist=True), dict(mos=2, mf=3), dict(mos=0, mf=3), dict(work=False)):
        rc, untouched = call(**kw)
        assert rc != 0 and untouched, kw
    assert call(count=0) == (0, True)
    rc, untouched = call()
    assert rc == 0 and not untouched
    rc, untouched = call(mos=3, mf=3, hist=True)
    assert rc == 0 and not untouched
