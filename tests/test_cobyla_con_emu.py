"""CPU twin of tests/test_gpu_cobyla_con.py: hip/cobyla_con.hip (the coroutine of hip/cobyla_ext.hip with the caller's NONLINEAR
CONSTRAINT values as rows in front of the bound rows — what nlopt_amd_optimize_batch runs for LN_COBYLA with a user's device
constraint blocks) compiled by g++ over tools/simt_emu, 64 lockstep threads per search.  The test is the host side of the coroutine
(tools/cobyla_emu_check.run_ext_con): launch, read req, evaluate the objective and every constraint block at each waiting row of EX,
write EF and the search's row of EC, launch again with resume = 1.  The oracle is the REAL reference's nlopt_optimize(LN_COBYLA) with
the same Python functions as its objective and its m-dimensional constraints: result code, evaluation count, minf, x and the whole
sequence of points each search asked for are the reference's bit for bit — no tolerance anywhere (every value the kernel is given is
the value the reference was given; the kernel's own sums are the reference's in the reference's order).

The problems (problem(name); + - x only) are the smallest shapes at which a piece can go wrong:
  tutorial   n = 2, box (-inf, inf) x [0, inf), two m = 1 cubic inequalities, objective x1: ONE bound row behind two user rows
  eq1        n = 1, one equality in a finite box: rows +h, -h
  mixed      n = 5, inequality blocks m = 3 and m = 1, one equality block m = 2: block order, column offsets, and the doubling by
             BLOCK (+h0, +h1, -h0, -h1 — by value it would be +h0, -h0, +h1, -h1)
  nobounds   n = 3, no finite bound, one inequality: m = mc
  cuts       n = 8, one block of 70 linear cuts: m + 2 > 64 lanes and > n + 1 (the lane-strided loops wrap, cw_vlen = m + 2)
  clash      n = 2, x0 <= -1 and x0 >= 1: no feasible point
  nearly     n = 2, a constraint that is violated by 1e-4 .. 2e-3 everywhere: feasible within a tolerance of 1e-2 only"""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

import _oracle as O
import test_cobyla_differential as T
from test_cobyla_ext_emu import FORCED_STOP, MAXEVAL_REACHED, MINF_MAX_REACHED, XTOL_REACHED, same, stays_finished

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")

pytestmark = pytest.mark.skipif(not shutil.which("g++") or not O.have_ref() or not os.path.exists(T.EMU), reason="no g++ / oracle/_ref / emulated library here")


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import cobyla_emu_check as E
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return E


@pytest.fixture(scope="module")
def kernel():
    E = _tool()
    return E, C.CDLL(E.build_con())


# ---- the problems: every function a sequential sum of products, left to right ----------------------------------------------------------
def _cubic(a, b):
    def g(x):
        t = a * x[0] + b
        return [t * t * t - x[1]]
    return g


def _wsq(centre, weight):
    def f(x):
        s = 0.0
        for i in range(len(x)):
            d = x[i] - centre[i]
            s += weight[i] * d * d
        return s
    return f


def _mixed_g3(x):
    return [x[j] * x[j + 1] - 0.5 * (j + 1) for j in range(3)]


def _ball(r2):
    def g(x):
        s = 0.0
        for v in x:
            s += v * v
        return [s - r2]
    return g


def _mixed_h2(x):
    return [x[0] + x[1] + x[2] - 1.0, x[3] * x[4] - 0.25]


CUTS_A = [[((7 * k + 3 * j) % 11 - 5) * 0.125 for j in range(8)] for k in range(70)]
CUTS_B = [1.0 + (k % 7) * 0.25 for k in range(70)]


def _cuts(x):
    out = []
    for k in range(70):
        s = 0.0
        for j in range(8):
            s += CUTS_A[k][j] * x[j]
        out.append(s - CUTS_B[k])
    return out


def problem(name, tol=None):
    """n, lb, ub, f, the inequality blocks [(m, fn, tolerances)], the equality blocks the same"""
    if name == "tutorial":
        p = dict(n=2, lb=[-INF, 0.0], ub=[INF, INF], f=lambda x: x[1], ineq=[(1, _cubic(2.0, 0.0), [1e-8]), (1, _cubic(-1.0, 1.0), [1e-8])], eq=[])
    elif name == "eq1":
        p = dict(n=1, lb=[0.0], ub=[3.0], f=_wsq([0.5], [1.0]), ineq=[], eq=[(1, lambda x: [x[0] * x[0] - 2.0], [1e-8])])
    elif name == "mixed":
        p = dict(n=5, lb=[-2.0] * 5, ub=[2.0] * 5, f=_wsq([1.0, -0.5, 0.75, 1.5, -1.0], [1.0, 2.0, 0.5, 1.5, 1.0]),
                 ineq=[(3, _mixed_g3, [1e-8, 0.0, 1e-6]), (1, _ball(4.0), [1e-8])], eq=[(2, _mixed_h2, [1e-8, 1e-6])])
    elif name == "nobounds":
        p = dict(n=3, lb=[-INF] * 3, ub=[INF] * 3, f=_wsq([2.0, 1.0, -1.0], [1.0, 1.0, 1.0]), ineq=[(1, _ball(1.0), [0.0])], eq=[])
    elif name == "cuts":
        p = dict(n=8, lb=[-3.0] * 8, ub=[3.0] * 8, f=_wsq([2.0, -2.0, 1.5, -1.5, 2.5, -2.5, 1.0, -1.0], [1.0] * 8), ineq=[(70, _cuts, [1e-8] * 70)], eq=[])
    elif name == "clash":
        p = dict(n=2, lb=[-3.0, -3.0], ub=[3.0, 3.0], f=_wsq([0.5, 0.5], [1.0, 1.0]),
                 ineq=[(2, lambda x: [x[0] + 1.0, 1.0 - x[0]], [0.0, 0.0])], eq=[])
    elif name == "nearly":
        t = 1e-2 if tol is None else tol
        p = dict(n=2, lb=[-3.0, -3.0], ub=[3.0, 3.0], f=_wsq([1.0, 1.0], [1.0, 1.0]),
                 ineq=[(1, lambda x: [1e-4 * (1.0 + (x[0] - 1.0) * (x[0] - 1.0))], [t])], eq=[])
    else:
        raise KeyError(name)
    p["lb"], p["ub"] = np.array(p["lb"]), np.array(p["ub"])
    p["mi"] = sum(m for m, _, _ in p["ineq"])
    p["eq_sizes"] = [m for m, _, _ in p["eq"]]
    p["tol"] = np.array([t for _, _, ts in p["ineq"] + p["eq"] for t in ts], dtype=np.float64)
    return p


def evaluator(p, sign=1.0):
    """what run_ext_con wants: x -> (f as the search is to see it, the inequality values, the equality values)"""
    def ev(x):
        x = [float(v) for v in x]
        return sign * p["f"](x), [v for _, fn, _ in p["ineq"] for v in fn(x)], [v for _, fn, _ in p["eq"] for v in fn(x)]
    return ev


def reference(p, starts, xtol_rel=1e-6, maxeval=0, dx=None, maximise=False, stopval=None, force_at=None):
    """the starts one after another through the real reference's LN_COBYLA: the objective records every point it is given and
    (force_at = k) calls nlopt_force_stop inside its k-th call; every block is an m-dimensional constraint"""
    R = T.more_bind(O.ref())
    R.nlopt_force_stop.argtypes = [C.c_void_p]
    n = p["n"]
    out = dict(x=[], f=[], ret=[], nevals=[], asked=[])
    for s in starts:
        opt = R.nlopt_create(T.LN_COBYLA, n)
        pts, keep = [], []

        def cb(nn, x, g, d):
            pts.append(np.array(x[:nn], dtype=np.float64))
            if force_at is not None and len(pts) == force_at:
                R.nlopt_force_stop(opt)
            return p["f"]([float(v) for v in pts[-1]])
        fcb = O.FUNC(cb)
        R.nlopt_set_lower_bounds(opt, T.dp(p["lb"])); R.nlopt_set_upper_bounds(opt, T.dp(p["ub"]))
        (R.nlopt_set_max_objective if maximise else R.nlopt_set_min_objective)(opt, C.cast(fcb, C.c_void_p), None)
        for blocks, add in ((p["ineq"], R.nlopt_add_inequality_mconstraint), (p["eq"], R.nlopt_add_equality_mconstraint)):
            for m, fn, tol in blocks:
                def mf(mm, res, nn, x, g, d, fn=fn):
                    for i, v in enumerate(fn([float(x[j]) for j in range(nn)])):
                        res[i] = v
                mcb = T.MFUNC(mf)
                keep.append(mcb)
                assert add(opt, m, C.cast(mcb, C.c_void_p), None, T.dp(np.array(tol, dtype=np.float64))) > 0
        R.nlopt_set_xtol_rel(opt, xtol_rel)
        if maxeval:
            R.nlopt_set_maxeval(opt, maxeval)
        if stopval is not None:
            R.nlopt_set_stopval(opt, stopval)
        if dx is not None:
            R.nlopt_set_initial_step(opt, T.dp(np.asarray(dx, dtype=np.float64)))
        x, minf = np.array(s, dtype=np.float64), C.c_double(0)
        out["ret"].append(R.nlopt_optimize(opt, T.dp(x), C.byref(minf)))
        out["f"].append(minf.value); out["x"].append(x); out["nevals"].append(R.nlopt_get_numevals(opt)); out["asked"].append(pts)
        R.nlopt_destroy(opt)
    out["x"], out["f"] = np.array(out["x"]), np.array(out["f"])
    return out


def kernel_run(E, K, p, starts, sign=1.0, mem=None, **kw):
    return E.run_ext_con(K, p["n"], np.asarray(starts, dtype=np.float64), p["lb"], p["ub"], evaluator(p, sign), p["mi"], p["eq_sizes"], tol=p["tol"],
                         mem=mem, **kw)


# the starts of the five shapes: (problem, starts, xtol_rel, maxeval).  tutorial: the second start violates the first cubic by ~500,
# far more than its initial step (1 .. 4): the penalty parameter rises and SHRINK rescales it
SHAPES = {
    "tutorial": ([[1.234, 5.678], [4.0, 0.5]], 1e-6, 400),
    "eq1": ([[2.5], [0.25]], 1e-8, 200),
    "mixed": ([[0.1, 0.2, -0.3, 0.4, 0.5], [-1.5, 1.5, 1.0, -1.0, 1.9]], 1e-6, 400),
    "nobounds": ([[3.0, -2.0, 0.5], [0.1, 0.1, 0.1]], 1e-7, 300),
    "cuts": ([[0.0] * 8, [2.5, -2.5, 2.0, -2.0, 2.9, -2.9, 1.0, -1.0]], 1e-5, 400),
}
SEVEN = [[0.1, 0.2, -0.3, 0.4, 0.5], [-1.5, 1.5, 1.0, -1.0, 1.9], [1.0, 1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0], [1.9, -1.9, 1.9, -1.9, 1.9],
         [-0.4, 0.9, 0.5, 0.5, 0.5], [0.3, 0.3, 0.4, 1.0, 0.25]]


@pytest.fixture(scope="module")
def refs():
    """the reference's runs, once"""
    r = {name: reference(problem(name), s, xtol, me) for name, (s, xtol, me) in SHAPES.items()}
    r["seven"] = reference(problem("mixed"), SEVEN, 1e-3, 120)
    return r


def test_the_inputs_make_the_reference_do_what_the_cases_are_about(refs):
    """checked against the reference alone: every search of the five shapes reaches the linear programme with user rows (n + 2
    evaluations at least), the file sees XTOL_REACHED, MAXEVAL_REACHED and MINF_MAX_REACHED, one start is infeasible by more than
    its initial step, and the seven searches of the batch end at different launches"""
    for name in SHAPES:
        assert min(refs[name]["nevals"]) >= problem(name)["n"] + 2, (name, refs[name]["nevals"])
    rets = [c for name in SHAPES for c in refs[name]["ret"]]
    assert XTOL_REACHED in rets, rets
    p = problem("tutorial")
    viol = max(p["ineq"][0][1]([4.0, 0.5])[0], p["ineq"][1][1]([4.0, 0.5])[0])
    assert viol > 4.0 * 10                                            # (the default initial step of that start: 4.0 and 0.375)
    assert len(set(refs["seven"]["nevals"])) >= 4, refs["seven"]["nevals"]
    assert MAXEVAL_REACHED in refs["seven"]["ret"] and XTOL_REACHED in refs["seven"]["ret"], refs["seven"]["ret"]


@pytest.mark.parametrize("name", list(SHAPES))
def test_constrained_coroutine_kernel_asks_for_the_references_points_and_returns_its_result(kernel, refs, name):
    E, K = kernel
    s, xtol, me = SHAPES[name]
    a = kernel_run(E, K, problem(name), s, xtol_rel=xtol, maxeval=me)
    same(a, refs[name])
    stays_finished(a)


def test_infeasible_starts_and_contradictory_constraints(kernel):
    """x0 <= -1 and x0 >= 1: the greatest violation never falls below 1; the search ends where the reference's ends, by its code"""
    E, K = kernel
    p = problem("clash")
    s = [[2.0, 2.0], [0.0, -1.0], [-2.5, 0.5]]
    r = reference(p, s, 1e-4, 300)
    a = kernel_run(E, K, p, s, xtol_rel=1e-4, maxeval=300)
    same(a, r)
    for x in a["x"]:
        assert max(p["ineq"][0][1]([float(v) for v in x])) >= 1.0


def test_stop_value_counts_a_point_that_is_feasible_within_the_tolerance_only(kernel):
    """f < stopval = 0.5 first at a point whose constraint value is ~2e-4: with tolerance 1e-2 the search stops there
    (MINF_MAX_REACHED, not at its first evaluation); with tolerance 0 no point is ever feasible and it must not"""
    E, K = kernel
    s = [[-1.0, -1.0], [-2.0, 0.0]]
    p = problem("nearly")
    r = reference(p, s, 1e-4, 200, stopval=0.5)
    assert r["ret"] == [MINF_MAX_REACHED] * 2 and min(r["nevals"]) > 1, (r["ret"], r["nevals"])
    same(kernel_run(E, K, p, s, xtol_rel=1e-4, maxeval=200, minf_max=0.5), r)
    p0 = problem("nearly", tol=0.0)
    r0 = reference(p0, s, 1e-4, 200, stopval=0.5)
    assert MINF_MAX_REACHED not in r0["ret"] and all(n0 > n1 for n0, n1 in zip(r0["nevals"], r["nevals"])), (r0["ret"], r0["nevals"])
    same(kernel_run(E, K, p0, s, xtol_rel=1e-4, maxeval=200, minf_max=0.5), r0)


@pytest.mark.parametrize("maxeval", [3, 7, 25])
def test_maxeval_inside_the_initial_simplex_at_its_end_and_behind_it(kernel, maxeval):
    E, K = kernel
    p = problem("mixed")
    s = SEVEN[:2]
    a = kernel_run(E, K, p, s, maxeval=maxeval)
    same(a, reference(p, s, maxeval=maxeval))
    assert a["ret"] == [MAXEVAL_REACHED] * 2 and a["nevals"] == [maxeval] * 2


@pytest.mark.parametrize("k", [4, 9])
def test_forced_stop_from_the_kth_relaunch_on(kernel, k):
    """ext.forced = 1 from relaunch k on (k = 4: inside the initial simplex of n = 5, k = 9: behind it).  Relaunch k delivers the k-th
    values; the search TAKES them and meets the flag in front of its next evaluation: k evaluations, the pole behind the k-th.  The
    reference drops the values of the call that forced the stop (cobyla.c:104, 582-589), and a constrained run has no memoized best
    point to hide that, so the oracle is the reference whose objective forces the stop inside call k + 1: the same pole, one
    evaluation (and one asked point) more"""
    E, K = kernel
    p = problem("mixed")
    s = SEVEN[:3]
    a = kernel_run(E, K, p, s, forced_from=k)
    r = reference(p, s, force_at=k + 1)
    assert a["ret"] == r["ret"] == [FORCED_STOP] * 3 and a["nevals"] == [k] * 3 and r["nevals"] == [k + 1] * 3 and a["launches"] == k + 1
    assert np.array_equal(a["f"], r["f"]) and np.array_equal(a["x"], r["x"])
    for pa, pr in zip(a["asked"], r["asked"]):
        assert len(pa) == k and all(np.array_equal(u, v) for u, v in zip(pa, pr[:k]))


def test_seven_searches_of_one_batch_that_end_at_different_launches(kernel, refs):
    """xtol_rel = 1e-3, 120 evaluations at the most: every search restores ITS saved state (the emulation has one LDS block for all),
    and a finished search's row of EC is never written again (run_ext_con leaves it as it was) while the others go on"""
    E, K = kernel
    a = kernel_run(E, K, problem("mixed"), SEVEN, xtol_rel=1e-3, maxeval=120)
    same(a, refs["seven"])
    stays_finished(a)
    assert sorted(a["finished_at"]) == sorted(refs["seven"]["nevals"]) and a["launches"] == max(refs["seven"]["nevals"]) + 1


def test_maximisation_changes_the_sign_of_f_only(kernel):
    """the tutorial's shape with objective -x1 MAXIMISED: the caller delivers -f = x1, the constraint values as they are"""
    E, K = kernel
    p = problem("tutorial")
    p["f"] = lambda x: -x[1]
    s, xtol, me = SHAPES["tutorial"]
    r = reference(p, s, xtol, me, maximise=True)
    a = kernel_run(E, K, p, s, sign=-1.0, xtol_rel=xtol, maxeval=me)
    same(a, r, sign=-1.0)


def test_given_initial_step_with_unequal_entries(kernel):
    """the rescaled search: user rows are taken at the unscaled point, bound rows at the scaled one"""
    E, K = kernel
    p = problem("mixed")
    dx = [0.3, 0.2, 0.45, 0.1, 0.25]
    a = kernel_run(E, K, p, SEVEN[:2], xtol_rel=1e-4, maxeval=150, dx=dx)
    same(a, reference(p, SEVEN[:2], 1e-4, 150, dx=dx))


def test_row_map_and_sizes():
    E = _tool()
    assert list(E.con_rowmap(2, [2, 1])) == [-1, -2, 2, 3, -3, -4, 4, -5]
    assert list(E.con_rowmap(0, [1])) == [0, -1] and list(E.con_rowmap(3, [])) == [-1, -2, -3]


def test_constrained_coroutine_launcher_contract_on_the_cpu(kernel):
    E, K = kernel
    E.con_bind(K)
    KE = E.ext_bind(C.CDLL(E.build_ext()))
    assert [K.nla_cobyla_con_serves(n, mc) for n, mc in ((0, 1), (1, 0), (1, 1), (8, 70), (256, 2), (256, 175), (256, 176), (257, 1), (8, 1200), (8, 100000))] \
        == [0, 0, 1, 1, 1, 1, 0, 0, 1, 0]
    assert K.nla_cobyla_con_work_doubles(256, 176, 1) == 0 and K.nla_cobyla_con_save_bytes(256, 176) == 0
    # more than the unconstrained coroutine's, by the user rows; the existing sizes are what they were
    assert K.nla_cobyla_con_work_doubles(5, 8, 3) > KE.nla_cobyla_ext_work_doubles(5, 3) and K.nla_cobyla_con_save_bytes(5, 8) > KE.nla_cobyla_save_bytes(5)
    assert K.nla_cobyla_con_save_bytes(256, 175) <= 64 * 1024 + 256
    # refusals: nothing is launched — X, req and the result records stay as they were
    n, ld, count, mi, me = 4, 4, 2, 2, 1
    X0 = np.random.default_rng(4600).uniform(-1, 1, (count, ld))
    lb, ub = np.full(n, -2.0), np.full(n, 2.0)

    def call(n=n, ld=ld, count=count, mi=mi, me=me, ldc=3, drop=None):
        rows = max(count, 1)
        X, req, out = X0.copy(), np.full((rows, 2), 7, dtype=np.int32), np.full(rows * 3, -1.0)
        nn, mm = min(max(n, 1), 256), 4
        bufs = dict(req=req, EX=np.zeros((rows, max(ld, 1))), EF=np.zeros(rows), save=np.zeros(max(8, K.nla_cobyla_con_save_bytes(nn, mm) * rows // 8)),
                    work=np.zeros(max(8, K.nla_cobyla_con_work_doubles(nn, mm, rows))), EC=np.zeros((rows, 8)), tol=np.zeros(8),
                    map=E.con_rowmap(max(mi, 0), [max(me, 0)] if me > 0 else []))
        ptr = lambda k: None if drop == k else bufs[k].ctypes.data
        e = E.Ext(ptr("req"), ptr("EX"), np.zeros(8).ctypes.data, ptr("EF"), ptr("save"), 0, 0, 0, 0)
        P = E.Params(-np.inf, 0.0, 0.0, 1e-6, 50, 0, 1.0, None, None, None)
        rc = K.nla_k_cobyla_batch_ext_con(n, ld, count, lb.ctypes.data, ub.ctypes.data, None, X.ctypes.data, ptr("work"), C.byref(P), out.ctypes.data,
                                          None if drop == "ext" else C.byref(e), mi, me, ldc, ptr("EC"), ptr("tol"), ptr("map"), None)
        return rc, np.array_equal(X, X0) and np.all(req == 7) and np.all(out == -1.0)
    for kw in (dict(n=0), dict(n=257, ld=258), dict(ld=3), dict(mi=0, me=0), dict(mi=-1), dict(me=-1), dict(ldc=2), dict(drop="work"), dict(drop="ext"),
               dict(drop="req"), dict(drop="EX"), dict(drop="EF"), dict(drop="save"), dict(drop="EC"), dict(drop="tol"), dict(drop="map")):
        rc, untouched = call(**kw)
        assert rc != 0 and untouched, kw
    assert call(count=0) == (0, True) and call(count=-1) == (0, True)
    rc, untouched = call()
    assert rc == 0 and not untouched
