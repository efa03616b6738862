"""CPU twin of tests/test_gpu_nldrmd.py's kernel-level part: hip/nldrmd_kernels.hip (batched NLOPT_LN_NELDERMEAD, one wavefront per search)
compiled by g++ over tools/simt_emu, 64 lockstep threads per search, and run AS A COROUTINE (tools/nldrmd_emu_check.run_ext: launch, read
req, evaluate, write EF, launch again with resume = 1).  The oracle is the REAL reference's nlopt_optimize(NLOPT_LN_NELDERMEAD) on the same
Python objective, its callback recording every point: the result code, the evaluation count, minf, x AND the whole sequence of points
each search asked for are the reference's bit for bit — no tolerance anywhere (both are handed identical values, the objectives are
sequential left-to-right sums).  PROBLEMS is the list the GPU test imports: the smallest shapes at which a piece can go wrong.
The emulation runs one workgroup at a time in ONE static LDS block, so a search that came back with anything but its own saved state
would continue from another search's vectors.  What it cannot see is the device's memory model: the GPU twin."""
import ctypes as C
import math
import os
import shutil
import sys

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAILURE, FORCED_STOP = -1, -5
SUCCESS, MINF_MAX_REACHED, FTOL_REACHED, XTOL_REACHED, MAXEVAL_REACHED, MAXTIME_REACHED = 1, 2, 3, 4, 5, 6

pytestmark = pytest.mark.skipif(not shutil.which("g++") or not O.have_ref(), reason="no g++ / oracle/_ref here")


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import nldrmd_emu_check as E
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return E


@pytest.fixture(scope="module")
def kernel():
    E = _tool()
    return E, C.CDLL(E.build())


# ---- objectives: sequential left-to-right sums in Python floats (IEEE doubles, no contraction) -------------------------------------------
def rosenbrock(x):
    s = 0.0
    for i in range(len(x) - 1):
        a, b = x[i + 1] - x[i] * x[i], 1.0 - x[i]
        s += 100.0 * a * a + b * b
    return s


def rosenbrock_plus_one(x):
    """a minimum value of 1: a relative f-tolerance can be met before the simplex has collapsed"""
    return rosenbrock(x) + 1.0


def parabola(x):
    return (x[0] - 0.3) * (x[0] - 0.3)


def wquad(x):
    """the minimiser (2, -2, 2, -2, 2) lies outside [-1, 1]^5: the search ends on a face, reflections pinned to bounds"""
    s = 0.0
    for i in range(len(x)):
        d = x[i] - (2.0 if i % 2 == 0 else -2.0)
        s += (i + 1.0) * d * d
    return s


def ridge(x):
    s = 0.0
    for i in range(len(x)):
        d = x[i] - 0.1 * (i % 7)
        s += (1.0 + (i % 3)) * d * d
    return s


def flat(x):
    return 1.0


def steps(x):
    return math.floor(4.0 * x[0]) + math.floor(4.0 * x[1])


def _box(n, lo, hi):
    return np.full(n, float(lo)), np.full(n, float(hi))


def _p(name, n, f, x0, lb, ub, expect=None, nevals=None, **kw):
    return dict(name=name, n=n, f=f, x0=np.array(x0, dtype=np.float64), lb=lb, ub=ub, expect=expect, nevals=nevals, kw=kw)


_R = np.random.default_rng(2800)
ROSEN_START = [-1.2, 1.0]
UNB2 = (np.full(2, -np.inf), np.full(2, np.inf))
PROBLEMS = [
    # n = 1: two points, pred(high) is low, ninv = 1
    _p("n1", 1, parabola, [1.5], *_box(1, -2, 2), xtol_rel=1e-8, maxeval=200),
    # n = 2 Rosenbrock from (-1.2, 1) with a step of 2: reflection, expansion, both contractions and a shrink
    # (test_rosenbrock_takes_every_branch; with the steps 0.05 .. 1.5 tried, the reference's run never shrinks)
    _p("rosen2", 2, rosenbrock, ROSEN_START, *UNB2, dx=[2.0, 2.0], xtol_rel=1e-10, maxeval=400),
    # n = 5: the minimiser on a face of the box
    _p("face5", 5, wquad, [0.3, -0.2, 0.1, 0.4, -0.5], *_box(5, -1, 1), xtol_rel=1e-8, maxeval=500),
    # n + 1 points and n coordinates straddle the 64 lanes, the strided loops wrap
    _p("n63", 63, ridge, _R.uniform(-1.5, 1.5, 63), *_box(63, -2, 2), xtol_rel=1e-6, maxeval=400),
    _p("n64", 64, ridge, _R.uniform(-1.5, 1.5, 64), *_box(64, -2, 2), xtol_rel=1e-6, maxeval=400),
    _p("n65", 65, ridge, _R.uniform(-1.5, 1.5, 65), *_box(65, -2, 2), xtol_rel=1e-6, maxeval=400),
    # every comparison is a tie: the index order decides; ends through reflectpt
    _p("flat", 3, flat, [1.0, 2.0, 3.0], *_box(3, -5, 5), expect=XTOL_REACHED, maxeval=2000),
    # partial ties
    _p("steps", 2, steps, [0.3, 0.7], *_box(2, -3, 3), xtol_rel=1e-6, maxeval=300),
    # the initial simplex's branches (nldrmd.c:140-161)
    _p("on_ub", 2, rosenbrock, [1.0, 0.9], *_box(2, 0, 1), dx=[0.2, 0.2], xtol_rel=1e-6, maxeval=120),        # other direction; onto ub
    _p("on_lb", 2, rosenbrock, [0.0, 0.1], *_box(2, 0, 1), dx=[-0.2, -0.2], xtol_rel=1e-6, maxeval=120),      # other direction; onto lb
    _p("narrow", 2, rosenbrock, [0.0005, 0.0095], *_box(2, 0, 0.01), dx=[-0.1, 0.1], xtol_rel=1e-6, maxeval=120),   # towards the further bound
    _p("tiny_step", 2, rosenbrock, [1.0, 2.0], *_box(2, -5, 5), dx=[1e-14, 2e-14], expect=FAILURE, nevals=1, maxeval=50),
    # the stops
    _p("maxeval1", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MAXEVAL_REACHED, nevals=1, maxeval=1),
    _p("maxeval3", 5, wquad, [0.3, -0.2, 0.1, 0.4, -0.5], *_box(5, -1, 1), expect=MAXEVAL_REACHED, nevals=3, maxeval=3),
    _p("stopval_start", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MINF_MAX_REACHED, nevals=1, minf_max=25.0),
    _p("stopval_mid", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MINF_MAX_REACHED, minf_max=1.0, maxeval=400),
    _p("ftol_rel", 2, rosenbrock_plus_one, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=FTOL_REACHED, ftol_rel=1e-4, maxeval=400),
    _p("ftol_abs", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=FTOL_REACHED, ftol_abs=1e-3, maxeval=400),
    _p("xtol_rel", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=XTOL_REACHED, xtol_rel=1e-3, maxeval=400),
    _p("xtol_abs", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=XTOL_REACHED, xtol_rel=1e-12, xtol_abs=[1e-2, 2e-2], maxeval=400),
    _p("x_weights", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=XTOL_REACHED, xtol_rel=1e-3, x_weights=[1.0, 100.0], xtol_abs=[1e-9, 1e-9],
       maxeval=400),
    # raised from a given evaluation on: inside the initial simplex (evaluations 1 .. 3) and behind it
    _p("forced2", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=FORCED_STOP, nevals=2, forced_from=2, maxeval=400),
    _p("forced9", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=FORCED_STOP, nevals=9, forced_from=9, maxeval=400),
    _p("timeout2", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MAXTIME_REACHED, nevals=2, timeout_from=2, maxeval=400),
    _p("timeout9", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MAXTIME_REACHED, nevals=9, timeout_from=9, maxeval=400),
]


def reference_of(E, p):
    """the real reference's run of problem p.  forced_from = k: its callback calls nlopt_force_stop inside its k-th call.  timeout_from =
    k: the reference's clock cannot be told to run out at a given evaluation without waiting for it, but CHECK_EVAL asks for the time
    right behind maxeval, with nothing in between (nldrmd.c:86-87) — so the run that times out behind evaluation k IS the run with
    maxeval = k, its code MAXTIME_REACHED instead of MAXEVAL_REACHED (k is below every problem's own maxeval)."""
    kw = dict(p["kw"])
    force_at, timeout = kw.pop("forced_from", None), kw.pop("timeout_from", None)
    if timeout is not None:
        assert kw.get("maxeval", 0) == 0 or timeout < kw["maxeval"]
        kw["maxeval"] = timeout
    r = E.reference(p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], force_at=force_at, **kw)
    if timeout is not None:
        assert r["ret"] == [MAXEVAL_REACHED]
        r["ret"] = [MAXTIME_REACHED]
    return r


def check_expectations(p, r):
    """what the problem is there for really happens in the reference's run"""
    if p["expect"] is not None:
        assert r["ret"] == [p["expect"]], (p["name"], r["ret"])
    if p["nevals"] is not None:
        assert r["nevals"] == [p["nevals"]], (p["name"], r["nevals"])
    else:
        assert r["nevals"][0] > p["n"] + 1, (p["name"], r["nevals"])      # (the search got past its initial simplex)


def stays_finished(a):
    """a search whose state was 2 after a launch has state 2 after every later one"""
    for i, at in enumerate(a["finished_at"]):
        assert at is not None and all(s[i] == 2 for s in a["seen"][at:])


@pytest.mark.parametrize("p", PROBLEMS, ids=[p["name"] for p in PROBLEMS])
def test_coroutine_kernel_asks_for_the_references_points_and_returns_its_result(kernel, p):
    E, K = kernel
    r = reference_of(E, p)
    check_expectations(p, r)
    a = E.run_ext(K, p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], **p["kw"])
    E.same(a, r)
    stays_finished(a)
    if p["expect"] == FAILURE:
        assert a["cols"] == [0] and b"too small in dimension 0" in r["errmsg"][0] and np.array_equal(a["x"][0], p["x0"])


def classify(n, xs, fs, dx):
    """the branches of an unbounded Nelder-Mead run, from the points and values a callback saw: the simplex is replayed with the recorded
    values (no objective call), every point the replay expects is compared with the recorded one, and each iteration is labelled"""
    best, fbest = np.array(xs[0]), fs[0]
    pts, fv, k = [np.array(xs[0])], [fs[0]], 1
    for i in range(n):
        pt = best.copy(); pt[i] += dx[i]
        assert np.array_equal(pt, xs[k])
        pts.append(pt); fv.append(fs[k])
        if fs[k] <= fbest:
            best, fbest = pt.copy(), fs[k]
        k += 1
    seen = []
    while k < len(xs):
        order = sorted(range(n + 1), key=lambda i: (fv[i], i))
        lo_, hi_, pred = order[0], order[-1], order[-2]
        c = np.zeros(n)
        for i in range(n + 1):
            if i != hi_:
                c = c + pts[i]
        c = c * (1.0 / n)
        xr = c + 1.0 * (c - pts[hi_])
        assert np.array_equal(xr, xs[k])
        fr = fs[k]; k += 1
        if fr < fv[lo_]:
            if k >= len(xs):
                break
            xe = c + 2.0 * (c - pts[hi_])
            assert np.array_equal(xe, xs[k])
            fe = fs[k]; k += 1
            seen.append("expansion")
            pts[hi_], fv[hi_] = (xr, fr) if fe >= fr else (xe, fe)
        elif fr < fv[pred]:
            seen.append("reflection")
            pts[hi_], fv[hi_] = xr, fr
        else:
            if k >= len(xs):
                break
            inside = fv[hi_] <= fr
            xc = c + (-0.5 if inside else 0.5) * (c - pts[hi_])
            assert np.array_equal(xc, xs[k])
            fc = fs[k]; k += 1
            if fc < fr and fc < fv[hi_]:
                seen.append("inside contraction" if inside else "outside contraction")
                pts[hi_], fv[hi_] = xc, fc
            else:
                seen.append("shrink")
                for i in range(n + 1):
                    if i != lo_ and k < len(xs):
                        pts[i] = pts[lo_] + (-0.5) * (pts[lo_] - pts[i])
                        assert np.array_equal(pts[i], xs[k])
                        fv[i] = fs[k]; k += 1
    return set(seen)


def test_rosenbrock_takes_every_branch(kernel):
    """so that the n = 2 case cannot silently stop covering one: read from the REFERENCE's trace"""
    E, _ = kernel
    p = next(q for q in PROBLEMS if q["name"] == "rosen2")
    r = reference_of(E, p)
    assert classify(2, r["asked"][0], r["fseq"][0], p["kw"]["dx"]) == {"reflection", "expansion", "inside contraction", "outside contraction", "shrink"}


# the searches above that share n (and here a box and the stops) as ONE launch sequence from different starts, with different objectives
BATCHES = [
    dict(name="n2", n=2, lb=np.full(2, -3.0), ub=np.full(2, 3.0), kw=dict(xtol_rel=1e-6, maxeval=150),
         searches=[(rosenbrock, ROSEN_START), (steps, [0.3, 0.7]), (rosenbrock, [3.0, 3.0]), (flat, [1.0, 2.0]), (rosenbrock, [2.0, -1.5])]),
    dict(name="n5", n=5, lb=np.full(5, -1.0), ub=np.full(5, 1.0), kw=dict(xtol_rel=1e-4, maxeval=300),
         searches=[(wquad, [0.3, -0.2, 0.1, 0.4, -0.5]), (ridge, [0.9, 0.9, -0.9, 0.0, 1.0]), (wquad, [-1.0, -1.0, -1.0, -1.0, -1.0])]),
    dict(name="n65", n=65, lb=np.full(65, -2.0), ub=np.full(65, 2.0), kw=dict(xtol_rel=1e-6, maxeval=90),
         searches=[(ridge, _R.uniform(-1.5, 1.5, 65)), (rosenbrock, _R.uniform(-1.5, 1.5, 65))]),
]


@pytest.mark.parametrize("b", BATCHES, ids=[b["name"] for b in BATCHES])
def test_searches_of_one_batch_equal_their_lone_runs_and_stay_finished(kernel, b):
    E, K = kernel
    fs, starts = [s[0] for s in b["searches"]], np.array([s[1] for s in b["searches"]], dtype=np.float64)
    a = E.run_ext(K, b["n"], starts, b["lb"], b["ub"], fs, **b["kw"])
    r = E.reference(b["n"], starts, b["lb"], b["ub"], fs, **b["kw"])
    E.same(a, r)
    stays_finished(a)
    for i, (f, s) in enumerate(b["searches"]):
        lone = E.run_ext(K, b["n"], [s], b["lb"], b["ub"], f, **b["kw"])
        assert lone["ret"][0] == a["ret"][i] and lone["nevals"][0] == a["nevals"][i]
        assert np.array_equal(E.bits(lone["f"][0]), E.bits(a["f"][i])) and np.array_equal(E.bits(lone["x"][0]), E.bits(a["x"][i]))
    if b["name"] == "n2":
        assert len(set(a["finished_at"])) > 1 and a["launches"] == max(r["nevals"]) + 1      # they end at different launches


def nan_among_healthy(E, K, mem=None):
    """n = 8, five searches, the third one's objective returns NaN from its 10th evaluation on (outside the parity contract): it must
    still end at maxeval = 200, and the other four must equal their lone runs — and the reference's"""
    n, lb, ub, kw = 8, np.full(8, -2.0), np.full(8, 2.0), dict(ftol_rel=1e-10, maxeval=200)
    starts = np.random.default_rng(2950).uniform(-1.5, 1.5, (5, n))
    count = [0]

    def sick(x):
        count[0] += 1
        return rosenbrock(x) if count[0] < 10 else float("nan")
    fs = [rosenbrock, ridge, sick, rosenbrock, ridge]
    a = E.run_ext(K, n, starts, lb, ub, fs, mem=mem, **kw)
    assert a["ret"][2] == MAXEVAL_REACHED and a["nevals"][2] == 200 and count[0] == 200
    healthy = [0, 1, 3, 4]
    r = E.reference(n, starts[healthy], lb, ub, [fs[i] for i in healthy], **kw)
    E.same(dict((k, [a[k][i] for i in healthy]) for k in ("ret", "nevals", "asked", "f", "x")), r)
    for i in healthy:
        lone = E.run_ext(K, n, [starts[i]], lb, ub, fs[i], mem=mem, **kw)
        assert lone["ret"][0] == a["ret"][i] and lone["nevals"][0] == a["nevals"][i]
        assert np.array_equal(E.bits(lone["f"][0]), E.bits(a["f"][i])) and np.array_equal(E.bits(lone["x"][0]), E.bits(a["x"][i]))
    stays_finished(a)


def test_a_search_whose_objective_turns_nan_ends_at_maxeval_and_disturbs_nobody(kernel):
    nan_among_healthy(*kernel)


def test_launcher_contract_on_the_cpu(kernel):
    E, K = kernel
    E.bind(K)
    assert [K.nla_nldrmd_serves(n) for n in (0, 1, 256, 257)] == [0, 1, 1, 0]
    assert [K.nla_nldrmd_work_doubles(n, 1) > 0 for n in (0, 1, 256, 257)] == [False, True, True, False]
    assert [K.nla_nldrmd_save_bytes(n) > 0 for n in (0, 1, 256, 257)] == [False, True, True, False]
    assert K.nla_nldrmd_save_bytes(5) % 128 == 0 and (K.nla_nldrmd_work_doubles(5, 3) - K.nla_nldrmd_work_doubles(5, 2)) % 16 == 0
    n, ld, count = 4, 4, 2
    X0 = np.random.default_rng(2900).uniform(-1, 1, (count, ld))
    lb, ub = np.full(n, -2.0), np.full(n, 2.0)

    def call(n=n, ld=ld, count=count, obj=E.NLA_OBJ_EXTERNAL, work=True, ext=True, drop=None):
        rows, ns = max(count, 1), min(max(n, 1), 256)
        X, req, out = X0.copy(), np.full((rows, 2), 7, dtype=np.int32), np.full(rows * 3, -1.0)
        bufs = dict(req=req, EX=np.zeros((rows, max(ld, 1))), EF=np.zeros(rows), save=np.zeros(max(8, K.nla_nldrmd_save_bytes(ns) * rows // 8)))
        e = E.Ext(*[None if drop == k else bufs[k].ctypes.data for k in ("req", "EX")], np.zeros(8).ctypes.data,
                  *[None if drop == k else bufs[k].ctypes.data for k in ("EF", "save")], 0, 0, 0, 0)
        w = np.zeros(max(8, K.nla_nldrmd_work_doubles(ns, rows)))
        P = E.Params(-np.inf, 0.0, 0.0, 1e-6, 50, 0, 1.0, None, None, None, None, 0, None)
        rc = K.nla_k_nldrmd_batch(obj, n, ld, count, lb.ctypes.data, ub.ctypes.data, None, X.ctypes.data, w.ctypes.data if work else None, C.byref(P),
                                  out.ctypes.data, C.byref(e) if ext else None, None)
        return rc, np.array_equal(X, X0) and np.all(req == 7) and np.all(out == -1.0)
    # refusals: nothing is launched — X, req and the result records stay as they were
    for kw in (dict(n=0), dict(n=257, ld=258), dict(ld=3), dict(work=False), dict(ext=False), dict(drop="req"), dict(drop="EX"), dict(drop="EF"),
               dict(drop="save"), dict(obj=-2), dict(obj=99, ext=False), dict(obj=5)):          # (a compiled-in objective takes no ext)
        rc, untouched = call(**kw)
        assert rc != 0 and untouched, kw
    assert call(count=0) == (0, True) and call(count=-1) == (0, True)
    rc, untouched = call()
    assert rc == 0 and not untouched                       # (and the same call with nothing missing does launch)
