"""CPU twin of tests/test_gpu_cobyla_ext.py: hip/cobyla_ext.hip (the batched LN_COBYLA search of hip/cobyla_search.h as a COROUTINE around
an objective outside the kernel — what GN_MLSL runs for a user-supplied device objective) compiled by g++ over tools/simt_emu, 64
lockstep threads per search.  The test is the host side of the coroutine (tools/cobyla_emu_check.run_ext): launch, read req, evaluate
every waiting row of EX with the sequential host twin of a compiled-in objective, write EF, launch again with resume = 1.  The oracle
is the REAL reference's nlopt_optimize(LN_COBYLA) on the same twin, its callback recording every point: result code, evaluation
count, f, the minimiser AND the sequence of points each search asked for are the reference's bit for bit — no tolerance anywhere
(sphere / Rosenbrock: no transcendental; every value the kernel is given is the value the reference was given).
The emulation runs one workgroup at a time in ONE static LDS block, so a search that came back with anything but its own saved state
would continue from another search's vectors.  What it cannot see is the device's memory model: the GPU twin."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

import _oracle as O
import test_cobyla_differential as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MINF_MAX_REACHED, XTOL_REACHED, MAXEVAL_REACHED, FORCED_STOP, INVALID_ARGS = 2, 4, 5, -5, -2

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
    return E, C.CDLL(E.build_ext()), C.CDLL(E.build())


def twin(obj):
    """the sequential host twin of a compiled-in objective (the emulated library's nlopt_amd_objective), as a Python callable on arrays"""
    A = C.CDLL(T.EMU)
    A.nlopt_amd_objective.restype = C.c_void_p
    f = O.FUNC(A.nlopt_amd_objective(O.OBJ[obj]))
    return lambda x: f(len(x), T.dp(np.ascontiguousarray(x, dtype=np.float64)), None, None)


def reference(obj, n, starts, lb, ub, xtol_rel=1e-6, maxeval=0, dx=None, maximise=False, stopval=None, force_at=None, tw=None):
    """the starts one after another through the real reference's LN_COBYLA; the callback is the twin (tw, or this file's), records
    every point it is given and (force_at = k) calls nlopt_force_stop inside its k-th call"""
    R, tw = T.more_bind(O.ref()), tw or twin(obj)
    R.nlopt_force_stop.argtypes = [C.c_void_p]
    out = dict(x=[], f=[], ret=[], nevals=[], asked=[])
    for s in starts:
        opt = R.nlopt_create(T.LN_COBYLA, n)
        pts = []

        def cb(nn, x, g, d):
            pts.append(np.array(x[:nn], dtype=np.float64))
            if force_at is not None and len(pts) == force_at:
                R.nlopt_force_stop(opt)
            return tw(pts[-1])
        fcb = O.FUNC(cb)
        R.nlopt_set_lower_bounds(opt, T.dp(lb)); R.nlopt_set_upper_bounds(opt, T.dp(ub))
        (R.nlopt_set_max_objective if maximise else R.nlopt_set_min_objective)(opt, C.cast(fcb, C.c_void_p), None)
        R.nlopt_set_xtol_rel(opt, xtol_rel)
        if maxeval:
            R.nlopt_set_maxeval(opt, maxeval)
        if stopval is not None:
            R.nlopt_set_stopval(opt, stopval)
        if dx is not None:
            R.nlopt_set_initial_step(opt, T.dp(dx))
        x, minf = np.array(s, dtype=np.float64), C.c_double(0)
        out["ret"].append(R.nlopt_optimize(opt, T.dp(x), C.byref(minf)))
        out["f"].append(minf.value); out["x"].append(x); out["nevals"].append(R.nlopt_get_numevals(opt)); out["asked"].append(pts)
        R.nlopt_destroy(opt)
    out["x"], out["f"] = np.array(out["x"]), np.array(out["f"])
    return out


def same(a, r, sign=1.0):
    """results and, per search, the sequence of requested points: the reference's"""
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"], (a["ret"], r["ret"], a["nevals"], r["nevals"])
    assert np.array_equal(sign * a["f"], r["f"]) and np.array_equal(a["x"], r["x"]), (a["f"], r["f"])
    for pa, pr in zip(a["asked"], r["asked"]):
        assert len(pa) == len(pr) and all(np.array_equal(u, v) for u, v in zip(pa, pr))


def stays_finished(a):
    """a search whose state was 2 after a launch has state 2 after every later one"""
    for i, at in enumerate(a["finished_at"]):
        assert at is not None and all(s[i] == 2 for s in a["seen"][at:])


def box(obj, n, kind="plain"):
    _, lo, hi = O.golden_x0(obj, n)
    lb, ub = np.full(n, float(lo)), np.full(n, float(hi))
    if kind == "halfinf":                                  # the box of tests/test_cobyla_global_emu.py: m = 2n - 4 rows
        ub[0] = np.inf; lb[1] = -np.inf; lb[2] = -np.inf; ub[2] = np.inf
    return lo, hi, lb, ub


# n = 1, 2: the smallest simplices; n = 6 half-infinite: fewer rows than 2n; n = 65: two trips of the 64 lanes over a column and
# over the LDS block on its way to the save record and back, n odd; n = 7 with maxeval 3: the stop inside the initial simplex
@pytest.mark.parametrize("obj,n,count,maxeval,xtol,kind", [("sphere", 1, 1, 0, 1e-6, "plain"), ("sphere", 2, 1, 0, 1e-6, "plain"),
                                                           ("rosenbrock", 6, 1, 300, 1e-7, "halfinf"), ("rosenbrock", 65, 2, 110, 1e-6, "plain"),
                                                           ("rosenbrock", 7, 1, 3, 1e-6, "plain")])
def test_coroutine_cobyla_kernel_asks_for_the_references_points_and_returns_its_result(kernels, obj, n, count, maxeval, xtol, kind):
    E, K, _ = kernels
    lo, hi, lb, ub = box(obj, n, kind)
    starts = np.random.default_rng(4000 + n).uniform(lo, hi, (count, n))
    a = E.run_ext(K, n, starts, lb, ub, twin(obj), xtol_rel=xtol, maxeval=maxeval)
    r = reference(obj, n, starts, lb, ub, xtol, maxeval)
    same(a, r)
    stays_finished(a)
    if maxeval == 3:
        assert a["ret"] == [MAXEVAL_REACHED] and a["nevals"] == [3]


def test_searches_of_one_batch_that_end_at_different_times(kernels):
    """Rosenbrock n = 7, three starts, xtol_rel = 0.02, 150 evaluations at the most: two searches stop by themselves after different
    numbers of evaluations and the third runs into the limit, so the finished ones sit through the later resumes untouched; the
    same starts through the LDS kernel (objective inside, exact order) give the same bits"""
    E, K, KL = kernels
    n = 7
    lo, hi, lb, ub = box("rosenbrock", n)
    starts = np.random.default_rng(4100).uniform(lo, hi, (3, n))
    r = reference("rosenbrock", n, starts, lb, ub, 0.02, 150)
    assert r["ret"] == [XTOL_REACHED, XTOL_REACHED, MAXEVAL_REACHED] and len(set(r["nevals"])) == 3, (r["ret"], r["nevals"])
    a = E.run_ext(K, n, starts, lb, ub, twin("rosenbrock"), xtol_rel=0.02, maxeval=150)
    same(a, r)
    stays_finished(a)
    assert a["launches"] == max(r["nevals"]) + 1 and sorted(a["finished_at"]) == sorted(r["nevals"])
    b = E.run(KL, "rosenbrock", n, starts, lb, ub, xtol_rel=0.02, maxeval=150)
    assert a["ret"] == b["ret"] and a["nevals"] == b["nevals"] and np.array_equal(a["f"], b["f"]) and np.array_equal(a["x"], b["x"])


def test_stop_value_above_the_first_value_ends_the_search_at_its_first_resume(kernels):
    E, K, _ = kernels
    n = 4
    lo, hi, lb, ub = box("sphere", n)
    starts = np.random.default_rng(4200).uniform(lo, hi, (2, n))
    stopval = max(twin("sphere")(s) for s in starts) + 1.0
    a = E.run_ext(K, n, starts, lb, ub, twin("sphere"), minf_max=stopval)
    same(a, reference("sphere", n, starts, lb, ub, stopval=stopval))
    assert a["ret"] == [MINF_MAX_REACHED] * 2 and a["nevals"] == [1, 1] and a["launches"] == 2


def test_given_initial_step_with_unequal_entries(kernels):
    """the rescaled search: the points that go out are unscaled again"""
    E, K, _ = kernels
    n = 5
    lo, hi, lb, ub = box("sphere", n)
    starts = np.random.default_rng(4300).uniform(lo, hi, (2, n))
    dx = np.linspace(0.3, 1.7, n) * 0.1 * (hi - lo)
    a = E.run_ext(K, n, starts, lb, ub, twin("sphere"), xtol_rel=1e-4, maxeval=60, dx=dx)
    same(a, reference("sphere", n, starts, lb, ub, 1e-4, 60, dx=dx))


def test_maximisation_takes_the_delivered_value_as_it_is(kernels):
    """the caller delivers -f (as the user's kernel does with sign = -1); the kernel must not apply a sign of its own.  Oracle: the
    reference MAXIMISING the twin (sphere in a box: the search runs into a corner)"""
    E, K, _ = kernels
    n = 3
    lo, hi, lb, ub = box("sphere", n)
    starts = np.random.default_rng(4400).uniform(lo, hi, (2, n))
    tw = twin("sphere")
    a = E.run_ext(K, n, starts, lb, ub, lambda x: -tw(x), xtol_rel=1e-4, maxeval=300)
    same(a, reference("sphere", n, starts, lb, ub, 1e-4, 300, maximise=True), sign=-1.0)


@pytest.mark.parametrize("k", [5, 10])
def test_forced_stop_from_the_kth_relaunch_on(kernels, k):
    """n = 7: ext.forced = 1 from relaunch k on (k = 5: inside the initial simplex, k = n + 3: behind it).  Relaunch k delivers the
    k-th value; the search takes it and meets the flag in front of its next evaluation — the reference whose callback calls
    nlopt_force_stop inside its k-th call"""
    E, K, _ = kernels
    n = 7
    lo, hi, lb, ub = box("rosenbrock", n)
    starts = np.random.default_rng(4500 + k).uniform(lo, hi, (2, n))
    a = E.run_ext(K, n, starts, lb, ub, twin("rosenbrock"), forced_from=k)
    r = reference("rosenbrock", n, starts, lb, ub, force_at=k)
    same(a, r)
    assert a["ret"] == [FORCED_STOP] * 2 and a["nevals"] == [k, k] and a["launches"] == k + 1


def test_coroutine_cobyla_launcher_contract_on_the_cpu(kernels):
    E, K, _ = kernels
    E.ext_bind(K)
    assert [K.nla_cobyla_ext_work_doubles(n, 1) > 0 for n in (0, 1, 51, 52, 256, 257)] == [False, True, True, True, True, False]
    assert [K.nla_cobyla_save_bytes(n) > 0 for n in (0, 1, 256, 257)] == [False, True, True, False]
    assert K.nla_cobyla_ext_work_doubles(256, 320) * 8 < 1.3e9 and K.nla_cobyla_save_bytes(256) < 64 * 1024
    # refusals: nothing is launched — X, req and the result records stay as they were
    n, ld, count = 4, 4, 2
    X0 = np.random.default_rng(4600).uniform(-1, 1, (count, ld))
    lb, ub = np.full(n, -2.0), np.full(n, 2.0)

    def call(n=n, ld=ld, count=count, work=True, ext=True, drop=None):
        rows = max(count, 1)                               # (count <= 0: buffers of one search, which nothing may touch either)
        X, req, out = X0.copy(), np.full((rows, 2), 7, dtype=np.int32), np.full(rows * 3, -1.0)
        bufs = dict(req=req, EX=np.zeros((rows, max(ld, 1))), EF=np.zeros(rows), save=np.zeros(max(8, K.nla_cobyla_save_bytes(min(max(n, 1), 256)) * rows // 8)))
        e = E.Ext(*[None if drop == k else bufs[k].ctypes.data for k in ("req", "EX")], np.zeros(8).ctypes.data,
                  *[None if drop == k else bufs[k].ctypes.data for k in ("EF", "save")], 0, 0, 0, 0)
        w = np.zeros(max(8, K.nla_cobyla_ext_work_doubles(min(max(n, 1), 256), rows)))
        P = E.Params(-np.inf, 0.0, 0.0, 1e-6, 50, 0, 1.0, None, None, None)
        rc = K.nla_k_cobyla_batch_ext(n, ld, count, lb.ctypes.data, ub.ctypes.data, None, X.ctypes.data, w.ctypes.data if work else None, C.byref(P),
                                      out.ctypes.data, C.byref(e) if ext else None, None)
        return rc, np.array_equal(X, X0) and np.all(req == 7) and np.all(out == -1.0)
    for kw in (dict(n=0), dict(n=257, ld=258), dict(ld=3), dict(work=False), dict(ext=False), dict(drop="req"), dict(drop="EX"), dict(drop="EF"), dict(drop="save")):
        rc, untouched = call(**kw)
        assert rc != 0 and untouched, kw
    assert call(count=0) == (0, True) and call(count=-1) == (0, True)
    rc, untouched = call()
    assert rc == 0 and not untouched                       # (and the same call with nothing missing does launch)
    # a fixed coordinate: refused before any objective call — INVALID_ARGS, state 2 at once, nothing asked for, the start untouched
    n = 7
    lo, hi, lb, ub = box("rosenbrock", n)
    starts = np.random.default_rng(4700).uniform(lo, hi, (2, n))
    lb[[0, 3]] = ub[[0, 3]] = starts[0, [0, 3]]
    starts[:, [0, 3]] = lb[[0, 3]]
    a = E.run_ext(K, n, starts, lb, ub, twin("rosenbrock"), maxeval=300)
    assert a["ret"] == [INVALID_ARGS] * 2 and a["nevals"] == [0, 0] and a["launches"] == 1 and a["asked"] == [[], []]
    assert np.all(a["seen"][0] == 2) and np.all(a["f"] == np.inf) and np.array_equal(a["x"], starts)
