"""CPU twin of tests/test_gpu_sbplx.py's kernel-level part: hip/sbplx_kernels.hip (batched NLOPT_LN_SBPLX: hip/nm_search.h with psi > 0 under
sbplx_minimize's outer loop, one wavefront per search) compiled by g++ over tools/simt_emu and run AS A COROUTINE
(tools/sbplx_emu_check.run_ext).  The oracle is the REAL reference's nlopt_optimize(NLOPT_LN_SBPLX) on the same Python objective, its
callback recording every point: the result code, the evaluation count, minf, x AND the whole sequence of FULL points each search asked
for are the reference's bit for bit — no tolerance anywhere.  What a problem is there for is asserted on the REFERENCE's run, from its
own trace (sbplx_verbose: one line per subspace, one per pass).  PROBLEMS and BATCHES are the lists the GPU test imports."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

import _oracle as O
import test_nldrmd_emu as NM
from test_nldrmd_emu import (FORCED_STOP, FTOL_REACHED, MAXEVAL_REACHED, MAXTIME_REACHED, MINF_MAX_REACHED, XTOL_REACHED, ROSEN_START, UNB2,
                             _box, flat, parabola, ridge, rosenbrock, rosenbrock_plus_one, stays_finished, steps, wquad)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not shutil.which("g++") or not O.have_ref(), reason="no g++ / oracle/_ref here")


def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import sbplx_emu_check as E
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return E


@pytest.fixture(scope="module")
def kernel():
    E = _tool()
    return E, C.CDLL(E.build())


def scaled(x):
    """coordinates of very different curvature: |dx| differs by orders of magnitude between them, which is what the partition looks at"""
    s = 0.0
    for i in range(len(x)):
        d = x[i] - 0.1 * (i % 7)
        s += (10.0 ** (i % 4)) * d * d
    return s


def _p(name, n, f, x0, lb, ub, expect=None, nevals=None, sizes=None, passes=None, min_passes=None, **kw):
    """expect / nevals / sizes (the set of subspace sizes) / passes / min_passes (completed passes): asserted on the reference's run"""
    return dict(name=name, n=n, f=f, x0=np.array(x0, dtype=np.float64), lb=lb, ub=ub, expect=expect, nevals=nevals, sizes=sizes, passes=passes,
                min_passes=min_passes, kw=kw)


def _scaled_start(n):
    return np.random.default_rng(3000 + (0 if n == 7 else n)).uniform(-1.5, 1.5, n)


ROSEN5_START = [-1.2, 1.0, 0.5, 0.2, -0.3]
FACE5_START = [0.3, -0.2, 0.1, 0.4, -0.5]
PROBLEMS = [
    # n = 1 and n = 2: a single subspace, nsubs == 1, scale = psi
    _p("n1", 1, parabola, [1.5], *_box(1, -2, 2), expect=XTOL_REACHED, nevals=105, sizes={1}, passes=13, xtol_rel=1e-8),
    _p("n2", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=XTOL_REACHED, nevals=346, sizes={2}, passes=12, xtol_rel=1e-8),
    # n = 3: subspaces of 2 + 1, stopped early
    _p("n3", 3, rosenbrock, [-1.2, 1.0, 0.5], *_box(3, -2, 2), expect=MAXEVAL_REACHED, nevals=40, sizes={1, 2}, maxeval=40),
    # the partition: every subspace size occurs, the permutation changes between passes (test_scaled7_...)
    _p("scaled7", 7, scaled, _scaled_start(7), *_box(7, -2, 2), expect=XTOL_REACHED, nevals=1313, sizes={1, 2, 3, 4, 5}, passes=23, xtol_rel=1e-6, maxeval=1500),
    # coordinates pinned to the box have dx = 0 in later passes: the stable order of ties decides p
    _p("face5", 5, wquad, FACE5_START, *_box(5, -1, 1), expect=XTOL_REACHED, nevals=125, passes=9, xtol_rel=1e-8),
    # every comparison and every |dx| is a tie
    _p("flat", 4, flat, [1.0, 2.0, 3.0, -1.0], *_box(4, -5, 5), expect=XTOL_REACHED, nevals=397, sizes={2}),
    # the outer ftol test with fdiff_max
    _p("ftol", 5, rosenbrock_plus_one, ROSEN5_START, *_box(5, -3, 3), expect=FTOL_REACHED, nevals=151, passes=3, ftol_rel=1e-4),
    # the strided loops wrap, the rank count straddles lanes; the reference is in its second pass
    _p("n63", 63, scaled, _scaled_start(63), *_box(63, -2, 2), expect=MAXEVAL_REACHED, min_passes=1, maxeval=800),
    _p("n64", 64, scaled, _scaled_start(64), *_box(64, -2, 2), expect=MAXEVAL_REACHED, min_passes=1, maxeval=800),
    _p("n65", 65, scaled, _scaled_start(65), *_box(65, -2, 2), expect=MAXEVAL_REACHED, min_passes=1, maxeval=800),
    # the initial simplex's bound branches (nldrmd.c:140-161)
    _p("on_ub", 2, rosenbrock, [1.0, 0.9], *_box(2, 0, 1), dx=[0.2, 0.2], xtol_rel=1e-6, maxeval=120),
    _p("on_lb", 2, rosenbrock, [0.0, 0.1], *_box(2, 0, 1), dx=[-0.2, -0.2], xtol_rel=1e-6, maxeval=120),
    _p("narrow", 2, rosenbrock, [0.0005, 0.0095], *_box(2, 0, 0.01), dx=[-0.1, 0.1], xtol_rel=1e-6, maxeval=120),
    # a too-small step: FAILURE inside, XTOL_REACHED outside, the whole search ends
    _p("tiny_step", 2, rosenbrock, [1.0, 2.0], *_box(2, -5, 5), dx=[1e-14, 2e-14], expect=XTOL_REACHED, nevals=1, maxeval=50),
    # the stops
    _p("maxeval1", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MAXEVAL_REACHED, nevals=1, maxeval=1),
    _p("maxeval_sub2", 7, scaled, _scaled_start(7), *_box(7, -2, 2), expect=MAXEVAL_REACHED, nevals=20, maxeval=20),    # test_maxeval_sub2_...
    _p("stopval_start", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MINF_MAX_REACHED, nevals=1, minf_max=25.0),
    _p("stopval_mid", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MINF_MAX_REACHED, minf_max=1.0, maxeval=400),
    _p("xtol_abs", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=XTOL_REACHED, xtol_rel=1e-12, xtol_abs=[1e-2, 2e-2], maxeval=600),
    _p("x_weights", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=XTOL_REACHED, xtol_rel=1e-3, x_weights=[1.0, 100.0], xtol_abs=[1e-9, 1e-9],
       maxeval=600),
    # raised from a given evaluation on: inside an initial simplex (evaluations 2 .. 3) and behind it
    _p("forced2", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=FORCED_STOP, nevals=2, forced_from=2, maxeval=400),
    _p("forced9", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=FORCED_STOP, nevals=9, forced_from=9, maxeval=400),
    _p("timeout2", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MAXTIME_REACHED, nevals=2, timeout_from=2, maxeval=400),
    _p("timeout9", 2, rosenbrock, ROSEN_START, *UNB2, dx=[0.5, 0.5], expect=MAXTIME_REACHED, nevals=9, timeout_from=9, maxeval=400),
]

_REFS = {}


def reference_of(E, p):
    """the real reference's run of problem p, computed once and shared (test_nldrmd_emu.reference_of: forced_from through nlopt_force_stop
    in the callback; timeout_from = k is the run with maxeval = k, CHECK_EVAL being the same macro)"""
    if p["name"] not in _REFS:
        _REFS[p["name"]] = NM.reference_of(E, p)
    return _REFS[p["name"]]


def check_expectations(p, r):
    """what the problem is there for really happens in the reference's run"""
    if p["expect"] is not None:
        assert r["ret"] == [p["expect"]], (p["name"], r["ret"])
    if p["nevals"] is not None:
        assert r["nevals"] == [p["nevals"]], (p["name"], r["nevals"])
    else:
        assert r["nevals"][0] > p["n"] + 1, (p["name"], r["nevals"])      # (the search got past its first initial simplex)
    sizes = set(s[1] for s in r["subspaces"][0])
    if p["sizes"] is not None:
        assert sizes == p["sizes"], (p["name"], sizes)
    if p["passes"] is not None:
        assert r["passes"] == [p["passes"]], (p["name"], r["passes"])
    if p["min_passes"] is not None:
        assert r["passes"][0] >= p["min_passes"], (p["name"], r["passes"])
    assert sum(s[2] for s in r["subspaces"][0]) == r["nevals"][0] - 1     # (the trace accounts for every evaluation behind the first)


@pytest.mark.parametrize("p", PROBLEMS, ids=[p["name"] for p in PROBLEMS])
def test_coroutine_kernel_asks_for_the_references_points_and_returns_its_result(kernel, p):
    E, K = kernel
    r = reference_of(E, p)
    check_expectations(p, r)
    a = E.run_ext(K, p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], **p["kw"])
    E.same(a, r)
    stays_finished(a)
    ended_by_a_small_step(a, r)
    if p["name"] == "tiny_step":
        assert a["cols"] == [1] and np.array_equal(a["x"][0], p["x0"])


def ended_by_a_small_step(a, r):
    """FAILURE inside becomes XTOL_REACHED and ends the search (scaled7 ends this way too): the record has 1 + the subspace's dimension
    exactly when the reference's nlopt_stop_msg has left its message, and the dimension is the message's"""
    msg = r["errmsg"][0] or b""
    if a["cols"][0] > 0:
        assert a["ret"] == [XTOL_REACHED] and ("too small in dimension %d:" % (a["cols"][0] - 1)).encode() in msg, (a["cols"], msg)
    else:
        assert b"too small" not in msg, msg


def partitions(r):
    """per completed or begun pass of the reference's run 0: the tuple of coordinate sets its subspaces worked on, read from the requested
    points (within a subspace's evaluations only its coordinates vary) with the evaluation counts of the reference's trace"""
    pts, pos, out = r["asked"][0], 1, []
    for is_, ns, cnt in r["subspaces"][0]:
        seg = np.array(pts[pos:pos + cnt])
        pos += cnt
        if is_ == 0:
            out.append([])
        out[-1].append(frozenset(np.nonzero(np.any(seg != seg[0], axis=0))[0]) if len(seg) > 1 else frozenset())
    return [tuple(p) for p in out]


def test_scaled7_has_every_subspace_size_and_permutations_that_differ_between_passes(kernel):
    E, _ = kernel
    r = reference_of(E, next(q for q in PROBLEMS if q["name"] == "scaled7"))
    assert set(s[1] for s in r["subspaces"][0]) == {1, 2, 3, 4, 5}
    parts = partitions(r)
    assert len(parts) >= 3 and len(set(parts)) >= 2, parts
    assert parts[0][0] == frozenset({0, 1})                              # the first pass: dx = 0 everywhere, p is the identity, ns = nsmin


def test_face5_and_flat_sort_ties(kernel):
    """face5: in a later pass at least two coordinates have dx == 0 exactly (pinned to the box); flat: every |dx| is 0 in every pass"""
    E, _ = kernel
    r = reference_of(E, next(q for q in PROBLEMS if q["name"] == "face5"))
    assert int(np.sum(np.abs(r["x"][0]) == 1.0)) >= 2, r["x"]
    r = reference_of(E, next(q for q in PROBLEMS if q["name"] == "flat"))
    assert r["passes"][0] >= 2 and all(p == (frozenset({0, 1}), frozenset({2, 3})) for p in partitions(r)[:-1])


def test_maxeval_sub2_stops_inside_the_second_subspace_of_a_pass(kernel):
    E, _ = kernel
    r = reference_of(E, next(q for q in PROBLEMS if q["name"] == "maxeval_sub2"))
    subs = r["subspaces"][0]
    assert len(subs) == 2 and subs[1][0] > 0 and subs[1][2] >= 1, subs   # the second inner search of the first pass was cut short


# searches of one n (and here a box and the stops) as ONE launch sequence from different starts, with different objectives
BATCHES = [
    dict(name="n2", n=2, lb=np.full(2, -3.0), ub=np.full(2, 3.0), kw=dict(xtol_rel=1e-6, maxeval=150),
         searches=[(rosenbrock, ROSEN_START), (steps, [0.3, 0.7]), (rosenbrock, [3.0, 3.0]), (flat, [1.0, 2.0]), (rosenbrock, [2.0, -1.5])]),
    dict(name="n7", n=7, lb=np.full(7, -2.0), ub=np.full(7, 2.0), kw=dict(xtol_rel=1e-4, maxeval=400),
         searches=[(scaled, _scaled_start(7)), (ridge, [0.9, 0.9, -0.9, 0.0, 1.0, -1.0, 0.3]), (rosenbrock, [-1.2, 1.0, 0.5, 0.2, -0.3, 0.7, 1.1])]),
    dict(name="n65", n=65, lb=np.full(65, -2.0), ub=np.full(65, 2.0), kw=dict(xtol_rel=1e-6, maxeval=150),
         searches=[(scaled, _scaled_start(65)), (rosenbrock, np.random.default_rng(3100).uniform(-1.5, 1.5, 65))]),
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
    still end at maxeval = 100, and the other four must equal their lone runs — and the reference's.  No tolerance is set: with an f
    tolerance a pass that improved nothing has fdiff_max = 0 (NaN compares false) and the outer ftol test ends the search, here as in the
    reference; that is the reference's logic, not a stop the kernel adds."""
    n, lb, ub, kw = 8, np.full(8, -2.0), np.full(8, 2.0), dict(maxeval=100)
    starts = np.random.default_rng(2950).uniform(-1.5, 1.5, (5, n))
    count = [0]

    def sick(x):
        count[0] += 1
        return rosenbrock(x) if count[0] < 10 else float("nan")
    fs = [rosenbrock, ridge, sick, rosenbrock, ridge]
    a = E.run_ext(K, n, starts, lb, ub, fs, mem=mem, **kw)
    assert a["ret"][2] == MAXEVAL_REACHED and a["nevals"][2] == 100 and count[0] == 100
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


def launcher_contract(E, K):
    E.bind(K)
    assert [K.nla_sbplx_serves(n) for n in (0, 1, 256, 257)] == [0, 1, 1, 0]
    assert [K.nla_sbplx_work_doubles(n, 1) > 0 for n in (0, 1, 256, 257)] == [False, True, True, False]
    assert [K.nla_sbplx_save_bytes(n) > 0 for n in (0, 1, 256, 257)] == [False, True, True, False]
    assert all(K.nla_sbplx_save_bytes(n) % 128 == 0 for n in (1, 5, 256))


def test_launcher_contract_on_the_cpu(kernel):
    E, K = kernel
    launcher_contract(E, K)
    n, ld, count = 4, 4, 2
    X0 = np.random.default_rng(2900).uniform(-1, 1, (count, ld))
    lb, ub = np.full(n, -2.0), np.full(n, 2.0)

    def call(n=n, ld=ld, count=count, obj=E.NLA_OBJ_EXTERNAL, work=True, ext=True, drop=None):
        rows, ns = max(count, 1), min(max(n, 1), 256)
        X, req, out = X0.copy(), np.full((rows, 2), 7, dtype=np.int32), np.full(rows * 3, -1.0)
        bufs = dict(req=req, EX=np.zeros((rows, max(ld, 1))), EF=np.zeros(rows), save=np.zeros(max(8, K.nla_sbplx_save_bytes(ns) * rows // 8)))
        e = E.Ext(*[None if drop == k else bufs[k].ctypes.data for k in ("req", "EX")], np.zeros(8).ctypes.data,
                  *[None if drop == k else bufs[k].ctypes.data for k in ("EF", "save")], 0, 0, 0, 0)
        w = np.zeros(max(8, K.nla_sbplx_work_doubles(ns, rows)))
        P = E.Params(-np.inf, 0.0, 0.0, 1e-6, 50, 0, 1.0, None, None, None, None, 0, None)
        rc = K.nla_k_sbplx_batch(obj, n, ld, count, lb.ctypes.data, ub.ctypes.data, None, X.ctypes.data, w.ctypes.data if work else None, C.byref(P),
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
