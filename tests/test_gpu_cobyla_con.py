"""-m gpu: the coroutine COBYLA kernel with the caller's nonlinear constraint values as rows (hip/cobyla_con.hip) on the MI355X, through
libnlopt_amd.so's launcher nla_k_cobyla_batch_ext_con.  The test is the host side of the coroutine (tools/cobyla_emu_check.run_ext_con
with device buffers): launch, read req, evaluate objective and constraint blocks at every waiting row of EX in Python, write EF and the
rows of EC, launch again with resume = 1.  Oracle: the REAL reference's nlopt_optimize(LN_COBYLA) with the same Python functions —
result code, evaluation count, minf, x and the sequence of points each search asked for are the reference's bit for bit.  The cases
are those of the CPU twin (tests/test_cobyla_con_emu.py, where they are described); what this adds is the device's memory model —
slice, save record, req, EX written by one launch and read by the next, EC written between them — and n = 256 at the top of the
LDS / slice sizing."""
import numpy as np
import pytest

import _oracle as O
import nlopt_amd
from test_cobyla_con_emu import (FORCED_STOP, MAXEVAL_REACHED, MINF_MAX_REACHED, SEVEN, SHAPES, _tool, _wsq, kernel_run, problem, reference, same,
                                 stays_finished)
from test_gpu_cobyla_ext import DevMem

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")]


def device(p, starts, **kw):
    return kernel_run(_tool(), nlopt_amd.lib(), p, starts, mem=DevMem(), **kw)


@pytest.mark.parametrize("name", list(SHAPES))
def test_constrained_coroutine_kernel_on_the_device_is_the_references_search_point_by_point(name):
    s, xtol, me = SHAPES[name]
    p = problem(name)
    a = device(p, s, xtol_rel=xtol, maxeval=me)
    same(a, reference(p, s, xtol, me))
    stays_finished(a)


def test_contradictory_constraints_on_the_device():
    p = problem("clash")
    s = [[2.0, 2.0], [0.0, -1.0], [-2.5, 0.5]]
    same(device(p, s, xtol_rel=1e-4, maxeval=300), reference(p, s, 1e-4, 300))


def test_stop_value_and_the_tolerance_on_the_device():
    s = [[-1.0, -1.0], [-2.0, 0.0]]
    p = problem("nearly")
    r = reference(p, s, 1e-4, 200, stopval=0.5)
    assert r["ret"] == [MINF_MAX_REACHED] * 2
    same(device(p, s, xtol_rel=1e-4, maxeval=200, minf_max=0.5), r)
    p0 = problem("nearly", tol=0.0)
    r0 = reference(p0, s, 1e-4, 200, stopval=0.5)
    assert MINF_MAX_REACHED not in r0["ret"]
    same(device(p0, s, xtol_rel=1e-4, maxeval=200, minf_max=0.5), r0)


@pytest.mark.parametrize("maxeval", [3, 25])
def test_maxeval_on_the_device(maxeval):
    p = problem("mixed")
    a = device(p, SEVEN[:2], maxeval=maxeval)
    same(a, reference(p, SEVEN[:2], maxeval=maxeval))
    assert a["ret"] == [MAXEVAL_REACHED] * 2 and a["nevals"] == [maxeval] * 2


@pytest.mark.parametrize("k", [4, 9])
def test_forced_stop_from_the_kth_relaunch_on_the_device(k):
    """the search takes the k-th values and stops in front of evaluation k + 1: the reference forced inside call k + 1 (the CPU twin says why)"""
    p = problem("mixed")
    a = device(p, SEVEN[:3], forced_from=k)
    r = reference(p, SEVEN[:3], force_at=k + 1)
    assert a["ret"] == r["ret"] == [FORCED_STOP] * 3 and a["nevals"] == [k] * 3 and a["launches"] == k + 1
    assert np.array_equal(a["f"], r["f"]) and np.array_equal(a["x"], r["x"])
    for pa, pr in zip(a["asked"], r["asked"]):
        assert len(pa) == k and all(np.array_equal(u, v) for u, v in zip(pa, pr[:k]))


def test_seven_searches_that_end_at_different_launches_on_the_device():
    p = problem("mixed")
    r = reference(p, SEVEN, 1e-3, 120)
    a = device(p, SEVEN, xtol_rel=1e-3, maxeval=120)
    same(a, r)
    stays_finished(a)
    assert sorted(a["finished_at"]) == sorted(r["nevals"])


def test_maximisation_on_the_device():
    p = problem("tutorial")
    p["f"] = lambda x: -x[1]
    s, xtol, me = SHAPES["tutorial"]
    same(device(p, s, sign=-1.0, xtol_rel=xtol, maxeval=me), reference(p, s, xtol, me, maximise=True), sign=-1.0)


def test_top_of_the_served_range_with_two_user_rows():
    """n = 256, one block of two inequalities: mc = 2 rows in front of 512 bound rows (the LDS block saved and restored at every
    evaluation and the slice are the largest the unconstrained coroutine has, plus two rows), n + 6 evaluations: the initial simplex
    and five steps of the linear programme"""
    n = 256
    centre = [0.5 - 0.003 * i for i in range(n)]

    def g2(x):
        s = 0.0
        for v in x:
            s += v * v
        return [s - 4.0, x[0] + x[1] - 0.25]
    p = dict(n=n, lb=np.full(n, -1.0), ub=np.full(n, 1.0), f=_wsq(centre, [1.0] * n), ineq=[(2, g2, [1e-8, 0.0])], eq=[], mi=2, eq_sizes=[],
             tol=np.array([1e-8, 0.0]))
    s = [list(np.random.default_rng(4900).uniform(-0.9, 0.9, n))]
    a = device(p, s, maxeval=n + 6)
    same(a, reference(p, s, maxeval=n + 6))
    assert a["ret"] == [MAXEVAL_REACHED] and a["nevals"] == [n + 6]
