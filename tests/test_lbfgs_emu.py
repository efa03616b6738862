"""CPU twin of the kernel-level part of tests/test_gpu_lbfgs.py, with the boxes that file never runs: hip/lbfgs_kernels.hip (streaming),
hip/lbfgs_resident.hip and hip/lbfgs_resident32.hip compiled by g++ over tools/simt_emu (tools/lbfgs_emu_check.py, workgroups of 64 host
threads) on CLOSED, FREE, LOWER-ONLY, UPPER-ONLY and MIXED boxes — the bound types ix = 0 / 1 / 2 of PLIS (plis.c:232-241), which a caller
who sets no bounds gets (nlopt_create: lb / ub = -/+HUGE_VAL), and everything behind them: the projection, the active set, pytrcg's
multipliers, pyrmc0's release, the step bound.

  reference order (params.exact = 3 / 1)   streaming == resident == oracle/port_lbfgs.c (pinned bit for bit to the real reference; the
        emulated device's libm is the host's): result code, evaluation count, f of EVERY evaluation, minimiser — on bits
  tree sums (params.exact = 2 / 0)          streaming == resident on bits

BOXES, CASES and problem() are what tests/test_mma_emu.py and tests/test_gpu_open_boxes.py import."""
import os
import shutil
import sys

import numpy as np
import pytest

import _oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++ here")

LB_T = 64
MAXEVAL = 300
BOXES = ("closed", "free", "lower", "upper", "mixed")
# (objective, n, history pairs; None: what the dispatcher would take, plis.c:441-445)
CASES = [("sphere", 5, None), ("rosenbrock", 10, None), ("rastrigin", 40, 5), ("ackley", 33, None), ("griewank", 64, 3), ("rastrigin", 300, 4)]
LEVY = ("levy", 17, None)          # its device gradient groups four terms differently from the host loop: resident == streaming only


def tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import lbfgs_emu_check as E
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return E


@pytest.fixture(scope="module")
def emu():
    E = tool()
    return E, E.load(LB_T)


def box(obj, n, kind):
    """the box of one kind around the objective's golden box [lo, hi] (centre c, width w).  A finite side is pulled INSIDE the region the
    starts are drawn from, so that some bounds are active from the start: lower = c + 0.05 w, upper = c - 0.05 w; a coordinate of the
    mixed box with both sides (j % 4 == 3) has [c - 0.2 w, c + 0.2 w] (the two values above would leave it no interior)."""
    _, lo, hi = O.golden_x0(obj, n)
    c, w = 0.5 * (lo + hi), hi - lo
    lb, ub = np.full(n, -np.inf), np.full(n, np.inf)
    if kind == "closed":
        lb[:], ub[:] = lo, hi
    elif kind == "lower":
        lb[:] = c + 0.05 * w
    elif kind == "upper":
        ub[:] = c - 0.05 * w
    elif kind == "mixed":
        j = np.arange(n) % 4
        lb[j == 1] = c + 0.05 * w
        ub[j == 2] = c - 0.05 * w
        lb[j == 3], ub[j == 3] = c - 0.2 * w, c + 0.2 * w
    else:
        assert kind == "free", kind
    return lb, ub


def problem(obj, n, kind, count=2):
    """(starts, lb, ub): `count` starts drawn in the golden box, then clipped into the box of `kind`"""
    _, lo, hi = O.golden_x0(obj, n)
    lb, ub = box(obj, n, kind)
    rng = np.random.default_rng(1000 * n + 10 * O.OBJ[obj] + BOXES.index(kind))
    return np.clip(rng.uniform(lo, hi, (count, n)), lb, ub), lb, ub


def history(n, mf):
    return mf or min(max(1310720 // n, 10), 400)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def identical(a, b):
    """two kernel runs are the same searches: f of every evaluation, minimiser, result, counts — on bits"""
    assert a["ret"] == b["ret"] and a["nevals"] == b["nevals"] and a["iterm"] == b["iterm"] and a["cols"] == b["cols"], (a["ret"], b["ret"], a["nevals"], b["nevals"])
    assert np.array_equal(bits(a["ftrace"]), bits(b["ftrace"]))
    assert np.array_equal(bits(a["f"]), bits(b["f"])) and np.array_equal(bits(a["x"]), bits(b["x"]))


_ORACLE = {}


def oracle(obj, n, mf, kind):
    """oracle/port_lbfgs.c from the starts of problem(): computed once, shared"""
    key = (obj, n, kind)
    if key not in _ORACLE:
        starts, lb, ub = problem(obj, n, kind)
        _ORACLE[key] = [O.run_port_lbfgs(obj, n, x0=s, ftol_rel=1e-8, maxeval=MAXEVAL, mf=mf or 0, lb=lb, ub=ub) for s in starts]
    return _ORACLE[key]


def is_the_oracles(a, orc):
    for s, p in enumerate(orc):
        assert a["ret"][s] == p["ret"] and a["nevals"][s] == p["nevals"] == len(p["fseq"]), (s, a["ret"][s], p["ret"], a["nevals"][s], p["nevals"])
        assert np.array_equal(bits(a["ftrace"][s][: p["nevals"]]), bits(p["fseq"])) and np.isnan(a["ftrace"][s][p["nevals"]:]).all(), s
        assert np.array_equal(bits(a["x"][s]), bits(p["x"])) and bits(a["f"][s]) == bits(p["minf"]), s


def test_the_boxes_are_what_they_claim():
    """every bound type of PLIS occurs, and bounds are active at the starts"""
    for obj, n, _ in CASES:
        for kind in BOXES:
            starts, lb, ub = problem(obj, n, kind)
            fl, fu = np.isfinite(lb), np.isfinite(ub)
            want = dict(closed=(True, True), free=(False, False), lower=(True, False), upper=(False, True))
            if kind == "mixed":
                assert all((fl[j], fu[j]) == ((j % 4) in (1, 3), (j % 4) in (2, 3)) for j in range(n))
            else:
                assert (fl.all(), fu.all()) == want[kind] and (fl.any(), fu.any()) == want[kind]
            assert (starts >= lb).all() and (starts <= ub).all()
            if kind not in ("free", "closed"):
                assert ((starts == lb) | (starts == ub)).any() and ((starts > lb) & (starts < ub)).any()


@pytest.mark.parametrize("kind", BOXES)
@pytest.mark.parametrize("obj,n,mf", CASES, ids=["%s%d" % c[:2] for c in CASES])
def test_reference_order_streaming_is_resident_is_the_oracle(emu, obj, n, mf, kind):
    E, L = emu
    starts, lb, ub = problem(obj, n, kind)
    m = history(n, mf)
    a = E.run(L, True, obj, n, starts, lb, ub, m, maxeval=MAXEVAL, exact=True, trace_cap=MAXEVAL + 8)
    b = E.run(L, False, obj, n, starts, lb, ub, m, maxeval=MAXEVAL, exact=True, trace_cap=MAXEVAL + 8)
    identical(a, b)
    orc = oracle(obj, n, mf, kind)
    is_the_oracles(a, orc)
    if (obj, n, kind) == ("rosenbrock", 10, "free"):
        # without a box the line search of a far start runs away: the reference gives up with NLOPT_FAILURE, and so must the kernels
        assert -1 in [p["ret"] for p in orc], [(p["ret"], p["nevals"]) for p in orc]


@pytest.mark.parametrize("kind", BOXES)
@pytest.mark.parametrize("obj,n,mf", CASES + [LEVY], ids=["%s%d" % c[:2] for c in CASES + [LEVY]])
def test_tree_sums_resident_is_streaming(emu, obj, n, mf, kind):
    E, L = emu
    starts, lb, ub = problem(obj, n, kind)
    m = history(n, mf)
    a = E.run(L, True, obj, n, starts, lb, ub, m, maxeval=MAXEVAL, trace_cap=MAXEVAL + 8)
    b = E.run(L, False, obj, n, starts, lb, ub, m, maxeval=MAXEVAL, trace_cap=MAXEVAL + 8)
    identical(a, b)
    assert max(a["nevals"]) > 1          # (sphere 5 under an upper bound of -1: a start with every coordinate on it is the minimiser)


@pytest.mark.parametrize("kind", BOXES)
def test_levy_reference_order_resident_is_streaming(emu, kind):
    E, L = emu
    obj, n, mf = LEVY
    starts, lb, ub = problem(obj, n, kind)
    a = E.run(L, True, obj, n, starts, lb, ub, history(n, mf), maxeval=MAXEVAL, exact=True, trace_cap=MAXEVAL + 8)
    b = E.run(L, False, obj, n, starts, lb, ub, history(n, mf), maxeval=MAXEVAL, exact=True, trace_cap=MAXEVAL + 8)
    identical(a, b)


@pytest.mark.parametrize("exact", [False, True], ids=["tree_sums", "reference_order"])
@pytest.mark.parametrize("obj,n,mf", [("sphere", 1100, 3), ("rastrigin", 1500, 4)])
def test_the_32_coordinates_per_thread_source_is_the_streaming_kernel(emu, obj, n, mf, exact):
    """with workgroups of 64 threads 1024 < n <= 2048 is served by hip/lbfgs_resident32.hip (4096 < n <= 8192 on the device)"""
    E, L = emu
    L.nla_lbfgs_resident_supported.argtypes = L.nla_lbfgs_resident32_supported.argtypes = [E.C.c_int, E.C.c_int, E.C.POINTER(E.Params)]
    P = E.Params(exact=1 if exact else 0)
    assert not L.nla_lbfgs_resident_supported(O.OBJ[obj], n, E.C.byref(P)) and L.nla_lbfgs_resident32_supported(O.OBJ[obj], n, E.C.byref(P))
    starts, lb, ub = problem(obj, n, "mixed")
    a = E.run(L, True, obj, n, starts, lb, ub, mf, maxeval=14, exact=exact, trace_cap=32)
    b = E.run(L, False, obj, n, starts, lb, ub, mf, maxeval=14, exact=exact, trace_cap=32)
    identical(a, b)
    assert min(a["nevals"]) > 2
    if exact:
        is_the_oracles(a, [O.run_port_lbfgs(obj, n, x0=s, ftol_rel=1e-8, maxeval=14, mf=mf, lb=lb, ub=ub) for s in starts])
