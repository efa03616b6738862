"""-m gpu: NLOPT_LD_TNEWTON, _RESTART, _PRECOND and _PRECOND_RESTART on the device (hip/tnewton_kernels.hip, tnewton_driver.c,
batch_driver.c) — lone runs and batches, against the REAL reference.

With exact-order sums (amd_exact_dot = 1; the default for a host callback) everything is == on bits: the result code, the evaluation
count, f of every evaluation (the CG probes included), minf and x — the best point SEEN inside the box, as the reference's memoize_func
returns it, not the last iterate.  Objectives with device libm inside (rastrigin, griewank) take tests/test_gpu_lbfgs.py's tolerance.
Tree-sum mode (the default for device objectives) is not bit-comparable — the finite-difference products divide by pp ~ 3e-8 / |xs| —
and is held to 10 x the deviation measured in the emulator (tools/tnewton_emu_check.py tree)."""
import ctypes as C
import os

import numpy as np
import pytest

import _oracle as O
import nlopt_amd
import test_tnewton_emu as T
from test_auglag_differential import FUNC, LD_AUGLAG, dp, vp
from test_gpu_batch import assert_batch_equals, bits, lone, same_outputs, starts, _genco
from test_lbfgs_emu import BOXES, problem

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")]
E = T.E
IDS = T.IDS
OURS = C.CDLL(nlopt_amd.LIB_PATH)                 # the NLopt C API of libnlopt_amd.so on a handle of its own (E.reference sets its argument types)
HERE = os.path.dirname(os.path.abspath(__file__))
USER_SRC, USER_CO = os.path.join(HERE, "userobj", "rosen_user.hip"), os.path.join(HERE, "userobj", "rosen_user.hsaco")


def opt_for(alg, obj, n, maximise=False, exact=1, lb=None, ub=None, **stops):
    _, lo, hi = O.golden_x0(obj, n)
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(lo if lb is None else lb)
    o.set_upper_bounds(hi if ub is None else ub)
    (o.set_max_objective if maximise else o.set_min_objective)(nlopt_amd.objective(obj))
    for k, v in stops.items():
        getattr(o, "set_" + k)(v)
    if exact is not None:
        o.set_param("amd_exact_dot", exact)
    return o


_RUN_REF = {}


def run_ref(alg, obj, n, x0=None):
    key = (alg, obj, n, None if x0 is None else bytes(np.ascontiguousarray(x0)))
    if key not in _RUN_REF:
        _RUN_REF[key] = O.run_ref(alg, obj, n, 0, 0, x0=x0)
    return _RUN_REF[key]


# ---- compiled-in objectives, exact-order sums: the lone run against the real reference ---------------------------------------------------
@pytest.mark.parametrize("obj,n", [("sphere", 5), ("rosenbrock", 10)])
@pytest.mark.parametrize("alg", IDS)
def test_a_lone_run_on_a_libm_free_objective_is_the_references_run(alg, obj, n):
    r = run_ref(alg, obj, n)
    o = opt_for(alg, obj, n)
    o.enable_trace(r["nevals"] + 8)
    x, minf, ret = o.optimize_raw(O.golden_x0(obj, n)[0])
    assert ret == r["ret"] and o.get_numevals() == r["nevals"], (ret, r["ret"], o.get_numevals(), r["nevals"], o.get_errmsg())
    t = o.trace()
    assert len(t) == len(r["fseq"]) == r["nevals"] and np.all(t["kind"] == 5)
    assert np.array_equal(bits(t["f"]), bits(r["fseq"]))             # f of every evaluation, probes included
    assert bits(minf) == bits(r["minf"]) and np.array_equal(bits(x), bits(r["x"])), (minf, r["minf"])


@pytest.mark.parametrize("obj,n", [("rastrigin", 40), ("griewank", 64)])
@pytest.mark.parametrize("alg", IDS)
def test_a_lone_run_with_device_libm_matches_the_reference(alg, obj, n):
    """tests/test_gpu_lbfgs.py::test_lbfgs_matches_oracle's convention: the code, the count within 2, minf and x to rounding"""
    r = run_ref(alg, obj, n)
    o = opt_for(alg, obj, n)
    x, minf, ret = o.optimize_raw(O.golden_x0(obj, n)[0])
    print(alg, obj, n, "ret", ret, r["ret"], "nevals", o.get_numevals(), r["nevals"], "minf", minf, r["minf"], "max |dx|", np.max(np.abs(x - r["x"])))
    assert ret == r["ret"], (ret, r["ret"], o.get_errmsg())
    assert abs(o.get_numevals() - r["nevals"]) <= 2, (o.get_numevals(), r["nevals"])
    assert abs(minf - r["minf"]) <= 1e-8 * max(abs(r["minf"]), 1e-300) + 1e-12, (minf, r["minf"])
    assert np.allclose(x, r["x"], rtol=1e-6, atol=1e-7 * max(np.abs(r["x"]).max(), 1.0))


# ---- host callbacks through the public API: the problem list of the emulated test ---------------------------------------------------------
@pytest.mark.parametrize("p,alg", T.CASES, ids=T.CASE_IDS)
def test_a_host_callback_run_is_the_references_run_point_by_point(p, alg):
    r = T.reference_of(p, alg)
    T.check_expectations(p, alg, r)
    a = E.reference(alg, p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], R=OURS, **p["kw"])
    E.same(a, r)


# ---- batches ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", IDS)
def test_a_batch_of_300_rosenbrock_searches_equals_the_lone_runs(alg):
    o = opt_for(alg, "rosenbrock", 10, maxeval=400)
    nlopt_amd.lib().nlopt_set_vector_storage(o._h, 7)     # (PRECOND ids: 7 pairs, the ring wraps; the default, 400 here, makes 300 lone runs take 6 s)
    _, lo, hi = O.golden_x0("rosenbrock", 10)
    X0 = starts(300, 10, lo, hi, 1500 + alg)
    ones = [lone(o, x) for x in X0]
    assert len({f for _, f, _, _ in ones}) > 2 and all(r > 0 for _, _, r, _ in ones)
    auto = assert_batch_equals(o, X0, ones, "300")
    _, _, _, nev = auto
    assert o.get_numevals() == int(np.sum(nev)) == sum(k for _, _, _, k in ones)
    o.set_param("amd_batch_chunk", 7)
    assert same_outputs(auto, assert_batch_equals(o, X0, ones, "chunk 7"))
    # search 0 against the reference too: the batch is not merely consistent with itself
    def seven(R, opt):
        R.nlopt_set_vector_storage.argtypes = [vp, C.c_uint]
        R.nlopt_set_vector_storage(opt, 7)
    r = O.run_ref(alg, "rosenbrock", 10, 0, 0, maxeval=400, x0=X0[0], setup=seven)
    assert r["ret"] == ones[0][2] and np.array_equal(bits(r["x"]), bits(ones[0][0])) and bits(r["minf"]) == bits(ones[0][1])


@pytest.mark.parametrize("n", [255, 256, 257])
@pytest.mark.parametrize("alg", IDS)
def test_sphere_batches_at_the_workgroups_edge_are_the_references_runs(alg, n):
    o = opt_for(alg, "sphere", n)
    _, lo, hi = O.golden_x0("sphere", n)
    X0 = starts(4, n, lo, hi, 1600 + n)
    X, minf, res, nev = o.optimize_batch(X0)
    assert o.last_optimize_result() == nlopt_amd.SUCCESS, o.get_errmsg()
    for i in range(4):
        r = run_ref(alg, "sphere", n, x0=X0[i])
        assert res[i] == r["ret"] and nev[i] == r["nevals"], (i, res[i], r["ret"], nev[i], r["nevals"])
        assert bits(minf[i]) == bits(r["minf"]) and np.array_equal(bits(X[i]), bits(r["x"])), (i, minf[i], r["minf"])


@pytest.mark.parametrize("alg", IDS)
def test_a_python_callback_batch_is_the_references_runs_best_seen_rule_included(alg):
    n, lb, ub = 5, np.full(5, -5.12), np.full(5, 5.12)
    X0 = np.random.default_rng(1700 + alg).uniform(-4.5, 4.5, (5, n))
    r = E.reference(alg, n, X0, lb, ub, E.rastr)
    assert any(not np.array_equal(r["x"][i], r["asked"][i][-1]) for i in range(5))        # (the rule decides at least one of them)
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(lb); o.set_upper_bounds(ub)

    def f(x, g):
        v, gr = E.rastr(x)
        if g.size:
            g[:] = gr
        return v
    o.set_min_objective(f)
    assert_batch_equals(o, X0, [(r["x"][i], r["f"][i], r["ret"][i], r["nevals"][i]) for i in range(5)], "callback batch")


# ---- a user device objective: the coroutine, one launch of the user's kernel per evaluation -----------------------------------------------
@pytest.mark.parametrize("host_list", [0, 1])
@pytest.mark.parametrize("alg", IDS)
def test_a_user_device_objective_gives_the_compiled_in_objectives_run(alg, host_list):
    """tree sums on both sides (n = 10: one term per lane, the same butterfly), so f, the gradient and every dot product have the same
    bits; host_list = 0: the waiting list of every step is built on the device"""
    co = _genco(USER_SRC, USER_CO)
    _, lo, hi = O.golden_x0("rosenbrock", 10)
    X0 = starts(6, 10, lo, hi, 1800)
    c = opt_for(alg, "rosenbrock", 10, exact=None, maxeval=300)
    ones = [lone(c, x) for x in X0]
    u = nlopt_amd.Opt(alg, 10)
    u.set_lower_bounds(lo); u.set_upper_bounds(hi)
    assert u.set_min_device_objective(co, "rosen_user") > 0, u.get_errmsg()
    u.set_maxeval(300)
    for i in (0, 1):
        x, minf, ret = u.optimize_raw(X0[i])
        assert ret == ones[i][2] and u.get_numevals() == ones[i][3] and bits(minf) == bits(ones[i][1]) and np.array_equal(bits(x), bits(ones[i][0]))
    u.set_param("amd_batch_host_list", host_list)
    assert_batch_equals(u, X0, ones, "user kernel")
    k = u.stats()["local_list_launches"]
    assert (k > 0) if host_list == 0 else (k == 0), k


# ---- maximisation ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", IDS)
def test_maximising_minus_f_returns_the_same_x_and_minus_minf(alg):
    n = 10
    x0, lo, hi = O.golden_x0("rosenbrock", n)
    r = E.reference(alg, n, [x0], np.full(n, lo), np.full(n, hi), E.rosen)

    def neg(x):
        f, g = E.rosen(x)
        return -f, -g
    a = E.reference(alg, n, [x0], np.full(n, lo), np.full(n, hi), neg, maximise=True, R=OURS)
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"]
    assert np.array_equal(bits(a["x"]), bits(r["x"])) and bits(a["f"][0]) == bits(-r["f"][0])
    # and on the device: the compiled-in objective negated there (set_max_objective keeps it on the device)
    o = opt_for(alg, "rosenbrock", n, maximise=True, maxeval=40)
    X0 = starts(3, n, lo, hi, 1900)
    ones = [lone(o, x) for x in X0]
    _, minf, _, _ = assert_batch_equals(o, X0, ones, "max")
    f = nlopt_amd.NLOPT_FUNC(nlopt_amd.objective("rosenbrock"))
    assert all(minf[i] >= f(n, np.ascontiguousarray(X0[i]).ctypes.data_as(C.POINTER(C.c_double)), None, None) for i in range(3))


# ---- open boxes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [k for k in BOXES if k != "closed"])
@pytest.mark.parametrize("alg", IDS)
def test_open_and_one_sided_boxes_at_n_33(alg, kind):
    n = 33
    X0, lb, ub = problem("rosenbrock", n, kind, count=1)
    r = E.reference(alg, n, X0, lb, ub, E.rosen, maxeval=120)
    a = E.reference(alg, n, X0, lb, ub, E.rosen, maxeval=120, R=OURS)
    assert r["nevals"][0] > 2
    E.same(a, r)
    # the compiled-in objective on the same box (its gradient groups its terms differently from the callback's: not comparable on bits):
    # it runs, ends with the reference's code inside the box, and a batch of one is the lone run
    o = opt_for(alg, "rosenbrock", n, lb=lb, ub=ub, maxeval=120)
    one = lone(o, X0[0])
    assert one[2] == r["ret"][0] and np.all(one[0] >= lb) and np.all(one[0] <= ub)       # (RESTART ids in the free box: FAILURE, as the reference)
    assert_batch_equals(o, X0, [one], kind)


# ---- AUGLAG over a truncated-Newton local optimiser ---------------------------------------------------------------------------------------
def test_ld_auglag_over_tnewton_precond_restart_is_the_references_run():
    """the constrained problem of tests/test_auglag_differential.py (its objective and the form of its first inequality, n = 3, the bound
    moved so that it is active); the sub-problem's objective
    is a host callback, so the local optimiser is a lone run on the coroutine"""
    n, centre = 3, np.array([0.7, -0.4, 1.3])
    lb, ub = np.full(n, -2.5), np.full(n, 3.5)

    def f(x):
        i = np.arange(n)
        return (float(np.sum((x - centre) ** 2 * (1 + 0.5 * i)) + 0.1 * np.sum(np.cos(3 * x))), 2 * (x - centre) * (1 + 0.5 * i) - 0.3 * np.sin(3 * x))

    def c(nn, x, g, d):
        xs = np.array([x[i] for i in range(nn)])
        if g:
            for i in range(nn):
                g[i] = 0.0
            g[0] += 2 * xs[0]
            g[1] += 1.0
        return float(xs[0] ** 2 + xs[1] + 0.5)                      # active at the constrained minimum
    cb = FUNC(c)

    def setup(R, opt):
        R.nlopt_set_local_optimizer.argtypes = [vp, vp]
        loc = R.nlopt_create(18, n)
        R.nlopt_set_xtol_rel(loc, 1e-6); R.nlopt_set_maxeval(loc, 60)
        R.nlopt_set_local_optimizer(opt, loc)
        R.nlopt_destroy(loc)
        R.nlopt_add_inequality_constraint(opt, C.cast(cb, vp), None, 1e-8)
        return cb
    kw = dict(xtol_rel=1e-6, maxeval=600, setup=setup)
    r = E.reference(LD_AUGLAG, n, [[1.5, 2.0, -1.0]], lb, ub, f, **kw)
    a = E.reference(LD_AUGLAG, n, [[1.5, 2.0, -1.0]], lb, ub, f, R=OURS, **kw)
    assert r["ret"][0] > 0 and r["nevals"][0] > 40, (r["ret"], r["nevals"])      # (several sub-optimisations)
    E.same(a, r)


# ---- tree-sum mode: held to 10 x the deviation measured in the emulator ------------------------------------------------------
# per problem: largest |minf - minf_ref|, largest |x - x_ref|_inf, largest ratio of evaluation counts over the four ids, measured with
# tools/tnewton_emu_check.py tree (workgroups of 64 threads)
TREE_MEASURED = {"sphere5": (0.0, 0.0, 1.0), "wquad4_65": (4.141e-21, 1.949e-11, 1.0), "rosenbrock10": (4.204e-20, 2.244e-10, 1.036)}


@pytest.mark.parametrize("alg", IDS)
@pytest.mark.parametrize("name", list(TREE_MEASURED))
def test_tree_sum_mode_stays_within_ten_times_the_measured_deviation(name, alg):
    _, fn, n, x0, lo, hi = next(p for p in E.tree_problems() if p[0] == name)
    dm, dx, ratio = TREE_MEASURED[name]
    r = E.reference(alg, n, [x0], lo, hi, fn)

    def tree(R, opt):
        R.nlopt_set_param.argtypes = [vp, C.c_char_p, C.c_double]
        R.nlopt_set_param(opt, b"amd_exact_dot", 0.0)
    a = E.reference(alg, n, [x0], lo, hi, fn, R=OURS, setup=tree)
    k = max(a["nevals"][0] / r["nevals"][0], r["nevals"][0] / a["nevals"][0])
    print(name, alg, "|dminf|", abs(a["f"][0] - r["f"][0]), "|dx|", np.max(np.abs(a["x"][0] - r["x"][0])), "ratio", k)
    assert a["ret"][0] > 0 and r["ret"][0] > 0
    assert abs(a["f"][0] - r["f"][0]) <= 10 * dm
    assert np.max(np.abs(a["x"][0] - r["x"][0])) <= 10 * dx
    assert k <= 1 + 10 * (ratio - 1)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def refused(o, X, msg):
    L = nlopt_amd.lib()
    Xc, minf, res = X.copy(), np.zeros(len(X)), np.zeros(len(X), np.intc)
    r = L.nlopt_amd_optimize_batch(o._h, len(X), Xc.ctypes.data_as(C.POINTER(C.c_double)), minf.ctypes.data_as(C.POINTER(C.c_double)),
                                   res.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert r == nlopt_amd.INVALID_ARGS and msg in o.get_errmsg(), (r, o.get_errmsg())
    assert np.array_equal(Xc, X)


@pytest.mark.parametrize("alg", IDS)
def test_the_refusals(alg):
    o = opt_for(alg, "rosenbrock", 4, maxeval=50)
    # nonlinear constraints: the setter refuses them for these algorithms, as the reference's does
    assert o.add_inequality_constraint(lambda x, g: x[0] - 10.0, 1e-8) == nlopt_amd.INVALID_ARGS
    assert "invalid algorithm for constraints" in o.get_errmsg()
    X0 = starts(2, 4, -1.0, 1.0, 2000)
    lb, ub = np.array([-2.0, 0.5, -2.0, -2.0]), np.array([2.0, 0.5, 2.0, 2.0])
    X1 = X0.copy(); X1[:, 1] = 0.5
    refused(opt_for(alg, "rosenbrock", 4, lb=lb, ub=ub, maxeval=50), X1, "fixed coordinates is out of scope")
    X2 = X0.copy(); X2[1, 2] = 1e3
    refused(opt_for(alg, "rosenbrock", 4, maxeval=50), X2, "search 1: bounds 2 fail")
    z = nlopt_amd.lib().nlopt_create(alg, 0)                             # n = 0
    try:
        one, res = np.zeros(1), np.zeros(1, np.intc)
        assert nlopt_amd.lib().nlopt_amd_optimize_batch(z, 1, one.ctypes.data_as(C.POINTER(C.c_double)), one.ctypes.data_as(C.POINTER(C.c_double)),
                                                        res.ctypes.data_as(C.POINTER(C.c_int)), None) == nlopt_amd.INVALID_ARGS
    finally:
        nlopt_amd.lib().nlopt_destroy(z)
    # a lone run with a fixed coordinate IS served (the rosen6_fixed row of the problem list runs it against the reference); on a device objective:
    x, minf, ret = opt_for(alg, "rosenbrock", 4, lb=lb, ub=ub, maxeval=50).optimize_raw(X1[0])
    assert ret > 0 and x[1] == 0.5
