"""-m gpu: NLOPT_LN_NELDERMEAD on the device (hip/nldrmd_kernels.hip, nldrmd_driver.c, batch_driver.c) — lone runs and batches.

Every comparison is == on bits, result codes and counts — no tolerance anywhere:
  - kernel level: nla_k_nldrmd_batch(NLA_OBJ_EXTERNAL) with device buffers, evaluated from the host, on the problem list of
    tests/test_nldrmd_emu.py against the REAL reference (result, count, minf, x and every requested point);
  - compiled-in objectives with exact-order sums: the lone nlopt_optimize against the real reference on the oracle's sequential twins,
    the per-evaluation f trace included;
  - default (tree) summation, user device objectives, ABI-3 row data, maximisation: search i of a batch is the lone run from x_i;
  - host callbacks through the public API against the reference; AUGLAG over an LN_NELDERMEAD local optimiser; fixed coordinates;
  - the stops (maxeval per search, force_stop, maxtime) and the refusals."""
import ctypes as C
import os

import numpy as np
import pytest

import _oracle as O
import nlopt_amd
import test_nldrmd_emu as T
from test_gpu_batch import T64, assert_batch_equals, bits, decay_curves, lone, same_outputs, starts, _genco, SRC, CO, ZOO_SRC, ZOO_CO
from test_gpu_cobyla_ext import DevMem

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")]
LN_NELDERMEAD, LN_AUGLAG = nlopt_amd.LN_NELDERMEAD, 30
E = T._tool()
OURS = C.CDLL(nlopt_amd.LIB_PATH)                 # the NLopt C API of libnlopt_amd.so on a handle of its own (E.reference sets its argument types)


@pytest.fixture(scope="module")
def co():
    return _genco(SRC, CO)


@pytest.fixture(scope="module")
def zoo():
    return _genco(ZOO_SRC, ZOO_CO)


def device(n, starts_, lb, ub, f, **kw):
    return E.run_ext(nlopt_amd.lib(), n, starts_, lb, ub, f, mem=DevMem(), **kw)


# ---- kernel level: the coroutine with device buffers ------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", T.PROBLEMS, ids=[p["name"] for p in T.PROBLEMS])
def test_coroutine_kernel_on_the_device_is_the_references_search_point_by_point(p):
    r = T.reference_of(E, p)
    T.check_expectations(p, r)
    a = device(p["n"], [p["x0"]], p["lb"], p["ub"], p["f"], **p["kw"])
    E.same(a, r)
    T.stays_finished(a)
    if p["expect"] == T.FAILURE:
        assert a["cols"] == [0] and np.array_equal(a["x"][0], p["x0"])


@pytest.mark.parametrize("b", T.BATCHES, ids=[b["name"] for b in T.BATCHES])
def test_searches_of_one_launch_sequence_on_the_device(b):
    fs, st = [s[0] for s in b["searches"]], np.array([s[1] for s in b["searches"]], dtype=np.float64)
    a = device(b["n"], st, b["lb"], b["ub"], fs, **b["kw"])
    E.same(a, E.reference(b["n"], st, b["lb"], b["ub"], fs, **b["kw"]))
    T.stays_finished(a)


def test_a_search_whose_objective_turns_nan_ends_at_maxeval_and_disturbs_nobody():
    T.nan_among_healthy(E, nlopt_amd.lib(), mem=DevMem())


# ---- compiled-in objectives, exact-order sums: the lone run against the real reference ----------------------------------------------------
def opt_for(obj, n, maximise=False, exact=None, alg=LN_NELDERMEAD, **stops):
    _, lo, hi = O.golden_x0(obj, n)
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(lo)
    o.set_upper_bounds(hi)
    (o.set_max_objective if maximise else o.set_min_objective)(nlopt_amd.objective(obj))
    for k, v in stops.items():
        getattr(o, "set_" + k)(v)
    if exact is not None:
        o.set_param("amd_exact_dot", exact)
    return o


@pytest.mark.parametrize("obj,n,maxeval", [("rosenbrock", 2, 600), ("rosenbrock", 8, 600), ("rosenbrock", 65, 400), ("sphere", 256, 400)])
def test_a_lone_run_with_exact_sums_is_the_references_run(obj, n, maxeval):
    r = O.run_ref(LN_NELDERMEAD, obj, n, 0, 1, maxeval=maxeval, xtol_rel=1e-8)
    o = opt_for(obj, n, exact=1, maxeval=maxeval, xtol_rel=1e-8)
    o.enable_trace(maxeval + 8)
    x, minf, ret = o.optimize_raw(O.golden_x0(obj, n)[0])
    assert ret == r["ret"] and o.get_numevals() == r["nevals"], (ret, r["ret"], o.get_numevals(), r["nevals"], o.get_errmsg())
    assert bits(minf) == bits(r["minf"]) and np.array_equal(bits(x), bits(r["x"])), (minf, r["minf"])
    t = o.trace()
    assert len(t) == len(r["fseq"]) == r["nevals"] and np.all(t["kind"] == 5)
    assert np.array_equal(bits(t["f"]), bits(r["fseq"]))             # f of every evaluation: the values the reference's callback saw


# ---- default summation: the trajectory may differ from the reference's; search i of a batch is the lone run --------------------------------
@pytest.mark.parametrize("obj", ["rosenbrock", "griewank"])
def test_a_chunked_batch_with_tree_sums_equals_the_lone_runs(obj):
    o = opt_for(obj, 8, maxeval=300, xtol_rel=1e-7)
    _, lo, hi = O.golden_x0(obj, 8)
    X0 = starts(7, 8, 0.9 * lo, 0.9 * hi, 2801)
    ones = [lone(o, x) for x in X0]
    assert len({f for _, f, _, _ in ones}) > 2
    auto = assert_batch_equals(o, X0, ones, obj)
    o.set_param("amd_batch_chunk", 3)
    assert same_outputs(auto, assert_batch_equals(o, X0, ones, obj + " chunk 3"))


def test_maximisation_of_a_compiled_in_objective():
    o = opt_for("rosenbrock", 4, maximise=True, maxeval=200, xtol_rel=1e-7)
    _, lo, hi = O.golden_x0("rosenbrock", 4)
    X0 = starts(5, 4, 0.9 * lo, 0.9 * hi, 2802)
    ones = [lone(o, x) for x in X0]
    _, minf, _, _ = assert_batch_equals(o, X0, ones, "max")
    f = nlopt_amd.NLOPT_FUNC(nlopt_amd.objective("rosenbrock"))
    f0 = [f(4, np.ascontiguousarray(x).ctypes.data_as(C.POINTER(C.c_double)), None, None) for x in X0]
    assert np.all(minf > 0) and all(minf[i] > f0[i] for i in range(5))   # the true maximum, not its negative: above the start's value


# ---- host callbacks through the public API against the reference ------------------------------------------------------------------------
def test_a_python_callback_lone_and_in_a_batch_is_the_references_run():
    n, lb, ub = 5, np.full(5, -1.0), np.full(5, 1.0)
    X0 = np.random.default_rng(2803).uniform(-0.9, 0.9, (5, n))
    kw = dict(xtol_rel=1e-6, maxeval=250)
    r = E.reference(n, X0, lb, ub, T.wquad, **kw)
    a = E.reference(n, X0, lb, ub, T.wquad, R=OURS, **kw)     # the same calls on libnlopt_amd.so: five lone runs
    E.same(a, r)
    calls = []
    o = nlopt_amd.Opt(LN_NELDERMEAD, n)
    o.set_lower_bounds(lb); o.set_upper_bounds(ub)
    o.set_min_objective(lambda x, g: (calls.append(x.copy()), T.wquad(x))[1])
    o.set_xtol_rel(1e-6); o.set_maxeval(250)
    assert_batch_equals(o, X0, [(r["x"][i], r["f"][i], r["ret"][i], r["nevals"][i]) for i in range(5)], "callback batch")
    assert all(np.array_equal(calls[i], X0[i]) for i in range(5))        # ascending search order within a step
    assert len(calls) == sum(r["nevals"])


def test_a_fixed_coordinate_is_eliminated_in_a_lone_run_and_refused_in_a_batch():
    n, lb, ub = 3, np.array([-2.0, 0.5, -2.0]), np.array([2.0, 0.5, 2.0])
    X0 = np.array([[-1.2, 0.5, 1.0], [1.0, 0.5, -1.0]])
    kw = dict(xtol_rel=1e-6, maxeval=200)
    r = E.reference(n, X0, lb, ub, T.rosenbrock, **kw)
    E.same(E.reference(n, X0, lb, ub, T.rosenbrock, R=OURS, **kw), r)
    assert all(len(p) == 3 and p[1] == 0.5 for p in r["asked"][0])
    o = nlopt_amd.Opt(LN_NELDERMEAD, n)
    o.set_lower_bounds(lb); o.set_upper_bounds(ub)
    o.set_min_objective(lambda x, g: T.rosenbrock(x))
    refused(o, X0, "fixed coordinates is out of scope")


def test_auglag_over_a_nelder_mead_local_optimiser_is_the_references_run():
    n, lb, ub = 2, np.full(2, -2.0), np.full(2, 2.0)

    def con(nn, x, g, d):
        return x[0] + x[1] - 1.0                                          # x0 + x1 <= 1: active at the constrained minimum
    fc = O.FUNC(con)

    def setup(R, opt):
        loc = R.nlopt_create(LN_NELDERMEAD, n)
        R.nlopt_set_xtol_rel(loc, 1e-6); R.nlopt_set_maxeval(loc, 80)
        R.nlopt_set_local_optimizer(opt, loc)
        R.nlopt_destroy(loc)
        R.nlopt_add_inequality_constraint(opt, C.cast(fc, C.c_void_p), None, 1e-8)
        return fc
    kw = dict(xtol_rel=1e-4, maxeval=400, alg=LN_AUGLAG, setup=setup)
    r = E.reference(n, [[-1.2, 1.0]], lb, ub, T.rosenbrock, **kw)
    a = E.reference(n, [[-1.2, 1.0]], lb, ub, T.rosenbrock, R=OURS, **kw)
    assert r["ret"][0] > 0 and r["nevals"][0] > 40, (r["ret"], r["nevals"])      # (several sub-optimisations)
    E.same(a, r)


# ---- user device objectives and row data ------------------------------------------------------------------------------------------------
def test_a_user_terms_objective_with_the_device_list_and_the_host_loop(zoo):
    out = []
    for host_list in (0, 1):
        o = nlopt_amd.Opt(LN_NELDERMEAD, 5)
        o.set_lower_bounds(-5.0); o.set_upper_bounds(5.0)
        assert o.set_min_device_objective(zoo, "myrastrigin") > 0, o.get_errmsg()
        o.set_xtol_rel(1e-7); o.set_maxeval(200)
        X0 = starts(9, 5, -4.0, 4.0, 2804)
        ones = [lone(o, x) for x in X0]
        o.set_param("amd_batch_host_list", host_list)
        out.append(assert_batch_equals(o, X0, ones, "myrastrigin"))
        k = o.stats()["local_list_launches"]
        assert (k > 0) if host_list == 0 else (k == 0), k
    assert same_outputs(out[0], out[1])


def fit_opt(co, name, n, lb, ub):
    o = nlopt_amd.Opt(LN_NELDERMEAD, n)
    o.set_lower_bounds(lb); o.set_upper_bounds(ub)
    assert o.set_min_device_objective(co, name) > 0, o.get_errmsg()
    o.set_xtol_rel(1e-8); o.set_maxeval(300)
    return o


@pytest.mark.parametrize("model", ["expfit", "polyfit5"])
def test_eight_fits_on_eight_rows_equal_eight_lone_fits(co, model):
    """tests/batch/fit_rows.hip: the exponential decay (its n is 3) and the polynomial at n = 5, eight data rows: search k on row k is the
    lone run under the ABI-2 macro with block k"""
    if model == "expfit":
        Y, X0, _ = decay_curves(8, seed=2805)
        rows, n, lb, ub, names = np.concatenate([np.tile(T64, (8, 1)), Y], axis=1), 3, np.array([0.1, 0.1, -1.0]), np.array([5.0, 5.0, 2.0]), ("expfit_rows", "expfit2")
    else:
        rng = np.random.default_rng(2806)
        t = np.linspace(-1.0, 1.0, 33)
        coef = rng.uniform(-1.0, 1.0, (8, 5))
        Y = sum(coef[:, i:i + 1] * t[None, :] ** i for i in range(5)) + 0.01 * rng.standard_normal((8, 33))
        rows, n, lb, ub, names = np.concatenate([np.tile(t, (8, 1)), Y], axis=1), 5, np.full(5, -3.0), np.full(5, 3.0), ("polyfit_rows", "polyfit2")
        X0 = rng.uniform(-0.5, 0.5, (8, 5))
    r, a = fit_opt(co, names[0], n, lb, ub), fit_opt(co, names[1], n, lb, ub)
    assert r.set_device_objective_row_data(rows) > 0, r.get_errmsg()
    ones = []
    for k in range(8):
        assert a.set_device_objective_data(rows[k]) > 0
        ones.append(lone(a, X0[k]))
    assert len({f for _, f, _, _ in ones}) == 8
    r.set_param("amd_batch_host_list", 0)                                 # the waiting lists built on the device
    dev = assert_batch_equals(r, X0, ones, names[0])
    assert r.stats()["local_list_launches"] > 0
    r.set_param("amd_batch_host_list", 1)
    r.set_param("amd_batch_chunk", 3)                                     # chunks 3 + 3 + 2: each starts at its own data row
    assert same_outputs(dev, assert_batch_equals(r, X0, ones, names[0] + " host list, chunk 3"))
    assert r.stats()["local_list_launches"] == 0


# ---- stops ------------------------------------------------------------------------------------------------------------------------------
def test_maxeval_stops_every_search_on_its_own():
    o = opt_for("rosenbrock", 6, maxeval=5)
    X0 = starts(6, 6, -1.8, 1.8, 2807)
    _, _, res, nev = assert_batch_equals(o, X0, [lone(o, x) for x in X0], "maxeval")
    assert np.all(res == nlopt_amd.MAXEVAL_REACHED) and np.all(nev == 5) and o.get_numevals() == 30


def test_force_stop_from_a_host_callback_ends_the_call_with_the_best_points():
    calls = []
    o = nlopt_amd.Opt(LN_NELDERMEAD, 4)

    def stopping(x, g):
        calls.append(x.copy())
        if len(calls) == 17:
            o.force_stop()
        return T.ridge(x)
    o.set_lower_bounds(-3.0); o.set_upper_bounds(4.0)
    o.set_min_objective(stopping)
    o.set_maxeval(150)
    X0 = starts(3, 4, -2.0, 3.0, 2808)
    X, minf, res, nev = o.optimize_batch(X0)
    assert o.last_optimize_result() == nlopt_amd.FORCED_STOP and np.all(res == nlopt_amd.FORCED_STOP), res
    assert len(calls) == 18 and list(nev) == [6, 6, 6]                    # the step in which the flag was raised is evaluated to its end
    for i in range(3):                                                    # CHECK_EVAL meets the flag in front of the sixth value: the best of five
        assert minf[i] == min(T.ridge(c) for c in calls[i::3][:5]) == T.ridge(X[i])


def test_maxtime_raises_the_abort_flag_of_a_running_search():
    """no tolerance and a maxeval far away (a backstop): only the clock can end these searches.  The code only."""
    o = opt_for("rosenbrock", 64, maxeval=100000, maxtime=0.02)
    x0 = O.golden_x0("rosenbrock", 64)[0]
    _, _, ret = o.optimize_raw(x0)
    assert ret == nlopt_amd.MAXTIME_REACHED and 64 < o.get_numevals() < 100000, (ret, o.get_numevals())
    _, _, res, _ = o.optimize_batch(np.stack([x0, 0.5 * x0, 0.25 * x0]))
    assert o.last_optimize_result() == nlopt_amd.MAXTIME_REACHED and np.all(res == nlopt_amd.MAXTIME_REACHED), res


def test_a_starting_step_that_is_too_small_fails_with_the_references_message_start():
    o = opt_for("rosenbrock", 3)
    o._L.nlopt_set_initial_step.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
    dx = np.array([0.1, 1e-15, 0.1])
    assert o._L.nlopt_set_initial_step(o._h, dx.ctypes.data_as(C.POINTER(C.c_double))) > 0
    x0 = np.array([0.5, 1.0, -0.5])
    x, minf, ret = o.optimize_raw(x0)
    assert ret == nlopt_amd.FAILURE and o.get_numevals() == 2, (ret, o.get_numevals())
    assert o.get_errmsg() == "starting step size led to simplex that was too small in dimension 1"


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def refused(o, X, msg):
    L = nlopt_amd.lib()
    Xc, minf, res = X.copy(), np.zeros(len(X)), np.zeros(len(X), np.intc)
    r = L.nlopt_amd_optimize_batch(o._h, len(X), Xc.ctypes.data_as(C.POINTER(C.c_double)), minf.ctypes.data_as(C.POINTER(C.c_double)),
                                   res.ctypes.data_as(C.POINTER(C.c_int)), None)
    assert r == nlopt_amd.INVALID_ARGS and msg in o.get_errmsg(), (r, o.get_errmsg())
    assert np.array_equal(Xc, X)


def test_the_refusals():
    o = opt_for("rosenbrock", 4, maxeval=50)
    X0 = starts(2, 4, -1.0, 1.0, 2809)
    # nonlinear constraints never reach the batch: the setter refuses them for this algorithm, as the reference's does (options.c:
    # "invalid algorithm for constraints"), so batch_driver.c's own message for them cannot be provoked through the public interface
    assert o.add_inequality_constraint(lambda x, g: x[0] - 10.0, 1e-8) == nlopt_amd.INVALID_ARGS
    assert "invalid algorithm for constraints" in o.get_errmsg()
    assert o.add_equality_constraint(lambda x, g: x[0] - 10.0, 1e-8) == nlopt_amd.INVALID_ARGS
    o = opt_for("rosenbrock", 4, maxeval=50)
    o.set_comm(nlopt_amd.Comm.host(0, 1, lambda b: b))
    refused(o, X0, "a communicator is set")
    o = opt_for("sphere", 257, maxeval=50)
    X1 = starts(2, 257, -1.0, 1.0, 2810)
    refused(o, X1, "serves n <= 256")
    x, _, ret = o.optimize_raw(X1[0])
    assert ret == nlopt_amd.INVALID_ARGS and "is not provided by libnlopt_amd" in o.get_errmsg() and np.array_equal(x, X1[0])
