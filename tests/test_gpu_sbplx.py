"""-m gpu: NLOPT_LN_SBPLX on the device (hip/sbplx_kernels.hip over hip/nm_search.h, nldrmd_driver.c, batch_driver.c) — lone runs and batches.

Every comparison is == on bits, result codes and counts — no tolerance anywhere:
  - kernel level: nla_k_sbplx_batch(NLA_OBJ_EXTERNAL) with device buffers, evaluated from the host, on the problem and batch lists of
    tests/test_sbplx_emu.py against the REAL reference (result, count, minf, x and every requested point);
  - compiled-in objectives with exact-order sums: the lone nlopt_optimize against the real reference on the oracle's sequential twins,
    the per-evaluation f trace included;
  - default (tree) summation, user device objectives, ABI-3 row data, maximisation: search i of a batch is the lone run from x_i;
  - host callbacks through the public API against the reference; AUGLAG over an LN_SBPLX local optimiser; fixed coordinates;
  - the stops (maxeval per search, force_stop) and the refusals."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import nlopt_amd
import test_sbplx_emu as T
from test_gpu_batch import T64, assert_batch_equals, bits, decay_curves, lone, same_outputs, starts, _genco, SRC, CO, ZOO_SRC, ZOO_CO
from test_gpu_cobyla_ext import DevMem
from test_gpu_nldrmd import opt_for, refused

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")]
LN_SBPLX, LN_AUGLAG = 29, 30
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
    T.ended_by_a_small_step(a, r)
    if p["name"] == "tiny_step":
        assert a["cols"] == [1] and np.array_equal(a["x"][0], p["x0"])


@pytest.mark.parametrize("b", T.BATCHES, ids=[b["name"] for b in T.BATCHES])
def test_searches_of_one_launch_sequence_on_the_device(b):
    fs, st = [s[0] for s in b["searches"]], np.array([s[1] for s in b["searches"]], dtype=np.float64)
    a = device(b["n"], st, b["lb"], b["ub"], fs, **b["kw"])
    r = E.reference(b["n"], st, b["lb"], b["ub"], fs, **b["kw"])
    E.same(a, r)
    T.stays_finished(a)
    if b["name"] == "n2":
        assert len(set(a["finished_at"])) > 1 and a["launches"] == max(r["nevals"]) + 1


def test_a_search_whose_objective_turns_nan_ends_at_maxeval_and_disturbs_nobody():
    T.nan_among_healthy(E, nlopt_amd.lib(), mem=DevMem())


def test_launcher_helpers_of_the_library():
    T.launcher_contract(E, nlopt_amd.lib())


# ---- compiled-in objectives, exact-order sums: the lone run against the real reference ----------------------------------------------------
@pytest.mark.parametrize("obj,n,maxeval", [("rosenbrock", 2, 400), ("rosenbrock", 8, 400), ("rosenbrock", 65, 300), ("sphere", 256, 300)])
def test_a_lone_run_with_exact_sums_is_the_references_run(obj, n, maxeval):
    r = O.run_ref(LN_SBPLX, obj, n, 0, 1, maxeval=maxeval, xtol_rel=1e-8)
    o = opt_for(obj, n, exact=1, alg=LN_SBPLX, maxeval=maxeval, xtol_rel=1e-8)
    o.enable_trace(maxeval + 8)
    x, minf, ret = o.optimize_raw(O.golden_x0(obj, n)[0])
    assert ret == r["ret"] and o.get_numevals() == r["nevals"], (ret, r["ret"], o.get_numevals(), r["nevals"], o.get_errmsg())
    assert bits(minf) == bits(r["minf"]) and np.array_equal(bits(x), bits(r["x"])), (minf, r["minf"])
    t = o.trace()
    assert len(t) == len(r["fseq"]) == r["nevals"] and r["nevals"] > n + 1
    assert np.array_equal(bits(t["f"]), bits(r["fseq"]))             # f of every evaluation: the values the reference's callback saw


# ---- default summation: the trajectory may differ from the reference's; search i of a batch is the lone run --------------------------------
def test_a_chunked_batch_with_tree_sums_equals_the_lone_runs():
    o = opt_for("rosenbrock", 8, alg=LN_SBPLX, maxeval=300, xtol_rel=1e-7)
    _, lo, hi = O.golden_x0("rosenbrock", 8)
    X0 = starts(7, 8, 0.9 * lo, 0.9 * hi, 2801)
    ones = [lone(o, x) for x in X0]
    assert len({f for _, f, _, _ in ones}) > 2
    auto = assert_batch_equals(o, X0, ones, "rosenbrock")
    o.set_param("amd_batch_chunk", 3)
    assert same_outputs(auto, assert_batch_equals(o, X0, ones, "rosenbrock chunk 3"))


def test_maximisation_of_a_compiled_in_objective():
    o = opt_for("rosenbrock", 4, maximise=True, alg=LN_SBPLX, maxeval=200, xtol_rel=1e-7)
    _, lo, hi = O.golden_x0("rosenbrock", 4)
    X0 = starts(5, 4, 0.9 * lo, 0.9 * hi, 2802)
    ones = [lone(o, x) for x in X0]
    _, minf, _, _ = assert_batch_equals(o, X0, ones, "max")
    f = nlopt_amd.NLOPT_FUNC(nlopt_amd.objective("rosenbrock"))
    f0 = [f(4, np.ascontiguousarray(x).ctypes.data_as(C.POINTER(C.c_double)), None, None) for x in X0]
    assert np.all(minf > 0) and all(minf[i] > f0[i] for i in range(5))   # the true maximum, not its negative: above the start's value


# ---- host callbacks through the public API against the reference ------------------------------------------------------------------------
def test_a_python_callback_lone_and_in_a_batch_is_the_references_run():
    n, lb, ub = 7, np.full(7, -2.0), np.full(7, 2.0)
    X0 = np.random.default_rng(2803).uniform(-1.5, 1.5, (4, n))
    kw = dict(xtol_rel=1e-6, maxeval=250)
    r = E.reference(n, X0, lb, ub, T.scaled, **kw)
    a = E.reference(n, X0, lb, ub, T.scaled, R=OURS, **kw)    # the same calls on libnlopt_amd.so: four lone runs
    E.same(a, r)
    assert [m or b"" for m in a["errmsg"]] == [(m or b"").split(b":")[0] for m in r["errmsg"]]
    calls = []
    o = nlopt_amd.Opt(LN_SBPLX, n)
    o.set_lower_bounds(lb); o.set_upper_bounds(ub)
    o.set_min_objective(lambda x, g: (calls.append(x.copy()), T.scaled(x))[1])
    o.set_xtol_rel(1e-6); o.set_maxeval(250)
    assert_batch_equals(o, X0, [(r["x"][i], r["f"][i], r["ret"][i], r["nevals"][i]) for i in range(4)], "callback batch")
    assert all(np.array_equal(calls[i], X0[i]) for i in range(4))        # ascending search order within a step
    assert len(calls) == sum(r["nevals"])


def test_a_too_small_step_ends_with_xtol_reached_and_the_references_message_start():
    n, lb, ub = 2, np.full(2, -5.0), np.full(2, 5.0)
    kw = dict(dx=[1e-14, 2e-14], maxeval=50)
    r = E.reference(n, [[1.0, 2.0]], lb, ub, T.rosenbrock, **kw)
    a = E.reference(n, [[1.0, 2.0]], lb, ub, T.rosenbrock, R=OURS, **kw)
    E.same(a, r)
    assert r["ret"] == [T.XTOL_REACHED] and r["nevals"] == [1]
    # the reference's message goes on with ": %g is too close to x[%d]=%g"
    assert a["errmsg"][0] == b"starting step size led to simplex that was too small in dimension 0" and r["errmsg"][0].startswith(a["errmsg"][0] + b":")


def test_a_fixed_coordinate_is_eliminated_in_a_lone_run_and_refused_in_a_batch():
    n, lb, ub = 4, np.array([-2.0, 0.5, -2.0, -2.0]), np.array([2.0, 0.5, 2.0, 2.0])
    X0 = np.array([[-1.2, 0.5, 1.0, 0.3], [1.0, 0.5, -1.0, -0.7]])
    kw = dict(xtol_rel=1e-6, maxeval=200)
    r = E.reference(n, X0, lb, ub, T.rosenbrock, **kw)
    E.same(E.reference(n, X0, lb, ub, T.rosenbrock, R=OURS, **kw), r)
    assert all(len(p) == 4 and p[1] == 0.5 for p in r["asked"][0])
    o = nlopt_amd.Opt(LN_SBPLX, n)
    o.set_lower_bounds(lb); o.set_upper_bounds(ub)
    o.set_min_objective(lambda x, g: T.rosenbrock(x))
    refused(o, X0, "fixed coordinates is out of scope")


def test_auglag_over_a_subplex_local_optimiser_is_the_references_run():
    n, lb, ub = 2, np.full(2, -2.0), np.full(2, 2.0)

    def con(nn, x, g, d):
        return x[0] + x[1] - 1.0                                          # x0 + x1 <= 1: active at the constrained minimum
    fc = O.FUNC(con)

    def setup(R, opt):
        loc = R.nlopt_create(LN_SBPLX, n)
        R.nlopt_set_xtol_rel(loc, 1e-6); R.nlopt_set_maxeval(loc, 80)
        R.nlopt_set_local_optimizer(opt, loc)
        R.nlopt_destroy(loc)
        R.nlopt_add_inequality_constraint(opt, C.cast(fc, C.c_void_p), None, 1e-8)
        return fc
    kw = dict(xtol_rel=1e-4, maxeval=400, alg=LN_AUGLAG, setup=setup)
    r = E.NM.reference(n, [[-1.2, 1.0]], lb, ub, T.rosenbrock, **kw)
    a = E.NM.reference(n, [[-1.2, 1.0]], lb, ub, T.rosenbrock, R=OURS, **kw)
    assert r["ret"][0] > 0 and r["nevals"][0] > 40, (r["ret"], r["nevals"])      # (several sub-optimisations)
    E.same(a, r)


# ---- user device objectives and row data ------------------------------------------------------------------------------------------------
def test_a_user_terms_objective_with_the_device_list_and_the_host_loop(zoo):
    out = []
    for host_list in (0, 1):
        o = nlopt_amd.Opt(LN_SBPLX, 5)
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
    o = nlopt_amd.Opt(LN_SBPLX, n)
    o.set_lower_bounds(lb); o.set_upper_bounds(ub)
    assert o.set_min_device_objective(co, name) > 0, o.get_errmsg()
    o.set_xtol_rel(1e-8); o.set_maxeval(300)
    return o


def test_eight_fits_on_eight_rows_equal_eight_lone_fits(co):
    """tests/batch/fit_rows.hip: the exponential decay (n = 3), eight data rows: search k on row k is the lone run under the ABI-2 macro
    with block k"""
    Y, X0, _ = decay_curves(8, seed=2805)
    rows, n, lb, ub = np.concatenate([np.tile(T64, (8, 1)), Y], axis=1), 3, np.array([0.1, 0.1, -1.0]), np.array([5.0, 5.0, 2.0])
    r, a = fit_opt(co, "expfit_rows", n, lb, ub), fit_opt(co, "expfit2", n, lb, ub)
    assert r.set_device_objective_row_data(rows) > 0, r.get_errmsg()
    ones = []
    for k in range(8):
        assert a.set_device_objective_data(rows[k]) > 0
        ones.append(lone(a, X0[k]))
    assert len({f for _, f, _, _ in ones}) == 8
    r.set_param("amd_batch_host_list", 0)                                 # the waiting lists built on the device
    dev = assert_batch_equals(r, X0, ones, "expfit_rows")
    assert r.stats()["local_list_launches"] > 0
    r.set_param("amd_batch_host_list", 1)
    r.set_param("amd_batch_chunk", 3)                                     # chunks 3 + 3 + 2: each starts at its own data row
    assert same_outputs(dev, assert_batch_equals(r, X0, ones, "expfit_rows host list, chunk 3"))
    assert r.stats()["local_list_launches"] == 0


# ---- stops ------------------------------------------------------------------------------------------------------------------------------
def test_maxeval_stops_every_search_on_its_own():
    o = opt_for("rosenbrock", 6, alg=LN_SBPLX, maxeval=5)
    X0 = starts(6, 6, -1.8, 1.8, 2807)
    _, _, res, nev = assert_batch_equals(o, X0, [lone(o, x) for x in X0], "maxeval")
    assert np.all(res == nlopt_amd.MAXEVAL_REACHED) and np.all(nev == 5) and o.get_numevals() == 30


def test_force_stop_from_a_host_callback_ends_the_call_with_the_best_points():
    calls = []
    o = nlopt_amd.Opt(LN_SBPLX, 4)

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


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_the_refusals():
    o = opt_for("rosenbrock", 4, alg=LN_SBPLX, maxeval=50)
    X0 = starts(2, 4, -1.0, 1.0, 2809)
    # nonlinear constraints never reach the batch: the setter refuses them for this algorithm, as the reference's does
    assert o.add_inequality_constraint(lambda x, g: x[0] - 10.0, 1e-8) == nlopt_amd.INVALID_ARGS
    assert "invalid algorithm for constraints" in o.get_errmsg()
    assert o.add_equality_constraint(lambda x, g: x[0] - 10.0, 1e-8) == nlopt_amd.INVALID_ARGS
    o = opt_for("rosenbrock", 4, alg=LN_SBPLX, maxeval=50)
    o.set_comm(nlopt_amd.Comm.host(0, 1, lambda b: b))
    refused(o, X0, "a communicator is set")
    o = opt_for("sphere", 257, alg=LN_SBPLX, maxeval=50)
    X1 = starts(2, 257, -1.0, 1.0, 2810)
    refused(o, X1, "the device LN_SBPLX launcher serves n <= 256")
    x, _, ret = o.optimize_raw(X1[0])
    assert ret == nlopt_amd.INVALID_ARGS and "algorithm LN_SBPLX is not provided by libnlopt_amd" in o.get_errmsg() and np.array_equal(x, X1[0])
    # an algorithm the batch does not serve: the message keeps its beginning and names the new one
    o = opt_for("rosenbrock", 4, alg=34, maxeval=50)                      # NLOPT_LN_BOBYQA
    refused(o, X0, "nlopt_amd_optimize_batch serves NLOPT_LD_LBFGS, NLOPT_LD_MMA, NLOPT_LN_COBYLA, NLOPT_LN_NELDERMEAD and NLOPT_LN_SBPLX, not")
