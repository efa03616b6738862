"""-m gpu: nlopt_amd_optimize_batch (include/nlopt_amd.h; csrc/batch_driver.c), the row-data device ABI (include/nlopt_amd_device.h
ABI 3; nlopt_amd_set_device_objective_row_data) and the waiting list of a coroutine step built on the device (csrc/hip/local_list.hip).

Every comparison is == on bits, result codes and counts — no tolerance anywhere:
  - search i of a batch is nlopt_optimize on the same optimiser from x_i (LD_LBFGS, LD_MMA; compiled-in, user, data-reading and host
    objectives; maximisation; exact-order sums); for LN_COBYLA: the same search run as a batch of one;
  - the chunking changes nothing;
  - a search on data row k is the ABI-2 kernel given block k alone — at the kernel level and through whole fits;
  - nla_k_local_waiting_list is the host loop's list entry for entry, and a run is the same with it and without;
  - maxeval per search, force_stop for the call, the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nlopt_amd

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SRC, CO = os.path.join(HERE, "batch", "fit_rows.hip"), os.path.join(HERE, "batch", "fit_rows.hsaco")
ZOO_SRC, ZOO_CO = os.path.join(HERE, "userobj", "zoo_extra.hip"), os.path.join(HERE, "userobj", "zoo_extra.hsaco")
LD_LBFGS, LD_MMA, LN_COBYLA = nlopt_amd.LD_LBFGS, nlopt_amd.LD_MMA, nlopt_amd.LN_COBYLA
MAXEVAL_REACHED = nlopt_amd.MAXEVAL_REACHED


def _genco(src, out):
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I",
                        os.path.join(os.path.dirname(HERE), "include"), src, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def co():
    return _genco(SRC, CO)


@pytest.fixture(scope="module")
def zoo():
    return _genco(ZOO_SRC, ZOO_CO)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def lone(o, x0):
    x, minf, ret = o.optimize_raw(x0)
    return x, minf, ret, o.get_numevals()


def assert_batch_equals(o, X0, ones, what=""):
    """the batch from the rows of X0 on optimiser o against ones[i] = (x, minf, ret, numevals) of search i run alone"""
    X, minf, res, nev = o.optimize_batch(X0)
    assert o.last_optimize_result() == nlopt_amd.SUCCESS, (what, o.get_errmsg())
    for i, (x1, f1, r1, n1) in enumerate(ones):
        assert res[i] == r1 and nev[i] == n1, (what, i, res[i], r1, nev[i], n1)
        assert np.array_equal(bits(X[i]), bits(x1)), (what, i, X[i], x1)
        assert bits(minf[i]) == bits(f1), (what, i, minf[i], f1)
    assert o.get_numevals() == sum(n for _, _, _, n in ones), what
    return X, minf, res, nev


def starts(count, n, lo, hi, seed):
    return np.random.default_rng(seed).uniform(lo, hi, (count, n))


def rosen_opt(alg, n, maximise=False, exact=None):
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(-2.0)
    o.set_upper_bounds(2.0)
    (o.set_max_objective if maximise else o.set_min_objective)(nlopt_amd.objective("rosenbrock"))
    o.set_ftol_rel(1e-9)
    o.set_maxeval(300)
    if exact is not None:
        o.set_param("amd_exact_dot", exact)
    return o


# ---- batch equals lone ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_a_batch_of_compiled_in_rosenbrock_equals_the_lone_runs(alg):
    o = rosen_opt(alg, 6)
    X0 = starts(64, 6, -1.8, 1.8, 11)
    ones = [lone(o, X0[i]) for i in range(64)]
    assert len({f for _, f, _, _ in ones}) > 2                                        # (the searches are not all alike)
    for count in (1, 2, 5, 64):
        assert_batch_equals(o, X0[:count], ones[:count], "count %d" % count)


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_one_case_under_set_max_objective_and_one_with_exact_sums(alg):
    o = rosen_opt(alg, 6, maximise=True)                                              # the maximum over the box: at a corner
    X0 = starts(5, 6, -1.8, 1.8, 12)
    X, minf, _, _ = assert_batch_equals(o, X0, [lone(o, x) for x in X0], "max")
    assert np.all(minf > 0)                                                           # the true maximum, not its negative
    o = rosen_opt(alg, 6, exact=1)
    assert_batch_equals(o, X0, [lone(o, x) for x in X0], "exact")


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_a_user_terms_objective_four_candidates_to_a_workgroup(zoo, alg):
    o = nlopt_amd.Opt(alg, 5)
    o.set_lower_bounds(-5.0)
    o.set_upper_bounds(5.0)
    assert o.set_min_device_objective(zoo, "myrastrigin") > 0, o.get_errmsg()
    o.set_ftol_rel(1e-9)
    o.set_maxeval(200)
    X0 = starts(5, 5, -4.0, 4.0, 13)
    ones = [lone(o, x) for x in X0]
    for count in (3, 4, 5):
        assert_batch_equals(o, X0[:count], ones[:count], "count %d" % count)


T64 = np.linspace(0.0, 4.0, 64)
EXP_LB, EXP_UB = np.array([0.1, 0.1, -1.0]), np.array([5.0, 5.0, 2.0])


def decay_curves(count=7, seed=2024):
    """synthetic decays a exp(-b t) + c with noise, and a start for each that is NOT the answer"""
    rng = np.random.default_rng(seed)
    a, b, c = rng.uniform(1.5, 3.5, count), rng.uniform(0.6, 2.0, count), rng.uniform(0.0, 1.0, count)
    Y = a[:, None] * np.exp(-b[:, None] * T64[None, :]) + c[:, None] + 0.01 * rng.standard_normal((count, 64))
    X0 = np.stack([rng.uniform(0.8, 1.6, count), rng.uniform(0.8, 1.4, count), rng.uniform(-0.2, 0.4, count)], axis=1)
    return Y, X0, np.stack([a, b, c], axis=1)


def exp_opt(alg, co, name):
    o = nlopt_amd.Opt(alg, 3)
    o.set_lower_bounds(EXP_LB)
    o.set_upper_bounds(EXP_UB)
    assert o.set_min_device_objective(co, name) > 0, o.get_errmsg()
    o.set_ftol_rel(1e-10)
    o.set_maxeval(400)
    return o


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_a_data_reading_objective_on_one_shared_block(co, alg):
    Y, X0, _ = decay_curves()
    o = exp_opt(alg, co, "expfit2")
    assert o.set_device_objective_data(np.concatenate([T64, Y[0]])) > 0
    X0 = np.concatenate([X0, X0[:3] * 1.1])                                          # 10 starts on one curve
    assert_batch_equals(o, X0, [lone(o, x) for x in X0], "expfit2")


def py_objective(calls):
    centre = np.array([0.7, -0.4, 1.3, 0.2])

    def f(x, g):
        calls.append(x.copy())
        if g.size:
            g[:] = 2 * (x - centre) - 1.5 * np.sin(3 * x)
        return float(np.sum((x - centre) ** 2) + 0.5 * np.sum(np.cos(3 * x)))
    return f


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_a_python_host_callback(alg):
    calls = []
    o = nlopt_amd.Opt(alg, 4)
    o.set_lower_bounds(-3.0)
    o.set_upper_bounds(4.0)
    o.set_min_objective(py_objective(calls))
    o.set_ftol_rel(1e-9)
    o.set_maxeval(150)
    X0 = np.array([[-1.5, 2.0, 0.1, -0.7], [2.5, 2.5, -2.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    ones = [lone(o, x) for x in X0]
    del calls[:]
    assert_batch_equals(o, X0, ones, "python callback")
    assert all(np.array_equal(calls[i], X0[i]) for i in range(3))                    # ascending search order within a step


# ---- COBYLA -----------------------------------------------------------------------------------------------------------------------------
def cobyla_case(o, X0, counts):
    ones = []
    for x in X0:                                                                     # each search as a batch of one
        X, minf, res, nev = o.optimize_batch(x[None, :])
        assert o.last_optimize_result() == nlopt_amd.SUCCESS and o.stats()["cobyla_host_searches"] == 0, o.get_errmsg()
        ones.append((X[0], minf[0], res[0], nev[0]))
    assert all(r > 0 for _, _, r, _ in ones), ones
    for count in counts:
        assert_batch_equals(o, X0[:count], ones[:count], "cobyla count %d" % count)
        assert o.stats()["cobyla_host_searches"] == 0


def test_cobyla_on_compiled_in_rosenbrock():
    o = rosen_opt(LN_COBYLA, 4)
    o.set_maxeval(400)
    cobyla_case(o, starts(9, 4, -1.8, 1.8, 14), (1, 3, 4, 5, 9))


def test_cobyla_on_a_user_terms_objective(zoo):
    o = nlopt_amd.Opt(LN_COBYLA, 4)
    o.set_lower_bounds(-5.0)
    o.set_upper_bounds(5.0)
    assert o.set_min_device_objective(zoo, "myrastrigin") > 0, o.get_errmsg()
    o.set_ftol_rel(1e-8)
    o.set_maxeval(300)
    cobyla_case(o, starts(9, 4, -4.0, 4.0, 15), (1, 3, 4, 5, 9))


# ---- chunking ---------------------------------------------------------------------------------------------------------------------------
def same_outputs(a, b):
    return all(np.array_equal(bits(u) if u.dtype == np.float64 else u, bits(v) if v.dtype == np.float64 else v) for u, v in zip(a, b))


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_a_forced_chunk_size_changes_nothing(co, alg):
    o = rosen_opt(alg, 6)
    X0 = starts(8, 6, -1.8, 1.8, 16)
    auto = o.optimize_batch(X0)
    o.set_param("amd_batch_chunk", 3)
    assert same_outputs(auto, o.optimize_batch(X0))
    Y, S0, _ = decay_curves(8, seed=77)                                              # row data: chunks 3 + 3 + 2 exercise row0
    o = exp_opt(alg, co, "expfit_rows")
    assert o.set_device_objective_row_data(np.concatenate([np.tile(T64, (8, 1)), Y], axis=1)) > 0, o.get_errmsg()
    auto = o.optimize_batch(S0)
    assert len({tuple(x) for x in auto[0]}) == 8                                     # eight different curves, eight different fits
    o.set_param("amd_batch_chunk", 3)
    assert same_outputs(auto, o.optimize_batch(S0))


# ---- row data, kernel level -------------------------------------------------------------------------------------------------------------
def bound(co, name, n, alg=LD_LBFGS):
    o = nlopt_amd.Opt(alg, n)
    assert o.set_min_device_objective(co, name) > 0, o.get_errmsg()
    return o


@pytest.mark.parametrize("n", [1, 3, 8])
def test_a_row_of_the_residual_kernel_is_the_abi_2_kernel_given_that_block(co, n):
    rng = np.random.default_rng(100 + n)
    m = 65                                                                           # row_bytes = 1040: not a multiple of 256
    rows = np.concatenate([rng.uniform(-1.2, 1.2, (5, m)), rng.uniform(-2.0, 2.0, (5, m))], axis=1)
    X = rng.uniform(-2.0, 2.0, (5, n))
    X[4] = X[0]                                                                      # the same point on rows 0 and 4
    r, a = bound(co, "polyfit_rows", n), bound(co, "polyfit2", n)
    assert r.set_device_objective_row_data(rows) > 0, r.get_errmsg()
    F, G = r.eval_device_objective(X, grad=True)
    assert np.array_equal(bits(F), bits(r.eval_device_objective(X)))
    for c in range(5):
        assert a.set_device_objective_data(rows[c]) > 0
        f, g = a.eval_device_objective(X[c], grad=True)
        assert bits(F[c]) == bits(f) and np.array_equal(bits(G[c]), bits(g)), (n, c, F[c], f)
    assert F[0] != F[4] and not np.array_equal(G[0], G[4])                           # different blocks, different values
    assert r.eval_device_objective(X[:3]).shape == (3,)                              # fewer points than rows is fine


@pytest.mark.parametrize("n", [1, 64, 65])
def test_a_row_of_the_terms_kernel_is_the_abi_2_kernel_given_that_block(co, n):
    rng = np.random.default_rng(200 + n)
    rows = rng.uniform(-1.0, 1.0, (5, n))                                            # the centres; n = 1: 8-byte rows 256 bytes apart
    X = rng.uniform(-2.0, 2.0, (5, n))
    X[4] = X[0]
    r, a = bound(co, "shifted_rows", n), bound(co, "shifted2", n)
    assert r.set_device_objective_row_data(rows) > 0, r.get_errmsg()
    F, G = r.eval_device_objective(X, grad=True)
    for c in range(5):
        assert a.set_device_objective_data(rows[c]) > 0
        f, g = a.eval_device_objective(X[c], grad=True)
        assert bits(F[c]) == bits(f) and np.array_equal(bits(G[c]), bits(g)), (n, c, F[c], f)
    assert F[0] != F[4]


# ---- row data, whole runs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_seven_fits_on_seven_rows_equal_seven_lone_fits(co, alg):
    Y, X0, truth = decay_curves()
    r, a = exp_opt(alg, co, "expfit_rows"), exp_opt(alg, co, "expfit2")
    assert r.set_device_objective_row_data(np.concatenate([np.tile(T64, (7, 1)), Y], axis=1)) > 0, r.get_errmsg()
    ones = []
    for k in range(7):
        assert a.set_device_objective_data(np.concatenate([T64, Y[k]])) > 0
        ones.append(lone(a, X0[k]))
    r.set_param("amd_batch_host_list", 0)                                            # the waiting lists built on the device
    X, minf, res, nev = assert_batch_equals(r, X0, ones, "expfit_rows")
    assert np.all(res > 0), res
    assert r.stats()["local_list_launches"] > 0
    if alg == LD_LBFGS:
        assert np.allclose(X, truth, atol=0.1), (X, truth)                           # the decays the curves were made from


def test_cobyla_fits_the_rows_through_batches_of_one_and_all_at_once(co):
    Y, X0, _ = decay_curves()
    r, a = exp_opt(LN_COBYLA, co, "expfit_rows"), exp_opt(LN_COBYLA, co, "expfit2")
    assert r.set_device_objective_row_data(np.concatenate([np.tile(T64, (7, 1)), Y], axis=1)) > 0, r.get_errmsg()
    ones = []
    for k in range(7):                                                               # fit k alone: the ABI-2 kernel on block k, a batch of one
        assert a.set_device_objective_data(np.concatenate([T64, Y[k]])) > 0
        X, minf, res, nev = a.optimize_batch(X0[k][None, :])
        ones.append((X[0], minf[0], res[0], nev[0]))
    _, _, res, _ = assert_batch_equals(r, X0, ones, "cobyla expfit_rows")
    assert np.all(res > 0), res


# ---- the device list --------------------------------------------------------------------------------------------------------------------
def host_list(state, want):
    """the loop of nla_local_ctx_run (local_ctx.c)"""
    return [i if (want[i] & 1) else -(i + 1) for i in range(len(state)) if state[i] == 1]


def patterns(count, rng):
    yield "none", np.zeros(count, np.int32), np.ones(count, np.int32)
    yield "all", np.ones(count, np.int32), np.ones(count, np.int32)
    yield "alternating", (np.arange(count) % 2).astype(np.int32), ((np.arange(count) // 2) % 2).astype(np.int32)
    last = np.zeros(count, np.int32)
    last[-1] = 1
    yield "last", last, np.zeros(count, np.int32)
    yield "random", rng.integers(0, 3, count).astype(np.int32), rng.integers(0, 4, count).astype(np.int32)


@pytest.mark.parametrize("count", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_the_device_list_is_the_host_loops_list(count):
    L = nlopt_amd.lib()
    rng = np.random.default_rng(300 + count)
    for name, state, want in patterns(count, rng):
        req = nlopt_amd.DevBuf.from_array(np.stack([state, want], axis=1))
        lst = nlopt_amd.DevBuf.from_array(np.full(count + 1, 0x7fffffff, np.int32))  # one guard entry behind the list
        nw = nlopt_amd.DevBuf.from_array(np.array([-7], np.int32))
        assert L.nla_k_local_waiting_list(req.ptr, count, lst.ptr, nw.ptr, None) == 0 and L.nla_stream_sync(None) == 0
        want_list = host_list(state, want)
        got = lst.to_array(np.int32, count + 1)
        assert nw.to_array(np.int32, 1)[0] == len(want_list), (count, name)
        assert list(got[:len(want_list)]) == want_list, (count, name)
        assert np.all(got[len(want_list):] == 0x7fffffff), (count, name)              # nothing written behind it
        for b in (req, lst, nw):
            b.free()


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA, LN_COBYLA])
def test_a_run_is_the_same_with_the_device_list_and_with_the_host_loop(zoo, alg):
    out = []
    for host_list_param in (0, 1):
        o = nlopt_amd.Opt(alg, 5)
        o.set_lower_bounds(-5.0)
        o.set_upper_bounds(5.0)
        assert o.set_min_device_objective(zoo, "myrastrigin") > 0, o.get_errmsg()
        o.set_ftol_rel(1e-9)
        o.set_maxeval(150)
        o.set_param("amd_batch_host_list", host_list_param)
        out.append(o.optimize_batch(starts(9, 5, -4.0, 4.0, 17)))
        n = o.stats()["local_list_launches"]
        assert (n > 0) if host_list_param == 0 else (n == 0), n
    assert same_outputs(out[0], out[1])


# ---- stops and refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_maxeval_stops_every_search_on_its_own(alg):
    o = rosen_opt(alg, 6)
    o.set_ftol_rel(0.0)
    o.set_maxeval(5)
    X0 = starts(6, 6, -1.8, 1.8, 18)
    ones = [lone(o, x) for x in X0]
    _, _, res, nev = assert_batch_equals(o, X0, ones, "maxeval")
    assert np.all(res == MAXEVAL_REACHED) and np.all(nev == 5), (res, nev)
    assert o.get_numevals() == 30


def test_force_stop_from_a_host_callback_ends_the_call():
    calls = []
    f = py_objective(calls)
    o = nlopt_amd.Opt(LD_LBFGS, 4)

    def stopping(x, g):
        v = f(x, g)
        if len(calls) == 7:
            o.force_stop()
        return v
    o.set_lower_bounds(-3.0)
    o.set_upper_bounds(4.0)
    o.set_min_objective(stopping)
    o.set_maxeval(150)
    X0 = np.array([[-1.5, 2.0, 0.1, -0.7], [2.5, 2.5, -2.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
    X, minf, res, nev = o.optimize_batch(X0)
    assert o.last_optimize_result() == nlopt_amd.FORCED_STOP
    assert np.all(res == nlopt_amd.FORCED_STOP), res
    assert len(calls) < 20 and np.all(np.isfinite(X))


def test_the_refusals_leave_x_and_the_optimiser_unchanged(co):
    L = nlopt_amd.lib()
    X0 = starts(3, 3, 0.9, 1.1, 19)

    def refused(o, X, msg, count=None):
        Xc = X.copy()
        minf, res = np.zeros(len(X)), np.zeros(len(X), np.intc)
        before = (L.nlopt_get_ftol_rel(o._h), L.nlopt_get_maxeval(o._h), L.nlopt_get_stopval(o._h), o.get_lower_bounds().tobytes())
        r = L.nlopt_amd_optimize_batch(o._h, len(X) if count is None else count, Xc.ctypes.data_as(C.POINTER(C.c_double)),
                                       minf.ctypes.data_as(C.POINTER(C.c_double)), res.ctypes.data_as(C.POINTER(C.c_int)), None)
        assert r == nlopt_amd.INVALID_ARGS and msg in o.get_errmsg(), (r, o.get_errmsg())
        assert np.array_equal(Xc, X)
        assert before == (L.nlopt_get_ftol_rel(o._h), L.nlopt_get_maxeval(o._h), L.nlopt_get_stopval(o._h), o.get_lower_bounds().tobytes())

    o = exp_opt(nlopt_amd.GN_CRS2_LM, co, "expfit2")
    refused(o, X0, "serves NLOPT_LD_LBFGS")
    o = exp_opt(LD_MMA, co, "expfit2")
    assert o.add_inequality_constraint(lambda x, g: x[0] - 10.0, 1e-8) > 0
    refused(o, X0, "nonlinear constraints")
    o = exp_opt(LD_LBFGS, co, "expfit2")
    refused(o, X0, "count == 0", count=0)
    refused(o, X0, "INT_MAX", count=2 ** 31)
    o.set_lower_bounds([0.1, 1.0, -1.0])
    o.set_upper_bounds([5.0, 1.0, 2.0])
    Xf = X0.copy()
    Xf[:, 1] = 1.0
    refused(o, Xf, "fixed coordinates is out of scope")
    o = nlopt_amd.Opt(LN_COBYLA, 4)
    o.set_min_objective(py_objective([]))
    refused(o, starts(2, 4, -1, 1, 20), "device objectives only")

    # a row-data objective: lone runs, the ABI-2 setter and more searches than rows are refused; row data on an ABI-2 objective too
    r = exp_opt(LD_LBFGS, co, "expfit_rows")
    Y, S0, _ = decay_curves(3, seed=5)
    refused(r, S0, "rows set")                                                       # no rows yet
    assert r.set_device_objective_row_data(np.concatenate([np.tile(T64, (2, 1)), Y[:2]], axis=1)) > 0
    refused(r, S0, "3 searches, 2 rows")
    _, _, ret = r.optimize_raw(S0[0])
    assert ret == nlopt_amd.INVALID_ARGS and "a row-data objective runs through nlopt_amd_optimize_batch" in r.get_errmsg()
    assert r.set_device_objective_data(np.concatenate([T64, Y[0]])) == nlopt_amd.INVALID_ARGS and "row_data" in r.get_errmsg()
    assert L.nlopt_amd_eval_device_objective(r._h, 3, S0.ctypes.data_as(C.POINTER(C.c_double)), np.zeros(3).ctypes.data_as(C.POINTER(C.c_double)),
                                             None) == nlopt_amd.INVALID_ARGS
    X, _, res, _ = r.optimize_batch(S0[:2])                                          # ... and two searches on two rows run
    assert np.all(res > 0)
    a = exp_opt(LD_LBFGS, co, "expfit2")
    assert a.set_device_objective_row_data(np.zeros((2, 128))) == nlopt_amd.INVALID_ARGS and "takes no row data" in a.get_errmsg()
