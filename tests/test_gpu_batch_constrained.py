"""-m gpu: nlopt_amd_optimize_batch with NLOPT_LN_COBYLA and NONLINEAR CONSTRAINTS from a user's device blocks (csrc/batch_driver.c,
csrc/local_ctx.c, csrc/hip/cobyla_con.hip), through nlopt_amd.Opt.  The objective family and the blocks are tests/batchcon/con_models.hip.

Every comparison is == on bits, result codes and counts.  The oracle is the lone nlopt_optimize on the SAME optimiser from x_i: the
host algorithm (cobyla_host.c, pinned to the reference evaluation by evaluation), which — no host twins are bound anywhere here —
evaluates its single points through the same kernels the batch launches over all rows.  For the ABI-3 objective: the lone run of the
same model under the ABI-2 macro with data block i."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import nlopt_amd
from test_gpu_batch import assert_batch_equals, bits, lone, same_outputs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SRC, CO = os.path.join(HERE, "batchcon", "con_models.hip"), os.path.join(HERE, "batchcon", "con_models.hsaco")
LN_COBYLA = nlopt_amd.LN_COBYLA

C5, W5 = np.array([1.0, -0.5, 0.75, 1.5, -1.0]), np.array([1.0, 2.0, 0.5, 1.5, 1.0])
STARTS5 = np.array([[0.1, 0.2, -0.3, 0.4, 0.5], [-1.5, 1.5, 1.0, -1.0, 1.9], [1.0, 1.0, 1.0, 1.0, 1.0], [0.0, 0.0, 0.0, 0.0, 0.0], [1.9, -1.9, 1.9, -1.9, 1.9],
                    [-0.4, 0.9, 0.5, 0.5, 0.5], [0.3, 0.3, 0.4, 1.0, 0.25], [-1.0, -1.0, 0.5, 1.5, -0.5], [0.6, -0.2, 1.1, -0.7, 0.9]])


@pytest.fixture(scope="module")
def co():
    if not os.path.exists(CO) or os.path.getmtime(CO) < os.path.getmtime(SRC):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I",
                        os.path.join(os.path.dirname(HERE), "include"), SRC, "-o", CO], check=True)
    return CO


def mixed(co, objective="wsq2", maximise=False, weights=W5, xtol=1e-6, maxeval=400):
    """n = 5 in [-2, 2]^5: inequality blocks prod3 (m = 3, ABI 1) and ball (m = 1, ABI 2, radius^2 = 4), the equality block heq2 (m = 2)"""
    o = nlopt_amd.Opt(LN_COBYLA, 5)
    o.set_lower_bounds(-2.0)
    o.set_upper_bounds(2.0)
    assert o.set_min_device_objective(co, objective, None, maximize=maximise) > 0, o.get_errmsg()
    if objective == "wsq2":
        assert o.set_device_objective_data(np.concatenate([C5, weights])) > 0, o.get_errmsg()
    assert o.add_inequality_device_constraints(co, "prod3", 3, tol=[1e-8, 0.0, 1e-6]) > 0, o.get_errmsg()
    assert o.add_inequality_device_constraints(co, "ball", 1, tol=1e-8, data=np.array([4.0])) > 0, o.get_errmsg()
    assert o.add_equality_device_constraints(co, "heq2", 2, tol=[1e-8, 1e-6]) > 0, o.get_errmsg()
    o.set_xtol_rel(xtol)
    o.set_maxeval(maxeval)
    return o


def test_batches_of_1_3_4_5_9_equal_the_lone_runs_abi_1_and_2_blocks_inequality_and_equality(co):
    o = mixed(co)
    ones = [lone(o, x) for x in STARTS5]
    assert all(r > 0 for _, _, r, _ in ones) and len({n for _, _, _, n in ones}) > 3, ones       # (the searches end at different steps)
    for count in (1, 3, 4, 5, 9):
        assert_batch_equals(o, STARTS5[:count], ones[:count], "count %d" % count)
        assert o.batch_constraint_launches() >= 3 and o.batch_constraint_launches() % 3 == 0      # three blocks per step
    X = o.optimize_batch(STARTS5)[0]
    for x in X:                                                      # ... and the answers satisfy what was asked for
        assert abs(x[0] + x[1] + x[2] - 1.0) < 1e-5 and abs(x[3] * x[4] - 0.25) < 1e-5 and np.sum(x * x) <= 4.0 + 1e-6
        assert all(x[j] * x[j + 1] - 0.5 * (j + 1) <= 1e-5 for j in range(3))


def test_the_tutorial_shape_one_bound_row_behind_two_cubic_blocks(co):
    """n = 2, box (-inf, inf) x [0, inf), two m = 1 ABI-2 blocks of one kernel with different data; objective wsq2 with centre (0, -1):
    it pulls x1 down onto the cubics"""
    o = nlopt_amd.Opt(LN_COBYLA, 2)
    o.set_lower_bounds([-np.inf, 0.0])
    o.set_upper_bounds([np.inf, np.inf])
    assert o.set_min_device_objective(co, "wsq2") > 0, o.get_errmsg()
    assert o.set_device_objective_data(np.array([0.0, -1.0, 0.0, 1.0])) > 0        # f = (x1 + 1)^2
    assert o.add_inequality_device_constraints(co, "cubic", 1, tol=1e-8, data=np.array([2.0, 0.0])) > 0, o.get_errmsg()
    assert o.add_inequality_device_constraints(co, "cubic", 1, tol=1e-8, data=np.array([-1.0, 1.0])) > 0, o.get_errmsg()
    o.set_xtol_rel(1e-6)
    o.set_maxeval(400)
    X0 = np.array([[1.234, 5.678], [4.0, 0.5], [-2.0, 3.0]])
    ones = [lone(o, x) for x in X0]
    X, minf, _, _ = assert_batch_equals(o, X0, ones, "tutorial")
    assert np.allclose(X, [1.0 / 3.0, 8.0 / 27.0], atol=1e-4), X


def test_seventy_cuts_and_a_band_the_wide_block_and_the_m_2_block(co):
    o = nlopt_amd.Opt(LN_COBYLA, 8)
    o.set_lower_bounds(-3.0)
    o.set_upper_bounds(3.0)
    assert o.set_min_device_objective(co, "wsq1") > 0, o.get_errmsg()
    assert o.add_inequality_device_constraints(co, "cuts70", 70, tol=1e-8) > 0, o.get_errmsg()
    assert o.add_inequality_device_constraints(co, "band2", 2, tol=0.0, data=np.array([-0.5, 0.25])) > 0, o.get_errmsg()
    o.set_xtol_rel(1e-5)
    o.set_maxeval(300)
    X0 = np.array([[0.0] * 8, [2.5, -2.5, 2.0, -2.0, 2.9, -2.9, 1.0, -1.0], [0.2, 0.1, 0.0, -0.1, -0.2, 0.3, 0.4, -0.4]])
    assert_batch_equals(o, X0, [lone(o, x) for x in X0], "cuts")


def test_a_forced_chunk_size_changes_nothing(co):
    o = mixed(co)
    auto = o.optimize_batch(STARTS5)
    o.set_param("amd_batch_chunk", 4)                                # chunks 4 + 4 + 1
    assert same_outputs(auto, o.optimize_batch(STARTS5))


def test_a_row_data_objective_with_shared_constraint_blocks_equals_the_lone_abi_2_runs_per_row(co):
    rng = np.random.default_rng(77)
    rows = np.concatenate([C5[None, :] + rng.uniform(-0.5, 0.5, (7, 5)), np.tile(W5, (7, 1))], axis=1)
    r, a = mixed(co, "wsq_rows"), mixed(co)
    assert r.set_device_objective_row_data(rows) > 0, r.get_errmsg()
    ones = []
    for k in range(7):
        assert a.set_device_objective_data(rows[k]) > 0
        ones.append(lone(a, STARTS5[k]))
    assert_batch_equals(r, STARTS5[:7], ones, "rows")
    r.set_param("amd_batch_chunk", 3)                                # chunks 3 + 3 + 1: row0
    assert_batch_equals(r, STARTS5[:7], ones, "rows, chunked")


def test_set_max_objective_flips_f_and_no_constraint(co):
    o = mixed(co, maximise=True, weights=-W5)                        # maximising -sum w (x - c)^2
    ones = [lone(o, x) for x in STARTS5[:5]]
    _, minf, _, _ = assert_batch_equals(o, STARTS5[:5], ones, "max")
    assert np.all(minf <= 0)                                         # the true maximum, not its negative
    p = mixed(co)                                                    # ... the same searches as the minimisation of +sum w (x - c)^2
    X, pminf, res, nev = p.optimize_batch(STARTS5[:5])
    assert np.array_equal(bits(X), bits(np.array([x for x, _, _, _ in ones]))) and np.array_equal(bits(pminf), bits(-minf))


def test_maxeval_stops_every_search_on_its_own(co):
    o = mixed(co, maxeval=9, xtol=0.0)
    ones = [lone(o, x) for x in STARTS5[:4]]
    _, _, res, nev = assert_batch_equals(o, STARTS5[:4], ones, "maxeval")
    assert np.all(res == nlopt_amd.MAXEVAL_REACHED) and np.all(nev == 9) and o.get_numevals() == 36


def test_force_stop_ends_the_call(co):
    """nlopt_force_stop from another thread while the batch runs (nothing on the device calls back): the call and every unfinished
    search report FORCED_STOP, with a point inside the box"""
    o = mixed(co, maxeval=400, xtol=0.0)
    done = threading.Event()

    def stopper():
        while not done.is_set():
            o.force_stop()
    t = threading.Thread(target=stopper)
    t.start()
    try:
        X, minf, res, nev = o.optimize_batch(STARTS5[:4])
    finally:
        done.set()
        t.join()
    assert o.last_optimize_result() == nlopt_amd.FORCED_STOP
    assert np.all(res == nlopt_amd.FORCED_STOP) and np.all(nev < 400), (res, nev)
    assert np.all(np.isfinite(X)) and np.all(np.abs(X) <= 2.0)


def test_the_counter_counts_constraint_launches_only(co):
    o = mixed(co, maxeval=20)
    o.optimize_batch(STARTS5[:3])
    assert o.batch_constraint_launches() == 3 * 20                   # three blocks, one step per evaluation of the longest search
    u = nlopt_amd.Opt(LN_COBYLA, 5)
    u.set_lower_bounds(-2.0)
    u.set_upper_bounds(2.0)
    assert u.set_min_device_objective(co, "wsq1") > 0
    u.set_maxeval(20)
    u.optimize_batch(STARTS5[:3])
    assert u.batch_constraint_launches() == 0
    o.optimize_batch(STARTS5[:1])                                    # (reset by every call)
    assert o.batch_constraint_launches() == 3 * 20


def test_the_refusals_leave_x_and_the_optimiser_unchanged(co):
    L = nlopt_amd.lib()
    X0 = STARTS5[:3].copy()

    def refused(o, X, msg):
        Xc = X.copy()
        minf, res = np.zeros(len(X)), np.zeros(len(X), np.intc)
        before = (L.nlopt_get_ftol_rel(o._h), L.nlopt_get_maxeval(o._h), L.nlopt_get_stopval(o._h), o.get_lower_bounds().tobytes())
        r = L.nlopt_amd_optimize_batch(o._h, len(X), Xc.ctypes.data_as(C.POINTER(C.c_double)), minf.ctypes.data_as(C.POINTER(C.c_double)),
                                       res.ctypes.data_as(C.POINTER(C.c_int)), None)
        assert r == nlopt_amd.INVALID_ARGS and msg in o.get_errmsg(), (r, o.get_errmsg())
        assert np.array_equal(Xc, X)
        assert before == (L.nlopt_get_ftol_rel(o._h), L.nlopt_get_maxeval(o._h), L.nlopt_get_stopval(o._h), o.get_lower_bounds().tobytes())

    def base(alg, n=5):
        o = nlopt_amd.Opt(alg, n)
        o.set_lower_bounds(-2.0)
        o.set_upper_bounds(2.0)
        o.set_maxeval(50)
        return o
    o = base(nlopt_amd.LD_MMA)                                       # a derivative-based algorithm with a device block
    assert o.set_min_device_objective(co, "wsq1") > 0                # (LD_LBFGS takes no constraint at all: the adder refuses, as the reference's)
    assert o.add_inequality_device_constraints(co, "ball", 1, data=np.array([4.0])) > 0, o.get_errmsg()
    refused(o, X0, "nonlinear constraints")
    o = base(nlopt_amd.LD_LBFGS)
    assert o.set_min_device_objective(co, "wsq1") > 0
    assert o.add_inequality_device_constraints(co, "ball", 1, data=np.array([4.0])) == nlopt_amd.INVALID_ARGS
    o = base(LN_COBYLA)                                              # a host callback among the constraints
    assert o.set_min_device_objective(co, "wsq1") > 0
    assert o.add_inequality_device_constraints(co, "ball", 1, data=np.array([4.0])) > 0
    assert o.add_inequality_constraint(lambda x, g: x[0] - 10.0, 1e-8) > 0
    refused(o, X0, "must be device blocks")
    o = base(LN_COBYLA)                                              # a compiled-in objective beside device blocks
    o.set_min_objective(nlopt_amd.objective("sphere"))
    assert o.add_inequality_device_constraints(co, "ball", 1, data=np.array([4.0])) > 0
    refused(o, X0, "user device objective")
    o = base(LN_COBYLA)                                              # a host objective beside device blocks
    o.set_min_objective(lambda x, g: float(np.sum(x * x)))
    assert o.add_inequality_device_constraints(co, "ball", 1, data=np.array([4.0])) > 0
    refused(o, X0, "user device objective")
    o = base(LN_COBYLA, 8)                                           # more rows than the launcher's LDS holds (n = 8: mc <= 1200)
    assert o.set_min_device_objective(co, "wsq1") > 0
    for _ in range(18):
        assert o.add_inequality_device_constraints(co, "cuts70", 70) > 0
    refused(o, np.zeros((2, 8)), "no device LN_COBYLA launcher serves n = 8 with 1260 inequality")
