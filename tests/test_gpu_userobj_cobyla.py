"""-m gpu: NLOPT_GN_MLSL / GN_MLSL_LDS with their default local optimiser (LN_COBYLA) on a USER-SUPPLIED device objective
(tests/userobj/zoo_extra.hip, bound with nlopt_amd_set_min/max_device_objective): the searches of a batch run on the device as
coroutines (hip/cobyla_ext.hip), all waiting searches evaluated by one launch of the user's kernel per step.

Every objective here is bound WITHOUT a host twin, so the host algorithm's single-point evaluations go through the same kernel (one
wavefront per point, the same sums): the oracle is the same problem with "amd_cobyla_host" = 1 — cobyla_host.c, which is pinned to
the reference evaluation by evaluation (tests/test_gpu_cobyla.py), behind the exact host-callback path.  Equality is bit for bit:
result, evaluation count, x, minf and the whole trace (kinds and f)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nlopt_amd

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "userobj", "zoo_extra.hip")
CO = os.path.join(HERE, "userobj", "zoo_extra.hsaco")
BOX = {"convexcosh": lambda n: (np.full(n, -1.0) + np.arange(n) * 0.5, np.arange(n) * 1.0 + 2.0),
       "shubert": lambda n: (np.full(n, -10.0), np.full(n, 10.0)), "myrastrigin": lambda n: (np.full(n, -5.12), np.full(n, 5.12))}


@pytest.fixture(scope="module")
def code_object():
    if not os.path.exists(CO) or os.path.getmtime(CO) < os.path.getmtime(SRC):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I",
                        os.path.join(os.path.dirname(HERE), "include"), SRC, "-o", CO], check=True)
    return CO


def run(co, alg, name, n, pop, maxeval, seed, host, maximise=False, fixed=(), local=None, stop_after=None):
    """one run; host = True: "amd_cobyla_host" = 1 (the oracle).  local = (xtol_rel, dx): an explicit LN_COBYLA local optimiser;
    stop_after = g: nlopt_force_stop from the progress hook once g iterations are done"""
    o = nlopt_amd.Opt(alg, n)
    lb, ub = BOX[name](n)
    x0 = lb + (ub - lb) * np.modf(np.arange(1, n + 1) * 0.6180339887498949)[0]
    for i in fixed:
        lb[i] = ub[i] = x0[i]
    o.set_lower_bounds(lb)
    o.set_upper_bounds(ub)
    assert o.set_min_device_objective(co, name, None, maximize=maximise) > 0, o.get_errmsg()      # no host twin
    if local:
        loc = nlopt_amd.Opt(nlopt_amd.LN_COBYLA, n)
        loc.set_xtol_rel(local[0])
        L = nlopt_amd.lib()
        L.nlopt_set_initial_step.argtypes = [C.c_void_p, C.POINTER(C.c_double)]
        dx = np.ascontiguousarray(local[1], dtype=np.float64)
        assert L.nlopt_set_initial_step(loc._h, dx.ctypes.data_as(C.POINTER(C.c_double))) > 0
        assert L.nlopt_set_local_optimizer(o._h, loc._h) > 0
    else:
        o.set_xtol_rel(1e-4)
    o.set_population(pop)
    o.set_maxeval(maxeval)
    o.enable_trace(maxeval + 64)
    if host:
        o.set_param("amd_cobyla_host", 1)
    if stop_after is not None:
        o.set_progress(lambda g, e: o.force_stop() if g >= stop_after else None)
    nlopt_amd.srand(seed)
    x, minf, ret = o.optimize_raw(x0)
    return dict(x=x, minf=minf, ret=ret, nev=o.get_numevals(), t=o.trace(), st=o.stats())


def identical(d, h):
    assert (d["ret"], d["nev"], d["minf"]) == (h["ret"], h["nev"], h["minf"]), (d["ret"], h["ret"], d["nev"], h["nev"], d["minf"], h["minf"])
    assert np.array_equal(d["x"], h["x"])
    assert len(d["t"]) == len(h["t"]) and np.array_equal(d["t"]["kind"], h["t"]["kind"]) and np.array_equal(d["t"]["f"], h["t"]["f"])


def test_gn_mlsl_runs_its_cobyla_searches_on_the_device_for_a_user_kernel(code_object):
    """myrastrigin n = 6, population 16, 2500 evaluations: the run ends by maxeval in the middle of a batch"""
    d = run(code_object, nlopt_amd.GN_MLSL, "myrastrigin", 6, 16, 2500, 5, host=False)
    h = run(code_object, nlopt_amd.GN_MLSL, "myrastrigin", 6, 16, 2500, 5, host=True)
    assert d["st"]["lbfgs_launches"] >= 1 and d["st"]["cobyla_host_searches"] == 0, d["st"]
    assert h["st"]["lbfgs_launches"] == 0, h["st"]
    assert d["ret"] == nlopt_amd.MAXEVAL_REACHED and int((d["t"]["kind"] == 4).sum()) >= 2
    identical(d, h)


def test_gn_mlsl_lds_maximising_a_user_kernel(code_object):
    """shubert n = 5 MAXIMISED (nlopt_amd_set_max_device_objective): the user's kernel applies the sign, the search must not"""
    d = run(code_object, nlopt_amd.GN_MLSL_LDS, "shubert", 5, 12, 2000, 9, host=False, maximise=True)
    h = run(code_object, nlopt_amd.GN_MLSL_LDS, "shubert", 5, 12, 2000, 9, host=True, maximise=True)
    assert d["st"]["lbfgs_launches"] >= 1 and h["st"]["lbfgs_launches"] == 0
    identical(d, h)


def test_gn_mlsl_with_an_explicit_cobyla_local_optimiser_and_initial_step(code_object):
    """convexcosh n = 4: xtol_rel and an initial step with unequal entries set on the local optimiser (nlopt_set_local_optimizer)"""
    local = (1e-3, [0.2, 0.35, 0.5, 0.3])
    d = run(code_object, nlopt_amd.GN_MLSL, "convexcosh", 4, 10, 1500, 11, host=False, local=local)
    h = run(code_object, nlopt_amd.GN_MLSL, "convexcosh", 4, 10, 1500, 11, host=True, local=local)
    assert d["st"]["lbfgs_launches"] >= 1 and h["st"]["lbfgs_launches"] == 0
    identical(d, h)


@pytest.mark.parametrize("name,n,pop,maxeval,fixed", [("myrastrigin", 4, 8, 600, (2,)), ("myrastrigin", 257, 4, 300, ())])
def test_routing_that_does_not_change(code_object, name, n, pop, maxeval, fixed):
    """a fixed coordinate (the kernel does not eliminate it) and a dimension beyond the kernel's: the host algorithm, as before"""
    d = run(code_object, nlopt_amd.GN_MLSL, name, n, pop, maxeval, 13, host=False, fixed=fixed)
    h = run(code_object, nlopt_amd.GN_MLSL, name, n, pop, maxeval, 13, host=True, fixed=fixed)
    assert d["st"]["lbfgs_launches"] == 0 and h["st"]["lbfgs_launches"] == 0
    identical(d, h)


def test_forced_stop_from_the_progress_hook(code_object):
    """nlopt_force_stop once the first iteration is done (it takes 3316 evaluations of this run, so the budget is 8000 here): FORCED_STOP,
    the best point so far is the oracle's"""
    d = run(code_object, nlopt_amd.GN_MLSL, "myrastrigin", 6, 16, 8000, 5, host=False, stop_after=1)
    h = run(code_object, nlopt_amd.GN_MLSL, "myrastrigin", 6, 16, 8000, 5, host=True, stop_after=1)
    assert d["ret"] == nlopt_amd.FORCED_STOP and d["st"]["lbfgs_launches"] >= 1
    identical(d, h)
