"""-m gpu: coordinates with lb[i] == ub[i].  The reference eliminates them in front of CRS2_LM / ISRES / ESCH
(elimdim, optimize.c:219-445): the algorithm runs in the reduced dimension (its default population, its RNG consumption).
Same client setup against the REAL reference and against libnlopt_amd: same result, evaluation count, minimum, argmin
(bit for bit for CRS2_LM; ISRES / ESCH go through exp / tan: to rounding)."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import nlopt_amd

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")]


def bounds_with_fixed(obj, n, fixed):
    xs, lo, hi = O.golden_x0(obj, n)
    lb, ub, x0 = np.full(n, lo), np.full(n, hi), np.array(xs)
    for i in fixed:
        lb[i] = ub[i] = x0[i]
    return lb, ub, x0


def run_ref(alg, obj, n, fixed, pop, seed, maxeval):
    lb, ub, x0 = bounds_with_fixed(obj, n, fixed)

    def setup(R, opt):
        R.nlopt_set_lower_bounds(opt, O.dptr(lb))
        R.nlopt_set_upper_bounds(opt, O.dptr(ub))
    return O.run_ref(alg, obj, n, pop, seed, maxeval=maxeval, x0=x0, setup=setup)


def run_amd(alg, obj, n, fixed, pop, seed, maxeval):
    lb, ub, x0 = bounds_with_fixed(obj, n, fixed)
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(lb)
    o.set_upper_bounds(ub)
    o.set_min_objective(nlopt_amd.objective(obj))
    if pop:
        o.set_population(pop)
    o.set_maxeval(maxeval)
    o.enable_trace(maxeval + 64)
    nlopt_amd.srand(seed)
    x, minf, ret = o.optimize_raw(x0)
    return dict(ret=ret, minf=minf, x=x, nevals=o.get_numevals(), f=o.trace()["f"], err=o.get_errmsg())


@pytest.mark.parametrize("fixed,pop", [([0], 0), ([2, 5, 6], 40), ([0, 1, 2, 3, 4, 5, 7], 0)])
def test_crs_with_fixed_coordinates(fixed, pop):
    a = run_amd(nlopt_amd.GN_CRS2_LM, "rastrigin", 8, fixed, pop, 42, 1500)
    r = run_ref(19, "rastrigin", 8, fixed, pop, 42, 1500)
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"], a["err"]
    assert np.array_equal(a["f"], r["fseq"]) and a["minf"] == r["minf"] and np.array_equal(a["x"], r["x"])
    lb, ub, x0 = bounds_with_fixed("rastrigin", 8, fixed)
    assert all(a["x"][i] == x0[i] for i in fixed)


@pytest.mark.parametrize("alg,refalg", [(nlopt_amd.GN_ISRES, 35), (nlopt_amd.GN_ESCH, 42)])
def test_isres_esch_with_fixed_coordinates(alg, refalg):
    a = run_amd(alg, "griewank", 7, [1, 4], 30, 5, 900)
    r = run_ref(refalg, "griewank", 7, [1, 4], 30, 5, 900)
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"], a["err"]
    assert np.allclose(a["f"], r["fseq"], rtol=1e-9, atol=0) and abs(a["minf"] - r["minf"]) <= 1e-9 * abs(r["minf"])
    assert np.allclose(a["x"], r["x"], rtol=1e-9, atol=1e-9)


def test_all_coordinates_fixed():
    """n0 = 0 after elimination: the objective is evaluated once at the only point (optimize.c:536-539)"""
    a = run_amd(nlopt_amd.GN_CRS2_LM, "sphere", 3, [0, 1, 2], 0, 1, 100)
    r = run_ref(19, "sphere", 3, [0, 1, 2], 0, 1, 100)
    assert a["ret"] == r["ret"] == 1 and a["minf"] == r["minf"] and np.array_equal(a["x"], r["x"])


# ---- MLSL and its local optimisers with lb[i] == ub[i] -----------------------------------------------------------------------------
# MLSL itself does not eliminate a fixed coordinate (mlsl.c is not in elimdim_wrapcheck): R_prefactor *= pow(ub - lb, 1/n) is 0
# (mlsl.c:315-317), so R = 0 and every distance test of is_potential_minimizer (mlsl.c:197-218) compares against an exact zero — nearly
# every ranked point starts a search; the bound test skips the fixed coordinate.  Its local optimiser sees the fixed coordinate as the
# reference's would: LN_COBYLA eliminates it per search (nlopt_optimize_limited -> elimdim), LD_LBFGS keeps it as PLIS bound type 5
# (plis.c:232-241), LD_MMA with sigma = 0 there.

import test_cobyla_differential as T          # noqa: E402
from test_gpu_cobyla import run_gn_mlsl          # noqa: E402
from test_gpu_exact_local import recorder, run_amd as run_local_amd          # noqa: E402


def fixed_box(obj, n, fixed, x0=None):
    """the objective's box, coordinates `fixed` pinned at the start point's value; the start point inside"""
    lo, hi = nlopt_amd.objective_box(obj)
    lb, ub = np.full(n, float(lo)), np.full(n, float(hi))
    x0 = np.linspace(0.3 * lo, 0.4 * hi, n) if x0 is None else np.array(x0, dtype=np.float64)
    for i in fixed:
        lb[i] = ub[i] = x0[i]
    return lb, ub, x0


GN_MODES = {"device-batches": [("amd_cobyla_min_batch", 1)], "default": [], "cobyla-host": [("amd_cobyla_host", 1)]}


@pytest.mark.parametrize("mode", list(GN_MODES))
@pytest.mark.parametrize("fixed", [[2], [0, 3, 5], [0, 1, 2, 3, 5]], ids=["one", "several", "all-but-one"])
@pytest.mark.parametrize("alg", [T.GN_MLSL, T.GN_MLSL_LDS], ids=["GN_MLSL", "GN_MLSL_LDS"])
def test_gn_mlsl_default_cobyla_with_fixed_coordinates_is_the_references_run(alg, fixed, mode):
    """GN_MLSL(_LDS), default LN_COBYLA, a compiled-in objective and a fixed coordinate: the batched device COBYLA does not eliminate
    it (it refuses such a box), so the searches run through the host algorithm, whose nlopt_optimize eliminates it per search like
    the reference's nlopt_optimize_limited.  That host path sums the objective in the reference's order: result, evaluation count,
    minimum and minimiser bit for bit in every mode — also with amd_cobyla_min_batch = 1, where a box without a fixed coordinate
    launches every batch on the device (the test below) — and no device COBYLA launch at all"""
    lb, ub, x0 = fixed_box("rosenbrock", 6, fixed)
    r = run_gn_mlsl(T.more_bind(O.ref()), alg, "rosenbrock", 6, 2500, lb=lb, ub=ub, x0=x0)
    a = run_gn_mlsl(T.more_bind(C.CDLL(nlopt_amd.LIB_PATH)), alg, "rosenbrock", 6, 2500, params=GN_MODES[mode], stats=True, lb=lb, ub=ub, x0=x0)
    assert r["ret"] > 0, r
    assert (a["ret"], a["nevals"]) == (r["ret"], r["nevals"]), (a, r)
    assert a["minf"] == r["minf"] and np.array_equal(a["x"], r["x"]), (a, r)
    assert all(a["x"][i] == lb[i] for i in fixed)
    assert a["launches"] == 0, a


@pytest.mark.parametrize("alg", [T.GN_MLSL, T.GN_MLSL_LDS], ids=["GN_MLSL", "GN_MLSL_LDS"])
def test_gn_mlsl_without_a_fixed_coordinate_keeps_the_device_cobyla(alg):
    """the other side of the routing above: the same problem with every coordinate free, amd_cobyla_min_batch = 1, exact order — every
    batch on the device, still the reference's run"""
    _, _, x0 = fixed_box("rosenbrock", 6, [])
    r = run_gn_mlsl(T.more_bind(O.ref()), alg, "rosenbrock", 6, 2500, x0=x0)
    a = run_gn_mlsl(T.more_bind(C.CDLL(nlopt_amd.LIB_PATH)), alg, "rosenbrock", 6, 2500, params=[("amd_exact_dot", 1), ("amd_cobyla_min_batch", 1)],
                    stats=True, x0=x0)
    assert (a["ret"], a["nevals"], a["minf"]) == (r["ret"], r["nevals"], r["minf"]) and np.array_equal(a["x"], r["x"]), (a, r)
    assert a["launches"] > 0 and a["host_searches"] == 0, a


def test_gn_mlsl_maximisation_with_a_fixed_coordinate():
    """nlopt_set_max_objective with a compiled-in objective (the dispatcher leaves the sign to the device, dev_sign): with a fixed
    coordinate the host COBYLA takes the searches and flips the sign itself — the reference's maximisation bit for bit"""
    lb, ub, x0 = fixed_box("sphere", 4, [1])
    for params in ([("amd_cobyla_min_batch", 1)], []):
        r = run_gn_mlsl(T.more_bind(O.ref()), T.GN_MLSL_LDS, "sphere", 4, 1200, lb=lb, ub=ub, x0=x0, maximise=True)
        a = run_gn_mlsl(T.more_bind(C.CDLL(nlopt_amd.LIB_PATH)), T.GN_MLSL_LDS, "sphere", 4, 1200, params=params, stats=True, lb=lb, ub=ub, x0=x0,
                        maximise=True)
        assert (a["ret"], a["nevals"], a["minf"]) == (r["ret"], r["nevals"], r["minf"]) and np.array_equal(a["x"], r["x"]), (a, r)
        assert a["x"][1] == lb[1] and a["launches"] == 0


def ref_mlsl(alg, local, obj, lb, ub, x0, ns, seed, maxeval, maximise=False, local_ftol_rel=1e-8):
    """the REAL reference: alg (G_MLSL / G_MLSL_LDS with LD_LBFGS / LD_MMA, or GD_MLSL with the dispatcher's default local optimiser,
    local = None) on the box lb / ub, every call through the oracle's recording callback"""
    n = len(lb)

    def setup(R, opt):
        R.nlopt_set_lower_bounds(opt, O.dptr(lb))
        R.nlopt_set_upper_bounds(opt, O.dptr(ub))
        if maximise:
            R.nlopt_set_max_objective(opt, O.port().orc_objective(O.OBJ[obj]), None)
        if local is None:
            R.nlopt_set_ftol_rel(opt, local_ftol_rel)
            return
        loc = R.nlopt_create(local, n)
        R.nlopt_set_ftol_rel(loc, local_ftol_rel)
        assert R.nlopt_set_local_optimizer(opt, loc) > 0
        R.nlopt_destroy(loc)
    return O.run_ref(alg, obj, n, ns, seed, maxeval=maxeval, x0=x0, setup=setup)


def amd_mlsl(alg, local, obj, lb, ub, x0, ns, seed, maxeval, host, exact, maximise=False, local_ftol_rel=1e-8):
    n = len(lb)
    L = nlopt_amd.lib()
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(lb)
    o.set_upper_bounds(ub)
    rec = None
    if host:
        rec, fbuf, hbuf, cb = recorder(obj, 2 * maxeval + 8192)
        o.set_min_objective(cb, C.cast(C.pointer(rec), C.c_void_p))
    elif maximise:
        o.set_max_objective(nlopt_amd.objective(obj))
    else:
        o.set_min_objective(nlopt_amd.objective(obj))
    if local is None:
        o.set_ftol_rel(local_ftol_rel)
    else:
        loc = nlopt_amd.Opt(local, n)
        loc.set_ftol_rel(local_ftol_rel)
        assert L.nlopt_set_local_optimizer(o._h, loc._h) > 0
    if ns:
        o.set_population(ns)
    o.set_maxeval(maxeval)
    if exact:
        o.set_param("amd_exact_dot", 1)
    nlopt_amd.srand(seed)
    x, minf, ret = o.optimize_raw(x0)
    out = dict(ret=ret, minf=minf, x=x, nevals=o.get_numevals(), err=o.get_errmsg(), stats=o.stats())
    if host:
        out["fseq"], out["xhash"] = fbuf[:rec.len].copy(), hbuf[:rec.len].copy()
    return out


#          alg, local optimiser, objective, n, fixed, population, seed, maxeval
MLSL_CASES = [(nlopt_amd.G_MLSL, nlopt_amd.LD_LBFGS, "sphere", 5, [1], 20, 3, 3000),
              (nlopt_amd.G_MLSL_LDS, nlopt_amd.LD_LBFGS, "rosenbrock", 4, [0, 2], 12, 9, 4000),
              (nlopt_amd.G_MLSL, nlopt_amd.LD_MMA, "sphere", 6, [0, 2, 3, 4, 5], 10, 5, 2500),
              (nlopt_amd.G_MLSL_LDS, nlopt_amd.LD_MMA, "rosenbrock", 3, [1], 8, 2, 3000),
              (nlopt_amd.GD_MLSL, None, "sphere", 4, [3], 10, 7, 2000),
              # R = 0 with 1200 samples: the first iteration ranks 361 points, all qualify — two batches of searches (320 + the rest),
              # maxeval binding inside the second
              (nlopt_amd.G_MLSL, nlopt_amd.LD_LBFGS, "sphere", 4, [3], 1200, 4, 2200)]
MLSL_IDS = ["mlsl-lbfgs-sphere", "lds-lbfgs-rosenbrock", "mlsl-mma-all-but-one", "lds-mma-rosenbrock", "gd-mlsl-default", "mlsl-two-batches"]


@pytest.mark.parametrize("mode", ["host-callback", "device-exact", "device-default"])
@pytest.mark.parametrize("alg,local,obj,n,fixed,ns,seed,maxeval", MLSL_CASES, ids=MLSL_IDS)
def test_mlsl_with_fixed_coordinates_is_the_references_run(alg, local, obj, n, fixed, ns, seed, maxeval, mode):
    """G_MLSL(_LDS) + LD_LBFGS / LD_MMA and GD_MLSL (default LD_MMA) in MLSL's R = 0 regime, against the REAL reference.
    Host callback: every call bit for bit.  Device objective, exact order (sphere / Rosenbrock: no transcendental): the result code and
    the evaluation count exactly, the minimum and the minimiser at the slack of test_gpu_exact_local.py's MLSL test.  Default (tree-sum)
    mode: at the slack of test_gpu_mlsl.py.  Every fixed coordinate of the minimiser is its bound exactly."""
    lb, ub, x0 = fixed_box(obj, n, fixed, O.golden_x0(obj, n)[0])
    r = ref_mlsl(alg, local, obj, lb, ub, x0, ns, seed, maxeval)
    a = amd_mlsl(alg, local, obj, lb, ub, x0, ns, seed, maxeval, host=mode == "host-callback", exact=mode != "device-default")
    assert all(a["x"][i] == lb[i] for i in fixed), a["x"]
    assert a["ret"] == r["ret"], (a["ret"], r["ret"], a["err"])
    if mode == "host-callback":
        assert a["nevals"] == r["nevals"] and np.array_equal(a["xhash"], r["xhash"]) and np.array_equal(a["fseq"], r["fseq"])
        assert a["minf"] == r["minf"] and np.array_equal(a["x"], r["x"])
        return
    if mode == "device-exact":
        assert a["nevals"] == r["nevals"], (a["nevals"], r["nevals"])
        assert abs(a["minf"] - r["minf"]) <= 1e-8 * max(abs(r["minf"]), 1.0)
        assert np.allclose(a["x"], r["x"], rtol=1e-6, atol=1e-7 * max(np.abs(r["x"]).max(), 1.0))
    else:
        assert abs(a["minf"] - r["minf"]) <= 1e-7 * max(abs(r["minf"]), 1.0)
        assert np.allclose(a["x"], r["x"], rtol=1e-5, atol=1e-6 * max(np.abs(r["x"]).max(), 1.0))


def test_mlsl_start_point_at_the_minimiser_with_a_fixed_coordinate():
    """a sample point that coincides with a minimiser, R = 0: sphere on a symmetric box, the fixed coordinate at 0 and the start point
    (MLSL's first sample, mlsl.c:330-334) at the origin — the minimiser itself.  It ranks first and starts the first search, which
    returns its own point; every later sample has a larger f.  closest_lm_d == 0 cannot decide a disqualification here, nor anywhere:
    a local minimum is compared only with points of strictly larger f (mlsl.c:147-157,178-193), a point at the minimum's own x has the
    same f, and two points of different f lie at a squared distance that underflows to 0 only below 1e-154 — not a point a sampler
    produces.  What is pinned: the reference's run, call by call, Sobol samples and pseudo-random ones"""
    n = 4
    lb, ub = np.full(n, -3.0), np.full(n, 3.0)
    lb[2] = ub[2] = 0.0
    for alg in (nlopt_amd.G_MLSL_LDS, nlopt_amd.G_MLSL):
        r = ref_mlsl(alg, nlopt_amd.LD_LBFGS, "sphere", lb, ub, np.zeros(n), 16, 1, 1500)
        a = amd_mlsl(alg, nlopt_amd.LD_LBFGS, "sphere", lb, ub, np.zeros(n), 16, 1, 1500, host=True, exact=True)
        assert (a["ret"], a["nevals"], a["minf"]) == (r["ret"], r["nevals"], r["minf"]) and np.array_equal(a["x"], r["x"])
        assert np.array_equal(a["xhash"], r["xhash"]) and np.array_equal(a["fseq"], r["fseq"])
        assert r["minf"] == 0.0 and not np.any(r["x"])


def test_mlsl_maximisation_with_a_fixed_coordinate_keeps_the_device_objective():
    """G_MLSL + LD_LBFGS maximising a compiled-in objective (the dev_sign path: f and gradient negated on the device) with a fixed
    coordinate, exact order, against the reference's maximisation"""
    lb, ub, x0 = fixed_box("sphere", 5, [0, 3], O.golden_x0("sphere", 5)[0])
    r = ref_mlsl(nlopt_amd.G_MLSL, nlopt_amd.LD_LBFGS, "sphere", lb, ub, x0, 10, 6, 1500, maximise=True)
    a = amd_mlsl(nlopt_amd.G_MLSL, nlopt_amd.LD_LBFGS, "sphere", lb, ub, x0, 10, 6, 1500, host=False, exact=True, maximise=True)
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"], (a, r["ret"], r["nevals"])
    assert abs(a["minf"] - r["minf"]) <= 1e-8 * max(abs(r["minf"]), 1.0) and np.allclose(a["x"], r["x"], rtol=1e-6, atol=1e-7)
    assert a["x"][0] == lb[0] and a["x"][3] == lb[3]


# ---- standalone LD_LBFGS / LD_MMA --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "tree"])
@pytest.mark.parametrize("n", [1000, 6000, 9000], ids=["resident", "resident32", "streaming"])
def test_lbfgs_with_fixed_coordinates_on_each_kernel(n, exact):
    """LD_LBFGS keeps a fixed coordinate as PLIS bound type 5 (plis.c:232-241,463-469): on the resident kernel (n <= 4096),
    lbfgs_resident32 (4097-8192) and the streaming kernel (above), fixed coordinates — one next to a coordinate that starts on its
    bound, others spread — against the REAL reference.  Exact order (Rosenbrock, 120 evaluations): the evaluation count and result
    exactly, f of every evaluation within 1e-10.  Tree sums follow the reference only to rounding, which a long descent cut by maxeval
    amplifies (measured: 6e-8 relative after 120 evaluations of Rosenbrock at n = 1000), so there the problem is one that converges —
    a sphere whose box keeps coordinate 4 on its lower bound: the result code and the minimum within 1e-10"""
    obj = "rosenbrock" if exact else "sphere"
    lo, hi = nlopt_amd.objective_box(obj)
    x0 = np.array(O.golden_x0(obj, n)[0], dtype=np.float64)
    lb, ub = np.full(n, float(lo)), np.full(n, float(hi))
    if exact:
        x0[4] = hi                                              # an active bound ...
    else:
        lb[4] = x0[4] = 0.5 * hi                                # (the minimiser's coordinate 4 is this bound)
    for i in (5, n // 3, n - 1):                                # ... with a fixed coordinate beside it
        lb[i] = ub[i] = x0[i]
    kw = dict(maxeval=120 if exact else 400, ftol_rel=1e-12)
    r = O.run_ref_lbfgs(obj, n, x0=x0, lb=lb, ub=ub, **kw)
    a = run_local_amd(nlopt_amd.LD_LBFGS, obj, n, False, x0=x0, lb=lb, ub=ub, exact=exact, **kw)
    assert all(a["x"][i] == lb[i] for i in (5, n // 3, n - 1))
    assert a["ret"] == r["ret"], (a["ret"], r["ret"], a["err"])
    if exact:
        assert a["nevals"] == r["nevals"] and len(a["fseq"]) == len(r["fseq"])
        assert np.all(np.abs(a["fseq"] - r["fseq"]) <= 1e-10 * np.abs(r["fseq"]))
    else:
        assert r["ret"] in (nlopt_amd.SUCCESS, nlopt_amd.FTOL_REACHED, nlopt_amd.XTOL_REACHED) and a["x"][4] == lb[4] == r["x"][4], (r["ret"], a["x"][4])
    assert abs(a["minf"] - r["minf"]) <= 1e-10 * abs(r["minf"])


def test_lbfgs_with_fixed_coordinates_host_callback_is_the_references_run():
    """the same with a host callback (the oracle's C objective): every call bit for bit"""
    obj, n = "rosenbrock", 40
    lo, hi = nlopt_amd.objective_box(obj)
    x0 = np.array(O.golden_x0(obj, n)[0], dtype=np.float64)
    lb, ub = np.full(n, float(lo)), np.full(n, float(hi))
    x0[4] = lo
    for i in (3, 5, 20):
        lb[i] = ub[i] = x0[i]
    r = O.run_ref_lbfgs(obj, n, x0=x0, lb=lb, ub=ub, maxeval=400)
    a = run_local_amd(nlopt_amd.LD_LBFGS, obj, n, True, x0=x0, lb=lb, ub=ub, maxeval=400)
    assert (a["ret"], a["nevals"], a["minf"]) == (r["ret"], r["nevals"], r["minf"]) and np.array_equal(a["x"], r["x"])
    assert np.array_equal(a["xhash"], r["xhash"]) and np.array_equal(a["fseq"], r["fseq"])


@pytest.mark.parametrize("step", [None, 0.3])
def test_mma_with_fixed_coordinates_exact_order(step):
    """LD_MMA with several fixed coordinates (sigma = 0 there), exact order, default and given initial step (sigma_init: the path MLSL
    passes its local optimiser's step through), against the REAL reference: result, evaluation count, every f within 1e-10"""
    obj, n = "rosenbrock", 9
    lo, hi = nlopt_amd.objective_box(obj)
    x0 = np.array(O.golden_x0(obj, n)[0], dtype=np.float64)
    lb, ub = np.full(n, float(lo)), np.full(n, float(hi))
    fixed = (0, 4, 5, 8)
    for i in fixed:
        lb[i] = ub[i] = x0[i]
    kw = dict(maxeval=300, ftol_rel=1e-10)
    r = O.run_ref_mma(obj, n, x0=x0, lb=lb, ub=ub, step=step, **kw)
    a = run_local_amd(nlopt_amd.LD_MMA, obj, n, False, x0=x0, lb=lb, ub=ub, step=step, **kw)
    assert (a["ret"], a["nevals"]) == (r["ret"], r["nevals"]), (a["ret"], r["ret"], a["nevals"], r["nevals"], a["err"])
    assert len(a["fseq"]) == len(r["fseq"]) and np.all(np.abs(a["fseq"] - r["fseq"]) <= 1e-10 * np.maximum(np.abs(r["fseq"]), 1.0))
    assert all(a["x"][i] == lb[i] for i in fixed)
    assert abs(a["minf"] - r["minf"]) <= 1e-10 * max(abs(r["minf"]), 1.0)
