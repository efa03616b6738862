"""-m gpu: device objectives and constraints that READ THE CALLER'S DATA (include/nlopt_amd_device.h ABI 2; include/nlopt_amd.h:
nlopt_amd_set_device_objective_data, nlopt_amd_add_*_device_mconstraint_data, nlopt_amd_eval_device_objective).
tests/userdata/fit_models.hip is written against the header only, the way a user would, and compiled into a code object outside the
library.

  - the residual-sum kernel (NLOPT_AMD_DEVICE_RESIDUALS) bit for bit against a numpy model that restates the header's documented
    order of the sums, and against a long double sequential sum to 1e-10; the same point gives the same bits wherever it stands in a
    launch;
  - an ABI-2 objective that ignores its data gives the bits of its ABI-1 statement;
  - every algorithm that launches a user kernel hands it the optimiser's data: CRS2_LM, ISRES, ESCH, LD_LBFGS, LD_MMA, MLSL with
    L-BFGS and with COBYLA, with and without a host twin, against the numpy twin as an ordinary host callback;
  - whose data: set in turn, after nlopt_copy, from two threads at once;
  - ISRES with a data-carrying constraint block; the error messages."""
import ctypes as C
import os
import subprocess
import threading

import numpy as np
import pytest

import nlopt_amd

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "userdata", "fit_models.hip")
CO = os.path.join(HERE, "userdata", "fit_models.hsaco")
ABI1_SRC = os.path.join(HERE, "userobj", "zoo_extra.hip")
ABI1_CO = os.path.join(HERE, "userobj", "zoo_extra.hsaco")
RTOL = 1e-10


def _genco(src, out):
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I",
                        os.path.join(os.path.dirname(HERE), "include"), src, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def co():
    return _genco(SRC, CO)


@pytest.fixture(scope="module")
def abi1_co():
    return _genco(ABI1_SRC, ABI1_CO)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the kernel, bit for bit --------------------------------------------------------------------------------------------------------
def polyfit_model(x, t, y, NP, grad=True):
    """f and gradient of the sample `polyfit` at x, in the order include/nlopt_amd_device.h documents for NLOPT_AMD_DEVICE_RESIDUALS:
    per-thread sums (thread t adds residuals t, t+256, ... in that order), the xor-butterfly 32..1 in each of the four wavefronts, the
    wave combine ((w0 + w1) + w2) + w3, G = 2 g.  Every product is rounded before it is added (no FMA: numpy, and -ffp-contract=off)."""
    n, m = len(x), len(t)
    p, s, d = np.ones(m), np.zeros(m), np.zeros((NP, m))
    for i in range(NP):
        if i < n:
            s = s + x[i] * p
            d[i] = -p
        p = p * t
    r = y - s
    acc = np.zeros((NP + 1, 256))                       # row 0: f, rows 1..NP: g
    for k0 in range(0, m, 256):
        rk, dk = r[k0:k0 + 256], d[:, k0:k0 + 256]
        c = len(rk)
        acc[0, :c] = acc[0, :c] + rk * rk
        acc[1:, :c] = acc[1:, :c] + rk * dk
    w = acc.reshape(NP + 1, 4, 64)
    lane = np.arange(64)
    for step in (32, 16, 8, 4, 2, 1):
        w = w + w[:, :, lane ^ step]
    tot = ((w[:, 0, 0] + w[:, 1, 0]) + w[:, 2, 0]) + w[:, 3, 0]
    return tot[0], (2 * tot[1:1 + n] if grad else None)


def polyfit_longdouble(x, t, y):
    """the same sums sequentially in long double; also the sum of the gradient terms' magnitudes (the scale of its rounding error)"""
    L = np.longdouble
    f, g, gabs = L(0), np.zeros(len(x), dtype=L), np.zeros(len(x), dtype=L)
    xs = [L(v) for v in x]
    for tk, yk in zip(t, y):
        p, s, d = L(1), L(0), []
        for xi in xs:
            s += xi * p
            d.append(-p)
            p *= L(tk)
        r = L(yk) - s
        f += r * r
        for i, di in enumerate(d):
            g[i] += 2 * r * di
            gabs[i] += abs(2 * r * di)
    return f, g, gabs


def fit_data(m, seed):
    rng = np.random.RandomState(seed)
    return rng.uniform(-1.2, 1.2, m), rng.uniform(-2.0, 2.0, m)


def bound_opt(co, name, n, alg=None, twin=None):
    o = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM if alg is None else alg, n)
    assert o.set_min_device_objective(co, name, twin) > 0, o.get_errmsg()
    return o


def check_kernel_bits(o, name_np, n, m, seed):
    t, y = fit_data(m, seed)
    X = np.random.RandomState(1000 + seed).uniform(-2.0, 2.0, (5, n))
    assert o.set_device_objective_data(np.concatenate([t, y])) > 0, o.get_errmsg()
    F, G = o.eval_device_objective(X, grad=True)
    F0 = o.eval_device_objective(X)
    assert np.array_equal(bits(F0), bits(F)), (n, m)                     # with and without the gradient: the same f
    for c in range(5):
        f, g = polyfit_model(X[c], t, y, name_np)
        print("n=%d m=%d row %d: f=%.17g model=%.17g" % (n, m, c, F[c], f))
        assert bits(F[c]) == bits(f), (n, m, c, F[c], f)
        assert np.array_equal(bits(G[c]), bits(g)), (n, m, c, G[c], g)
        fl, gl, gabs = polyfit_longdouble(X[c], t, y)
        assert abs(np.longdouble(F[c]) - fl) <= RTOL * abs(fl), (n, m, c)
        # (a gradient component is a sum of terms of both signs: its rounding error scales with the sum of their magnitudes)
        assert np.all(np.abs(G[c].astype(np.longdouble) - gl) <= RTOL * gabs), (n, m, c)
        if m == 0:
            assert F[c] == 0.0 and not G[c].any()


@pytest.mark.parametrize("n", [1, 3, 8])
def test_the_residual_kernel_bit_for_bit(co, n):
    """m = 0 (no data: f = 0, g = 0), one residual, around one wavefront, around one pass of the workgroup, several passes"""
    o = bound_opt(co, "polyfit", n)
    for m in (0, 1, 63, 64, 65, 255, 256, 257, 1000):
        check_kernel_bits(o, 8, n, m, seed=m + 7 * n)


def test_the_residual_kernel_at_np_32_bit_for_bit(co):
    check_kernel_bits(bound_opt(co, "polyfit32", 32), 32, 32, 300, seed=5)


def test_the_same_point_gives_the_same_bits_wherever_it_stands(co):
    """alone, as row 3 of 5, as row 4999 of 5000: the split of the sums depends on m only"""
    n, m = 8, 257
    t, y = fit_data(m, 3)
    o = bound_opt(co, "polyfit", n)
    assert o.set_device_objective_data(np.concatenate([t, y])) > 0
    rng = np.random.RandomState(17)
    x = rng.uniform(-2, 2, n)
    f1, g1 = o.eval_device_objective(x, grad=True)
    X5 = rng.uniform(-2, 2, (5, n)); X5[3] = x
    X5k = rng.uniform(-2, 2, (5000, n)); X5k[4999] = x
    F5, G5 = o.eval_device_objective(X5, grad=True)
    F5k, G5k = o.eval_device_objective(X5k, grad=True)
    assert bits(f1) == bits(F5[3]) == bits(F5k[4999])
    assert np.array_equal(bits(g1), bits(G5[3])) and np.array_equal(bits(g1), bits(G5k[4999]))
    f, g = polyfit_model(x, t, y, 8)
    assert bits(f1) == bits(f) and np.array_equal(bits(g1), bits(g))
    assert np.array_equal(bits(F5k[:5]), bits(o.eval_device_objective(X5k[:5])))


@pytest.mark.parametrize("n", [1, 64, 65, 200])
def test_an_abi_2_objective_that_ignores_its_data_gives_the_abi_1_bits(co, n):
    """`shifted` with an all-zero centre (and with no data at all) against the same sphere stated with the ABI-1 macro, and against the
    library's compiled-in sphere"""
    X = np.random.RandomState(n).uniform(-3, 3, (7, n))
    a = bound_opt(co, "sphere1", n)
    F1, G1 = a.eval_device_objective(X, grad=True)
    b = bound_opt(co, "shifted", n)
    for data in (None, np.zeros(n)):
        assert b.set_device_objective_data(data) > 0, b.get_errmsg()
        F2, G2 = b.eval_device_objective(X, grad=True)
        assert np.array_equal(bits(F1), bits(F2)) and np.array_equal(bits(G1), bits(G2))
    L = nlopt_amd.lib()
    ld = (n + 1) & ~1
    Xp = np.zeros((7, ld)); Xp[:, :n] = X
    d_X, d_F = L.nla_dev_malloc(Xp.nbytes), L.nla_dev_malloc(8 * 7)
    Fc = np.empty(7)
    try:
        assert L.nla_memcpy_h2d(d_X, Xp.ctypes.data, Xp.nbytes, None) == 0
        assert L.nla_k_eval(nlopt_amd.OBJECTIVES["sphere"], n, ld, d_X, 7, d_F, None) == 0
        assert L.nla_memcpy_d2h(Fc.ctypes.data, d_F, 8 * 7, None) == 0 and L.nla_stream_sync(None) == 0
    finally:
        L.nla_dev_free(d_X); L.nla_dev_free(d_F)
    assert np.array_equal(bits(Fc), bits(F2))
    c = np.linspace(-1, 1, n)                                 # ... and a centre that is not zero moves it
    assert b.set_device_objective_data(c) > 0
    F3, G3 = b.eval_device_objective(X, grad=True)
    assert np.allclose(F3, ((X - c) ** 2).sum(axis=1), rtol=1e-12) and np.array_equal(bits(G3), bits(2 * (X - c)))


# ---- end to end against the host twin -------------------------------------------------------------------------------------------------
def poly_problem(m=200, shift=0.0):
    k = np.arange(m)
    t = np.linspace(-1.0, 1.0, m)
    y = (0.5 + shift) - 1.2 * t + 0.8 * t * t + (2.0 - shift) * t ** 3 + 0.01 * np.sin(37.0 * k)
    return t, y


def poly_twin(t, y):
    def f(x, g):
        V = np.vander(t, len(x), increasing=True)
        r = y - V @ x
        if g.size:
            g[:] = -2.0 * (V.T @ r)
        return float(r @ r)
    return f


def exp_problem(m=200):
    k = np.arange(m)
    t = np.linspace(0.0, 4.0, m)
    return t, 2.5 * np.exp(-1.3 * t) + 0.5 + 0.01 * np.sin(29.0 * k)


def exp_twin(t, y):
    def f(x, g):
        e = np.exp(-x[1] * t)
        r = y - (x[0] * e + x[2])
        if g.size:
            g[:] = 2.0 * np.array([(r * -e).sum(), (r * x[0] * t * e).sum(), -r.sum()])
        return float(r @ r)
    return f


POLY_N = 4
POLY_X0 = -3.0 + 6.0 * np.modf(np.arange(1, POLY_N + 1) * 0.6180339887498949)[0]


def make_poly(alg, co, t, y, device=True, twin=True, n=POLY_N):
    o = nlopt_amd.Opt(alg, n)
    o.set_lower_bounds(-3.0)
    o.set_upper_bounds(3.0)
    if device:
        assert o.set_min_device_objective(co, "polyfit", poly_twin(t, y) if twin else None) > 0, o.get_errmsg()
        assert o.set_device_objective_data(np.concatenate([t, y])) > 0, o.get_errmsg()
    else:
        o.set_min_objective(poly_twin(t, y))
    return o


def run_global(alg, co, t, y, pop, me, seed, device=True, twin=True):
    o = make_poly(alg, co, t, y, device, twin)
    o.set_population(pop)
    o.set_maxeval(me)
    o.enable_trace(me + 64)
    nlopt_amd.srand(seed)
    x, minf, ret = o.optimize_raw(POLY_X0)
    return dict(x=x, minf=minf, ret=ret, nev=o.get_numevals(), t=o.trace(), st=o.stats())


def same_run(d, h):
    assert d["ret"] == h["ret"] and d["nev"] == h["nev"] and len(d["t"]) == len(h["t"]), (d["ret"], h["ret"], d["nev"], h["nev"])
    assert d["st"]["mt_words"] == h["st"]["mt_words"]
    for k in ("kind", "row", "accepted"):
        assert np.array_equal(d["t"][k], h["t"][k]), k
    scale = np.abs(h["t"]["f"]).mean()
    assert np.all(np.abs(d["t"]["f"] - h["t"]["f"]) <= RTOL * np.maximum(np.abs(h["t"]["f"]), scale))
    assert abs(d["minf"] - h["minf"]) <= RTOL * max(abs(h["minf"]), scale)


@pytest.mark.parametrize("alg,pop,me", [(nlopt_amd.GN_CRS2_LM, 300, 3000), (nlopt_amd.GN_ISRES, 60, 1500), (nlopt_amd.GN_ESCH, 60, 1500)])
def test_global_algorithms_with_a_data_reading_kernel_equal_the_host_twin(co, alg, pop, me):
    t, y = poly_problem()
    d = run_global(alg, co, t, y, pop, me, 42)
    h = run_global(alg, co, t, y, pop, me, 42, device=False)
    same_run(d, h)
    assert d["minf"] < np.abs(h["t"]["f"]).mean()             # (the run got somewhere: f is not the constant a kernel without data would give)
    if alg == nlopt_amd.GN_CRS2_LM:
        assert np.array_equal(d["x"], h["x"])                                   # x does not depend on f: bit for bit
        assert d["st"]["slots_launched"] > d["st"]["rounds"]                    # windows of several slots: the device path


def test_crs_without_a_twin_gives_the_same_trace(co):
    t, y = poly_problem()
    a = run_global(nlopt_amd.GN_CRS2_LM, co, t, y, 300, 3000, 42)
    b = run_global(nlopt_amd.GN_CRS2_LM, co, t, y, 300, 3000, 42, twin=False)
    assert (a["ret"], a["nev"], a["minf"]) == (b["ret"], b["nev"], b["minf"])
    assert np.array_equal(a["t"], b["t"]) and np.array_equal(a["x"], b["x"])


EXP_LB, EXP_UB, EXP_X0 = np.array([0.1, 0.1, -1.0]), np.array([5.0, 5.0, 2.0]), np.array([1.0, 1.0, 0.0])


def run_local(alg, co, device, twin=True, fixed=None):
    t, y = exp_problem()
    lb, ub, x0 = EXP_LB.copy(), EXP_UB.copy(), EXP_X0.copy()
    if fixed is not None:
        lb[fixed[0]] = ub[fixed[0]] = x0[fixed[0]] = fixed[1]
    o = nlopt_amd.Opt(alg, 3)
    o.set_lower_bounds(lb)
    o.set_upper_bounds(ub)
    if device:
        assert o.set_min_device_objective(co, "expfit", exp_twin(t, y) if twin else None) > 0, o.get_errmsg()
        assert o.set_device_objective_data(np.concatenate([t, y])) > 0, o.get_errmsg()
    else:
        o.set_min_objective(exp_twin(t, y))
    o.set_ftol_rel(1e-10)
    o.set_maxeval(400)
    o.set_param("amd_exact_dot", 1)
    x, minf, ret = o.optimize_raw(x0)
    return dict(x=x, minf=minf, ret=ret, nev=o.get_numevals())


@pytest.mark.parametrize("alg", [nlopt_amd.LD_LBFGS, nlopt_amd.LD_MMA])
def test_local_optimisers_fit_an_exponential_on_the_device(co, alg):
    d, h = run_local(alg, co, True), run_local(alg, co, False)
    assert d["ret"] == h["ret"] and d["ret"] > 0, (d, h)
    assert abs(d["minf"] - h["minf"]) <= 1e-8 * max(abs(h["minf"]), 1.0)
    assert np.allclose(d["x"], h["x"], rtol=1e-6, atol=1e-7), (d, h)
    assert np.allclose(d["x"], [2.5, 1.3, 0.5], atol=0.05)                      # the decay the data were made from


def test_lbfgs_with_a_fixed_coordinate_and_no_twin(co):
    """lb == ub in one coordinate, nothing but the kernel to evaluate with: every path to it carries the data"""
    d, h = run_local(nlopt_amd.LD_LBFGS, co, True, twin=False, fixed=(2, 0.45)), run_local(nlopt_amd.LD_LBFGS, co, False, fixed=(2, 0.45))
    assert d["ret"] > 0 and h["ret"] > 0 and d["x"][2] == 0.45
    assert np.allclose(d["x"], h["x"], rtol=1e-6, atol=1e-7), (d, h)


@pytest.mark.parametrize("alg,local", [(nlopt_amd.GD_MLSL, nlopt_amd.LD_LBFGS), (nlopt_amd.GN_MLSL, nlopt_amd.LN_COBYLA)])
def test_mlsl_runs_batched_on_the_device_with_a_data_reading_kernel(co, alg, local):
    t, y = poly_problem()
    res = []
    for device in (True, False):
        o = make_poly(alg, co, t, y, device, twin=False)
        loc = nlopt_amd.Opt(local, POLY_N)
        if local == nlopt_amd.LD_LBFGS:
            loc.set_ftol_rel(1e-10)
        else:
            loc.set_xtol_rel(1e-6)
        assert nlopt_amd.lib().nlopt_set_local_optimizer(o._h, loc._h) > 0
        o.set_population(16)
        o.set_maxeval(2500)
        o.enable_trace(2600)
        nlopt_amd.srand(3)
        x, minf, ret = o.optimize_raw(POLY_X0)
        res.append(dict(ret=ret, x=x, minf=minf, t=o.trace(), st=o.stats()))
    d, h = res
    assert d["ret"] > 0 and h["ret"] > 0
    assert d["st"]["lbfgs_launches"] >= 1 and d["st"]["cobyla_host_searches"] == 0, d["st"]        # the batched device path
    scale = np.abs(h["t"]["f"][h["t"]["kind"] == 3]).mean()                    # f over the sample points
    print("minf device %.17g host %.17g scale %.6g" % (d["minf"], h["minf"], scale))
    assert abs(d["minf"] - h["minf"]) <= RTOL * scale


# ---- whose data ------------------------------------------------------------------------------------------------------------------------
def lbfgs_poly(o):
    o.set_ftol_rel(1e-12)
    o.set_maxeval(400)
    o.set_param("amd_exact_dot", 1)
    x, minf, ret = o.optimize_raw(POLY_X0)
    assert ret > 0, o.get_errmsg()
    return x, minf


def test_two_data_sets_in_turn_on_one_optimiser(co):
    A, B = poly_problem(), poly_problem(shift=0.7)
    o = make_poly(nlopt_amd.LD_LBFGS, co, *A, twin=False)
    xa, fa = lbfgs_poly(o)
    assert o.set_device_objective_data(np.concatenate(B)) > 0                   # no rebinding
    xb, fb = lbfgs_poly(o)
    ha, _ = lbfgs_poly(make_poly(nlopt_amd.LD_LBFGS, co, *A, device=False))
    hb, _ = lbfgs_poly(make_poly(nlopt_amd.LD_LBFGS, co, *B, device=False))
    assert np.allclose(xa, ha, rtol=1e-6, atol=1e-7) and np.allclose(xb, hb, rtol=1e-6, atol=1e-7), (xa, ha, xb, hb)
    assert np.abs(xa - xb).max() > 0.1
    assert o.set_device_objective_data(None) > 0                                # cleared: the kernel sees m = 0
    assert o.eval_device_objective(xa) == 0.0


def test_data_set_on_a_copy_leaves_the_original_alone(co):
    A, B = poly_problem(), poly_problem(shift=0.7)
    o = make_poly(nlopt_amd.LD_LBFGS, co, *A, twin=False)
    xa, fa = lbfgs_poly(o)
    c = o.copy()
    xc, fc = lbfgs_poly(c)                                                      # the copy shares the block
    assert np.array_equal(xc, xa) and fc == fa
    assert c.set_device_objective_data(np.concatenate(B)) > 0
    xa2, fa2 = lbfgs_poly(o)
    assert np.array_equal(xa2, xa) and fa2 == fa
    xb, fb = lbfgs_poly(c)
    hb, _ = lbfgs_poly(make_poly(nlopt_amd.LD_LBFGS, co, *B, device=False))
    assert np.allclose(xb, hb, rtol=1e-6, atol=1e-7) and np.abs(xa - xb).max() > 0.1
    del o                                                                       # nlopt_destroy(original): the copy keeps kernel and data
    xb2, fb2 = lbfgs_poly(c)
    assert np.array_equal(xb2, xb) and fb2 == fb


def test_two_threads_each_with_a_copy_and_its_own_data(co):
    sets = [poly_problem(), poly_problem(shift=0.7)]
    o = make_poly(nlopt_amd.GN_CRS2_LM, co, *sets[0], twin=False)
    o.set_population(300)
    o.set_maxeval(3000)

    def work(c, out, i):
        nlopt_amd.srand(42)                                                     # (the generator is the calling thread's)
        x, minf, ret = c.optimize_raw(POLY_X0)
        out[i] = (x, minf, ret, c.get_numevals())

    copies = [o.copy(), o.copy()]
    for c, s in zip(copies, sets):
        assert c.set_device_objective_data(np.concatenate(s)) > 0
    serial, conc = [None, None], [None, None]
    for i, c in enumerate(copies):
        work(c, serial, i)
    th = [threading.Thread(target=work, args=(c, conc, i)) for i, c in enumerate(copies)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for s, c in zip(serial, conc):
        assert c is not None and s[2] > 0 and np.array_equal(s[0], c[0]) and s[1:] == c[1:]
    assert serial[0][1] != serial[1][1]


# ---- constraints ---------------------------------------------------------------------------------------------------------------------------
CON_A = np.array([[1.0, 1.0, 0.0, 0.0, 0.0, 0.0], [0.0, -1.0, 2.0, 0.0, 0.5, 0.0], [0.25, 0.0, 0.0, 1.0, 0.0, -1.0]])
CON_B = np.array([1.0, 0.5, 0.75])


def lincons_twin(x):
    out = []
    for j in range(3):
        s = 0.0
        for i in range(len(x)):
            s += CON_A[j, i] * float(x[i])
        out.append(s - CON_B[j])
    return out


def run_isres_lincons(co, device):
    n, pop, me = 6, 60, 300                                                     # 5 generations
    L = nlopt_amd.lib()
    o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, n)
    o.set_lower_bounds(-5.12)
    o.set_upper_bounds(5.12)
    o.set_min_objective(nlopt_amd.objective("rastrigin"))
    if device:
        assert o.add_inequality_device_constraints(co, "lincons", 3, lincons_twin, data=np.concatenate([CON_A.ravel(), CON_B])) > 0, o.get_errmsg()
    else:
        def _cb(mm, res, nn, x, g, d):
            v = lincons_twin(np.ctypeslib.as_array(x, shape=(nn,)))
            for j in range(mm):
                res[j] = v[j]
        cb = nlopt_amd.NLOPT_MFUNC(_cb)
        o._keep.append(cb)
        L.nlopt_add_inequality_mconstraint.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
        assert L.nlopt_add_inequality_mconstraint(o._h, 3, C.cast(cb, C.c_void_p).value, None, None) > 0
    o.set_population(pop)
    o.set_maxeval(me)
    o.enable_trace(me + 64)
    nlopt_amd.srand(7)
    x, minf, ret = o.optimize_raw(np.zeros(n))
    assert ret > 0, o.get_errmsg()
    return dict(x=x, minf=minf, ret=ret, nev=o.get_numevals(), t=o.trace(), st=o.stats(), o=o)


def test_isres_with_a_data_carrying_constraint_block(co):
    d, h = run_isres_lincons(co, True), run_isres_lincons(co, False)
    assert d["ret"] == h["ret"] and d["nev"] == h["nev"] and len(d["t"]) == len(h["t"])
    assert d["st"]["mt_words"] == h["st"]["mt_words"]
    acc = h["t"]["accepted"][:60]
    assert acc.min() == 0 and acc.max() == 1                                    # feasible and infeasible candidates: the block decides
    for k in ("kind", "row", "accepted"):
        assert np.array_equal(d["t"][k], h["t"][k]), k
    scale = np.abs(h["t"]["f"]).mean()
    assert np.all(np.abs(d["t"]["f"] - h["t"]["f"]) <= RTOL * np.maximum(np.abs(h["t"]["f"]), scale))
    assert d["st"]["isres_usercon_launches"] > 0 and h["st"]["isres_usercon_launches"] == 0
    # one point through the block's kernel (no twin bound): the twin's bits, so the kernel read A and b
    o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, 6)
    assert o.add_inequality_device_constraints(co, "lincons", 3, data=np.concatenate([CON_A.ravel(), CON_B])) > 0, o.get_errmsg()
    x = np.random.RandomState(2).uniform(-2, 2, 6)
    out = np.empty(3)
    L = nlopt_amd.lib()
    L.nla_constraint_eval.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    assert L.nla_constraint_eval(o._h, 0, 0, 6, x.ctypes.data_as(C.POINTER(C.c_double)), out.ctypes.data_as(C.POINTER(C.c_double))) == 0
    assert np.array_equal(bits(out), bits(lincons_twin(x)))


# ---- errors --------------------------------------------------------------------------------------------------------------------------------
def test_errors_are_loud_and_leave_the_optimiser_as_it_was(co, abi1_co):
    L = nlopt_amd.lib()
    blk = np.arange(8.0)
    o = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, 4)
    assert o.set_device_objective_data(blk) == nlopt_amd.INVALID_ARGS and "no device objective is bound" in o.get_errmsg()
    assert L.nlopt_amd_has_device_objective(o._h) == 0
    o.set_min_objective(lambda x, g: 0.0)                                       # an ordinary objective is no device objective either
    assert o.set_device_objective_data(blk) == nlopt_amd.INVALID_ARGS and "no device objective is bound" in o.get_errmsg()

    assert o.set_min_device_objective(abi1_co, "shubert") > 0, o.get_errmsg()   # ABI 1: takes no data
    x = np.array([0.3, -1.0, 2.0, 0.7])
    before = o.eval_device_objective(x)                                         # (the evaluator serves either ABI)
    assert o.set_device_objective_data(blk) == nlopt_amd.INVALID_ARGS and "ABI 1" in o.get_errmsg()
    assert L.nlopt_amd_has_device_objective(o._h) == 1 and o.eval_device_objective(x) == before

    t, y = poly_problem(64)
    assert o.set_min_device_objective(co, "polyfit") > 0, o.get_errmsg()
    assert o.set_device_objective_data(np.concatenate([t, y])) > 0
    before = o.eval_device_objective(x)
    assert before > 0
    assert L.nlopt_amd_set_device_objective_data(o._h, None, 16) == nlopt_amd.INVALID_ARGS and "NULL" in o.get_errmsg()
    assert o.eval_device_objective(x) == before                                 # the block that was set is still the one read

    assert o.set_min_device_objective(co, "future") == nlopt_amd.INVALID_ARGS    # <name>_abi writes 3
    assert "ABI 3" in o.get_errmsg()
    assert L.nlopt_amd_has_device_objective(o._h) == 1 and o.eval_device_objective(x) == before

    big = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, 9)                                 # polyfit serves n <= 8: refused where it is bound
    assert big.set_min_device_objective(co, "polyfit") == nlopt_amd.INVALID_ARGS and "n <= 8" in big.get_errmsg()
    assert L.nlopt_amd_has_device_objective(big._h) == 0

    i = nlopt_amd.Opt(nlopt_amd.GN_ISRES, 6)                                    # a constraint block of ABI 1 takes no data either
    cons1 = _genco(os.path.join(HERE, "usercon", "cons_extra.hip"), os.path.join(HERE, "usercon", "cons_extra.hsaco"))
    assert i.add_inequality_device_constraints(cons1, "pair", 2, data=blk) == nlopt_amd.INVALID_ARGS and "ABI 1" in i.get_errmsg()
    assert i.device_constraint_count() == 0
