"""-m gpu: user-supplied device constraints for NLOPT_GN_ISRES (include/nlopt_amd_device.h: NLOPT_AMD_DEVICE_CONSTRAINTS;
include/nlopt_amd.h: nlopt_amd_add_inequality_device_mconstraint / ..._equality_...).  tests/usercon/cons_extra.hip is written
against the public header only and compiled into a code object outside the library.  Checked here:
  - the fold kernel behind nla_k_isres_eval_cv against the reference's loop (isres.c:141-166), bit for bit;
  - the user's <name>_coneval kernel through the adapter (no host twin) against sequential Python twins, bit for bit;
  - whole ISRES runs with bound blocks against the same runs with the twins as ordinary host constraints (the host-callback path
    is the one pinned to the reference, tests/test_gpu_host_callbacks.py) — and the counter isres_usercon_launches, which says
    where the constraints ran;
  - lifetime of the blocks (nlopt_copy, nlopt_remove_*_constraints, nlopt_destroy) and the error messages."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import nlopt_amd
from nlopt_amd import DevBuf

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "usercon", "cons_extra.hip")
CO = os.path.join(HERE, "usercon", "cons_extra.hsaco")
OBJ_ONLY = os.path.join(HERE, "userobj", "zoo_extra.hsaco")          # holds objectives, no constraint block
OBJ_ONLY_SRC = os.path.join(HERE, "userobj", "zoo_extra.hip")
RTOL = 1e-10
R, CC, D = 60.0, 1.0, 1.5                                            # the constants of cons_extra.hip


def _genco(src, out):
    if not os.path.exists(out) or os.path.getmtime(out) < os.path.getmtime(src):
        subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I",
                        os.path.join(os.path.dirname(HERE), "include"), src, "-o", out], check=True)
    return out


@pytest.fixture(scope="module")
def code_object():
    return _genco(SRC, CO)


@pytest.fixture(scope="module")
def L():
    return nlopt_amd.lib()


# ---- host twins: the sample's formulas as sequential loops over Python floats (IEEE doubles, no contraction) ------------------
def g0(x):
    s = 0.0
    for v in x:
        s += v * v
    return s - R


def g1(x):
    return x[0] * x[1 if len(x) > 1 else 0] - CC


def g2(x):
    s = 0.0
    for v in x[1::2]:
        s += v
    return s - 1.0


def h0(x):
    return x[0] + 2.0 * x[-1] - D


def twin_cons(x):
    x = [float(v) for v in x]
    return [g0(x), g1(x), g2(x), h0(x)]


def twin_pair(x):
    x = [float(v) for v in x]
    return [g0(x), g2(x)]


def twin_eqh(x):
    x = [float(v) for v in x]
    return [h0(x)]


def twin_many(x):
    x = [float(v) for v in x]
    return [x[j % len(x)] * float(j + 1) - 1.0 for j in range(70)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the fold: nla_k_isres_eval_cv ----------------------------------------------------------------------------------------------
CON = np.dtype([("type", "<i4"), ("q", "<u4"), ("Q", "<u4"), ("pad", "<i4"), ("tol", "<f8")])      # nla_dev_constraint
SENT = -7.25
TOLS = (0.0, 0.125, 0.5)
KPOP = 70                       # 18 workgroups of four wavefronts, the last with two


def fold_inputs(n, m, p):
    """entries alternate: even entries are values computed beforehand (type 1, their own column of C), odd ones block sums
    (type 0).  C: multiples of 1/64 and arbitrary doubles; row 0: every value equals its tolerance exactly, row 1: the first value
    is NaN, row 2: every value is negative."""
    mp = m + p
    rng = np.random.default_rng(1000 * n + 10 * m + p)
    con = np.zeros(max(mp, 1), CON)
    ncols = 0
    Q = max(1, min(n, (mp + 1) // 2))
    for c in range(mp):
        if c % 2 == 0:
            con[c] = (1, ncols, 0, 0, TOLS[c % 3])
            ncols += 1
        else:
            con[c] = (0, (c // 2) % Q, Q, 0, TOLS[c % 3])
    ldc = max(2, (ncols + 1) & ~1)
    X = rng.uniform(-1.5, 1.5, size=(KPOP, n))
    X[3:20] = rng.integers(-128, 129, size=(17, n)) / 64.0
    Cv = np.full((KPOP, ldc), SENT)
    Cv[:, :ncols] = rng.uniform(-1.0, 1.0, size=(KPOP, ncols))
    Cv[20:40, :ncols] = rng.integers(-64, 65, size=(20, ncols)) / 64.0
    for c in range(mp):
        if con[c]["type"] == 1:
            Cv[0, con[c]["q"]] = con[c]["tol"]
            Cv[2, con[c]["q"]] = -0.75
    if ncols:
        Cv[1, 0] = np.nan
    return con, X, Cv, ldc


def fold_reference(X, m, p, con, Cv):
    """isres.c:141-166 on scalar entries"""
    n = X.shape[1]
    PEN, GPEN, FEAS = [], [], []
    seen = set()
    for k, x in enumerate(X.tolist()):
        pen = gpen = 0.0
        feas = 1
        for c in range(m + p):
            tol = float(con[c]["tol"])
            if con[c]["type"] == 1 and Cv is not None:
                g = float(Cv[k, con[c]["q"]])
                seen.add("nan" if g != g else "neg" if g < 0 else "eq" if g == tol else "other")
            else:
                q, Q = int(con[c]["q"]), int(con[c]["Q"])
                s = 0.0
                for i in range((q * n) // Q, ((q + 1) * n) // Q):
                    s += x[i]
                g = s - 1.0
            if c == m:
                gpen = pen
            if c < m:
                if g > tol:
                    feas = 0
                if g < 0:
                    g = 0.0
                pen += g * g
            else:
                if abs(g) > tol:
                    feas = 0
                pen += g * g
        if p == 0:
            gpen = pen
        PEN.append(pen)
        GPEN.append(gpen)
        FEAS.append(feas)
    return np.array(PEN), np.array(GPEN), np.array(FEAS, np.int32), seen


def run_fold(L, X, m, p, con, Cv, ldc, cv=True):
    pop, n = X.shape
    ld = (n + 1) & ~1
    Xp = np.zeros((pop, ld))
    Xp[:, :n] = X
    dX, dcon = DevBuf.from_array(Xp), DevBuf.from_array(con)
    dC = DevBuf.from_array(Cv) if Cv is not None else None
    dF, dP, dG = (DevBuf.from_array(np.full(pop + 1, SENT)) for _ in range(3))
    dfe = DevBuf.from_array(np.full(pop + 1, -9, np.int32))
    if cv:
        rc = L.nla_k_isres_eval_cv(-1, n, ld, dX.ptr, pop, m, p, dcon.ptr, dC.ptr if dC else None, ldc, dF.ptr, dP.ptr, dG.ptr, dfe.ptr, None)
    else:
        L.nla_k_isres_eval.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_int] + [C.c_void_p] * 6
        rc = L.nla_k_isres_eval(-1, n, ld, dX.ptr, pop, m, p, dcon.ptr, dF.ptr, dP.ptr, dG.ptr, dfe.ptr, None)
    assert rc == 0
    assert L.nla_stream_sync(None) == 0
    F, PEN, GPEN = (d.to_array(np.float64, pop + 1) for d in (dF, dP, dG))
    FEAS = dfe.to_array(np.int32, pop + 1)
    for d in (dX, dcon, dF, dP, dG, dfe) + ((dC,) if dC else ()):
        d.free()
    assert np.all(F == SENT) and PEN[pop] == SENT and GPEN[pop] == SENT and FEAS[pop] == -9      # obj < 0: F untouched
    return PEN[:pop], GPEN[:pop], FEAS[:pop]


@pytest.mark.parametrize("n", [1, 3, 64])
@pytest.mark.parametrize("m,p", [(1, 0), (0, 1), (64, 0), (64, 3), (65, 2), (0, 0)])
def test_fold_of_precomputed_values_is_the_references_loop(L, n, m, p):
    """PEN, GPEN, FEAS bit for bit; the gpen snapshot at a 64-entry chunk boundary (64, 3), inside the second chunk (65, 2), nowhere
    (p = 0); a value equal to its tolerance (feasible), a NaN, negative inequality values"""
    con, X, Cv, ldc = fold_inputs(n, m, p)
    PENr, GPENr, FEASr, seen = fold_reference(X, m, p, con, Cv)
    if m + p:
        assert {"nan", "neg", "eq", "other"} <= seen
        if m + p == 1:
            assert FEASr[0] == 1                     # row 0: the precomputed value sits on its tolerance
        assert np.isnan(PENr[1]) and 0 in FEASr
    PEN, GPEN, FEAS = run_fold(L, X, m, p, con, Cv, ldc)
    assert np.array_equal(bits(PEN), bits(PENr)) and np.array_equal(bits(GPEN), bits(GPENr)) and np.array_equal(FEAS, FEASr)


def test_fold_of_a_value_entry_without_values_is_nan(L):
    """C == NULL with an entry of type 1 (the driver never does that): its value is NaN — no block sum with Q = 0, no read"""
    n, m, p = 3, 2, 1
    con, X, _, _ = fold_inputs(n, m, p)                       # entries 0 and 2 are of type 1, entry 1 a block sum
    PEN, GPEN, FEAS = run_fold(L, X, m, p, con, None, 0)
    assert np.all(np.isnan(PEN)) and np.all(np.isnan(GPEN))
    con[0]["type"] = 0; con[0]["q"], con[0]["Q"] = 0, 1       # only the equality entry is left without a value: GPEN is finite again
    PENr, GPENr, _, _ = fold_reference(X, m, 0, con, None)
    PEN, GPEN, FEAS = run_fold(L, X, m, p, con, None, 0)
    assert np.all(np.isnan(PEN)) and np.array_equal(bits(GPEN), bits(GPENr))


@pytest.mark.parametrize("m,p", [(4, 3), (65, 2)])
def test_fold_without_values_is_nla_k_isres_eval(L, m, p):
    """a block-sum-only list: nla_k_isres_eval and nla_k_isres_eval_cv(C = NULL) give equal bits (and the reference's)"""
    n = 64
    con, X, _, _ = fold_inputs(n, m, p)
    Q = min(n, m + p)
    for c in range(m + p):
        con[c] = (0, c % Q, Q, 0, TOLS[c % 3])
    PENr, GPENr, FEASr, _ = fold_reference(X, m, p, con, None)
    a = run_fold(L, X, m, p, con, None, 0, cv=False)
    b = run_fold(L, X, m, p, con, None, 0, cv=True)
    for u, v, r in zip(a, b, (PENr, GPENr, FEASr)):
        assert np.array_equal(bits(u), bits(v)) if u.dtype == np.float64 else np.array_equal(u, v)
        assert np.array_equal(bits(u), bits(r)) if u.dtype == np.float64 else np.array_equal(u, r)


# ---- the user's kernel through the adapter ---------------------------------------------------------------------------------------
def eval_entry(L, o, equality, index, x, m):
    """the values of constraint entry `index` of the object at x, as every host path gets them: through the entry's callback (for a
    bound block without a twin: one point through <name>_coneval)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(m, np.nan)
    L.nla_constraint_eval.argtypes = [C.c_void_p, C.c_int, C.c_uint, C.c_uint, C.c_void_p, C.c_void_p]
    assert L.nla_constraint_eval(o._h, int(equality), index, len(x), x.ctypes.data, out.ctypes.data) == 0
    return out


@pytest.mark.parametrize("n", [2, 7])
def test_coneval_through_the_adapter_equals_the_python_twin(L, code_object, n):
    o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, n)
    assert o.add_inequality_device_constraints(code_object, "cons", 4) > 0, o.get_errmsg()        # no twin
    assert o.add_equality_device_constraints(code_object, "many", 70) > 0, o.get_errmsg()
    assert o.device_constraint_count() == 2
    pts = np.random.default_rng(n).uniform(-3.0, 3.0, size=(50, n))
    for x in pts:
        got = eval_entry(L, o, 0, 0, x, 4)
        assert np.array_equal(bits(got), bits(twin_cons(x))), (x, got, twin_cons(x))
    for x in pts[:5]:
        got = eval_entry(L, o, 1, 0, x, 70)
        assert np.array_equal(bits(got), bits(twin_many(x)))
        assert np.array_equal(bits(eval_entry(L, o, 1, 0, x, 70)), bits(got))                      # the same point again
    assert np.array_equal(bits(eval_entry(L, o, 0, 0, pts[0], 4)), bits(twin_cons(pts[0])))


# ---- whole runs ------------------------------------------------------------------------------------------------------------------
def rastrigin(x, g):
    f = 10.0 * len(x)
    for xi in x:
        f += xi * xi - 10.0 * np.cos(6.283185307179586 * xi)
    return float(f)


def seqsphere(x, g):
    s = 0.0
    for xi in x:
        d = float(xi) - 0.3
        s += d * d
    return s


def start_point(n):
    """feasible for the sample's g0, g2, h0 (h0 exactly 0) and for block sums: row 0 of the first generation is feasible, the random
    rows are not (an equality with tolerance 1e-8)"""
    x0 = np.zeros(n)
    x0[0] = 0.5
    x0[n - 1] += 0.5 if n > 1 else 0.0
    return x0


def add_host_block(L, o, equality, m, twin, tol):
    """the twin as an ordinary m-dimensional host constraint (nlopt_add_*_mconstraint): today's path"""
    def _cb(mm, res, n, x, g, d):
        v = twin(np.ctypeslib.as_array(x, shape=(n,)))
        for j in range(mm):
            res[j] = float(v[j])
    cb = nlopt_amd.NLOPT_MFUNC(_cb)
    o._keep.append(cb)
    fn = L.nlopt_add_equality_mconstraint if equality else L.nlopt_add_inequality_mconstraint
    fn.argtypes = [C.c_void_p, C.c_uint, C.c_void_p, C.c_void_p, C.POINTER(C.c_double)]
    t = np.full(m, float(tol))
    assert fn(o._h, m, C.cast(cb, C.c_void_p).value, None, t.ctypes.data_as(C.POINTER(C.c_double))) > 0


def add_blocksum(L, o, q, Q, equality, tol):
    data = (C.c_uint * 2)(q, Q)
    o._keep.append(data)
    cb = C.cast(L.nlopt_amd_constraint_blocksum(), C.c_void_p).value
    add = L.nlopt_add_equality_constraint if equality else L.nlopt_add_inequality_constraint
    assert add(o._h, cb, C.addressof(data), float(tol)) > 0


PAIR_EQH = (("blk", "pair", 2, twin_pair, False, 0.0), ("blk", "eqh", 1, twin_eqh, True, 1e-8))


def run_isres(L, co, n, pop, me, spec, device, objective="rastrigin", maximize=False, host_eval=False, twins=True, seed=7, x0=None):
    o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, n)
    o.set_lower_bounds(-5.12)
    o.set_upper_bounds(5.12)
    if objective == "rastrigin":
        (o.set_max_objective if maximize else o.set_min_objective)(nlopt_amd.objective("rastrigin"))
    elif objective == "seqsphere":                        # the objective `cons` that the sample holds beside its block `cons`
        if device:
            assert o.set_min_device_objective(co, "cons", seqsphere) > 0, o.get_errmsg()
        else:
            o.set_min_objective(seqsphere)
    elif device:
        assert o.set_min_device_objective(_genco(OBJ_ONLY_SRC, OBJ_ONLY), objective, rastrigin) > 0, o.get_errmsg()
    else:
        o.set_min_objective(rastrigin)
    for e in spec:
        if e[0] == "bs":
            add_blocksum(L, o, e[1], e[2], e[3], e[4])
        elif device:
            add = o.add_equality_device_constraints if e[4] else o.add_inequality_device_constraints
            assert add(co, e[1], e[2], e[3] if twins else None, e[5]) > 0, o.get_errmsg()
        else:
            add_host_block(L, o, e[4], e[2], e[3], e[5])
    if host_eval:
        o.set_param("amd_host_eval", 1)
    o.set_population(pop)
    o.set_maxeval(me)
    o.enable_trace(me + 64)
    nlopt_amd.srand(seed)
    x, minf, ret = o.optimize_raw(start_point(n) if x0 is None else x0)
    assert ret > 0, o.get_errmsg()
    return dict(x=x, minf=minf, ret=ret, nev=o.get_numevals(), t=o.trace(), st=o.stats(), o=o)


def assert_same_run(d, h, pop):
    assert d["ret"] == h["ret"] and d["nev"] == h["nev"] and len(d["t"]) == len(h["t"])
    assert d["st"]["mt_words"] == h["st"]["mt_words"]
    first = h["t"]["accepted"][:pop]
    assert first.min() == 0 and first.max() == 1          # feasible and infeasible candidates: the ranking is the stochastic one
    assert np.array_equal(d["t"]["accepted"], h["t"]["accepted"])
    scale = np.abs(h["t"]["f"]).mean()
    assert np.all(np.abs(d["t"]["f"] - h["t"]["f"]) <= RTOL * np.maximum(np.abs(h["t"]["f"]), scale))
    assert abs(d["minf"] - h["minf"]) <= RTOL * max(abs(h["minf"]), scale)
    assert np.allclose(d["x"], h["x"], rtol=1e-9, atol=1e-9)
    if np.array_equal(d["t"]["f"], h["t"]["f"]):
        assert np.array_equal(d["x"], h["x"])             # identical f on both paths: x bit for bit


@pytest.mark.parametrize("objective,n,pop,me", [("rastrigin", 6, 60, 1500), ("myrastrigin", 40, 200, 2400)])
def test_isres_with_device_blocks_equals_the_host_path(L, code_object, objective, n, pop, me):
    """g0, g2 (tolerance 0) and h0 (tolerance 1e-8) as bound blocks against the twins as ordinary host constraints"""
    d = run_isres(L, code_object, n, pop, me, PAIR_EQH, True, objective)
    h = run_isres(L, code_object, n, pop, me, PAIR_EQH, False, objective)
    assert_same_run(d, h, pop)
    gens = d["st"]["generations"] + 1                      # (the generation the run stopped in is not counted as finished)
    assert d["st"]["isres_usercon_launches"] == 2 * gens and h["st"]["isres_usercon_launches"] == 0
    e = run_isres(L, code_object, n, pop, me, PAIR_EQH, True, objective, host_eval=True)
    assert e["st"]["isres_usercon_launches"] == 0
    assert_same_run(e, h, pop)
    if objective == "rastrigin":
        assert np.array_equal(e["t"]["f"], h["t"]["f"]) and np.array_equal(e["x"], h["x"]) and e["minf"] == h["minf"]


def test_inequalities_decide_feasibility_and_the_run_is_the_host_run_bit_for_bit(L, code_object):
    """inequality entries only (g0, g2, tolerance 0): among the RANDOM rows of the first generation some are feasible and some are not, so
    the entries' own feasibility flags decide candidates.  The objective sums sequentially on the device as on the host (the sample's
    objective `cons`), so f is identical on both paths and the whole run is: trace, x, minf bit for bit, no condition"""
    n, pop, me = 6, 60, 1500
    spec = (PAIR_EQH[0],)
    d = run_isres(L, code_object, n, pop, me, spec, True, "seqsphere")
    h = run_isres(L, code_object, n, pop, me, spec, False, "seqsphere")
    rnd = h["t"]["accepted"][1:pop]                          # row 0 is the caller's start point
    assert rnd.min() == 0 and rnd.max() == 1
    assert_same_run(d, h, pop)
    assert np.array_equal(bits(d["t"]["f"]), bits(h["t"]["f"])) and np.array_equal(d["x"], h["x"]) and d["minf"] == h["minf"]
    assert d["st"]["isres_usercon_launches"] > 0 and h["st"]["isres_usercon_launches"] == 0
    tw = run_isres(L, code_object, n, pop, me, spec, True, "seqsphere", twins=False)       # no twins bound: nothing else changes
    assert np.array_equal(bits(tw["t"]["f"]), bits(h["t"]["f"])) and np.array_equal(tw["x"], h["x"])


def test_block_sums_and_device_blocks_interleaved(L, code_object):
    """block sum, device block, block sum — in that order — and an equality block: the flattened list is [bs0, g0, g2, bs1 | h0].
    GPEN (the penalty before the first equality) takes part in choosing the best candidate (isres.c:174-177) and every entry's own
    tolerance in its feasibility, so the run equals the host path only with every entry in its place"""
    n, pop, me = 6, 60, 1500
    spec = (("bs", 0, 2, False, 0.0), PAIR_EQH[0], ("bs", 1, 2, False, 1e-8), PAIR_EQH[1])
    d = run_isres(L, code_object, n, pop, me, spec, True)
    h = run_isres(L, code_object, n, pop, me, spec, False)
    assert_same_run(d, h, pop)
    assert d["st"]["isres_usercon_launches"] > 0 and h["st"]["isres_usercon_launches"] == 0


def test_more_than_64_scalar_constraints(L, code_object):
    """70 entries from one block: two chunks of the fold.  x0 = 0 is feasible (every g = -1); a random row is feasible only with every
    coordinate below 1/66"""
    n, pop, me = 5, 40, 800
    spec = (("blk", "many", 70, twin_many, False, 1e-8),)
    x0 = np.zeros(n)
    d = run_isres(L, code_object, n, pop, me, spec, True, x0=x0)
    h = run_isres(L, code_object, n, pop, me, spec, False, x0=x0)
    assert_same_run(d, h, pop)
    assert d["st"]["isres_usercon_launches"] > 0
    e = run_isres(L, code_object, n, pop, 200, spec, True, host_eval=True, twins=False, x0=x0)   # no twin: every point through the kernel
    assert e["st"]["isres_usercon_launches"] == 0
    g = run_isres(L, code_object, n, pop, 200, spec, False, x0=x0)
    assert_same_run(e, g, pop)


def test_maximisation_keeps_the_objective_on_the_device(L, code_object):
    n, pop, me = 6, 60, 1500
    d = run_isres(L, code_object, n, pop, me, PAIR_EQH, True, maximize=True)
    h = run_isres(L, code_object, n, pop, me, PAIR_EQH, False, maximize=True)
    assert_same_run(d, h, pop)
    assert d["st"]["isres_usercon_launches"] > 0
    assert d["minf"] > 0 and abs(d["minf"] - rastrigin(d["x"], None)) <= RTOL * d["minf"]        # the caller's sign: max f, not -f
    assert np.all(d["t"]["f"] <= 0)                                                              # ... while the run minimised -f


# ---- lifetime ----------------------------------------------------------------------------------------------------------------------
def wrap(L, handle, n):
    o = nlopt_amd.Opt.__new__(nlopt_amd.Opt)
    o._L, o._h, o.n, o._keep, o._trace, o._last, o._minf = L, handle, n, [], None, None, None
    return o


def bound(code_object, n=6, pop=60, me=600):
    o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, n)
    o.set_lower_bounds(-5.12)
    o.set_upper_bounds(5.12)
    o.set_min_objective(nlopt_amd.objective("rastrigin"))
    assert o.add_inequality_device_constraints(code_object, "pair", 2) > 0, o.get_errmsg()        # no twins: nothing of Python's is shared
    assert o.add_equality_device_constraints(code_object, "eqh", 1, tol=1e-8) > 0, o.get_errmsg()
    o.set_population(pop)
    o.set_maxeval(me)
    return o


def go(o, n=6):
    nlopt_amd.srand(11)
    x, minf, ret = o.optimize_raw(start_point(n))
    assert ret > 0, o.get_errmsg()
    return x, minf, o.get_numevals(), o.stats()["isres_usercon_launches"]


def test_copies_share_the_blocks(L, code_object):
    o = bound(code_object)
    c = wrap(L, L.nlopt_copy(o._h), 6)
    assert c._h and c.device_constraint_count() == 2
    a, b = go(o), go(c)
    assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[3] > 0
    del o                                                   # nlopt_destroy(original): the copy keeps the blocks alive
    b2 = go(c)
    assert np.array_equal(b2[0], b[0]) and b2[1:] == b[1:]


def test_removed_constraints_release_the_blocks(L, code_object):
    o = bound(code_object)
    assert o.device_constraint_count() == 2
    assert L.nlopt_remove_inequality_constraints(o._h) > 0
    assert o.device_constraint_count() == 1
    assert L.nlopt_remove_equality_constraints(o._h) > 0
    assert o.device_constraint_count() == 0
    x, minf, nev, launches = go(o)
    assert launches == 0
    u = nlopt_amd.Opt(nlopt_amd.GN_ISRES, 6)                # the same run as an unconstrained object
    u.set_lower_bounds(-5.12); u.set_upper_bounds(5.12)
    u.set_min_objective(nlopt_amd.objective("rastrigin"))
    u.set_population(60); u.set_maxeval(600)
    xu, minfu, nevu, _ = go(u)
    assert np.array_equal(x, xu) and minf == minfu and nev == nevu


LN_AUGLAG_EQ, LN_COBYLA = 32, 25


def auglag(L, code_object, device, n=4):
    """LN_AUGLAG_EQ hands every inequality entry — (callback, data) as they are — to its subsidiary optimiser (LN_COBYLA) through the plain
    adders and keeps the equalities for its penalty: a bound block then sits in two objects"""
    o = nlopt_amd.Opt(LN_AUGLAG_EQ, n)
    o.set_lower_bounds(-2.0)
    o.set_upper_bounds(2.0)
    o.set_min_objective(nlopt_amd.objective("sphere"))
    if device:
        assert o.add_inequality_device_constraints(code_object, "pair", 2) > 0, o.get_errmsg()     # no twins: single points through the kernel
        assert o.add_equality_device_constraints(code_object, "eqh", 1, tol=1e-8) > 0, o.get_errmsg()
    else:
        add_host_block(L, o, False, 2, twin_pair, 0.0)
        add_host_block(L, o, True, 1, twin_eqh, 1e-8)
    loc = nlopt_amd.Opt(LN_COBYLA, n)
    loc.set_xtol_rel(1e-6)
    loc.set_maxeval(60)
    assert L.nlopt_set_local_optimizer(o._h, loc._h) > 0
    o.set_xtol_rel(1e-6)
    o.set_maxeval(300)
    return o


def test_auglag_shares_a_bound_block_with_its_subsidiary_optimiser(L, code_object):
    n = 4
    x0 = np.full(n, 0.25)
    h = auglag(L, code_object, False)
    xh, fh, rh = h.optimize_raw(x0)
    assert rh > 0, h.get_errmsg()
    o = auglag(L, code_object, True)
    for _ in range(2):                                        # the second run removes and re-adds the subsidiary's entries
        x, f, r = o.optimize_raw(x0)
        assert r == rh and f == fh and np.array_equal(x, xh), o.get_errmsg()
        assert o.device_constraint_count() == 2
    c = wrap(L, L.nlopt_copy(o._h), n)
    del o                                                     # destroys the subsidiary optimiser's entries with the original
    assert c.device_constraint_count() == 2
    x, f, r = c.optimize_raw(x0)
    assert r == rh and f == fh and np.array_equal(x, xh), c.get_errmsg()
    i = nlopt_amd.Opt(nlopt_amd.GN_ISRES, 6)                  # ... and the blocks still load and run elsewhere
    del c
    assert i.add_inequality_device_constraints(code_object, "pair", 2) > 0, i.get_errmsg()


# ---- errors --------------------------------------------------------------------------------------------------------------------------
def test_binding_errors_are_loud_and_add_nothing(L, code_object, tmp_path):
    o = nlopt_amd.Opt(nlopt_amd.GN_ISRES, 4)
    for co, name, msg in ((str(tmp_path / "nosuch.hsaco"), "cons", "could not load code object"),
                          (code_object, "nosuch", "kernel nosuch_coneval not found"),
                          (_genco(OBJ_ONLY_SRC, OBJ_ONLY), "myrastrigin", "kernel myrastrigin_coneval not found")):
        for add in (o.add_inequality_device_constraints, o.add_equality_device_constraints):
            assert add(co, name, 2) == nlopt_amd.INVALID_ARGS
            assert msg in o.get_errmsg(), o.get_errmsg()
            assert o.device_constraint_count() == 0
    c = nlopt_amd.Opt(nlopt_amd.GN_CRS2_LM, 4)              # an algorithm without constraints: the reference's refusal (options.c:549-557)
    for add in (c.add_inequality_device_constraints, c.add_equality_device_constraints):
        assert add(code_object, "cons", 2) == nlopt_amd.INVALID_ARGS
        assert c.get_errmsg() == "invalid algorithm for constraints"
        assert c.device_constraint_count() == 0
