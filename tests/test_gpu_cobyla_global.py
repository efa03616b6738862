"""-m gpu: batched device COBYLA beyond n = 51 (hip/cobyla_global.hip: the search of hip/cobyla_search.h, one wavefront per start, with its
five matrices in a per-search slice of a global-memory workspace) on the MI355X — the kernel against the real reference's LN_COBYLA
and against the LDS kernel bit for bit, its contract, and NLOPT_GN_MLSL(_LDS) with its default local optimiser at n = 52 / 64 staying
on the device.  Everything is compared in exact-order mode (sphere / Rosenbrock: no transcendental; the device's + - x / sqrt are IEEE)
unless a test says otherwise.  The CPU twin (the kernel on 64 lockstep threads) is tests/test_cobyla_global_emu.py."""
import ctypes as C

import numpy as np
import pytest

import _oracle as O
import nlopt_amd
import test_cobyla_differential as T
from test_gpu_cobyla import _Params, _Result, kernel_batch, reference_cobyla, run_gn_mlsl

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref not built")]

XTOL_REACHED, MAXEVAL_REACHED = 4, 5


def global_batch(obj, n, starts, lb, ub, xtol_rel=1e-6, maxeval=0, dx=None, exact=1, expect_rc=0):
    """nla_k_cobyla_batch_global on the device: test_gpu_cobyla.kernel_batch with the workspace the global kernel asks for"""
    L = nlopt_amd.lib()
    count, ld = starts.shape[0], (n + 1) & ~1
    X = np.zeros((count, ld)); X[:, :n] = starts
    bX, bl, bu = nlopt_amd.DevBuf.from_array(X), nlopt_amd.DevBuf.from_array(np.asarray(lb, dtype=np.float64)), nlopt_amd.DevBuf.from_array(np.asarray(ub, dtype=np.float64))
    bd = nlopt_amd.DevBuf.from_array(np.asarray(dx, dtype=np.float64)) if dx is not None else None
    L.nla_cobyla_global_work_doubles.restype = C.c_size_t
    L.nla_cobyla_global_work_doubles.argtypes = [C.c_int, C.c_int]
    bw, bi, bo = nlopt_amd.DevBuf(8 * max(8, L.nla_cobyla_global_work_doubles(n, count))), nlopt_amd.DevBuf(4 * max(8, count)), nlopt_amd.DevBuf(C.sizeof(_Result) * count)
    P = _Params(-np.inf, 0.0, 0.0, xtol_rel, maxeval, exact, 1.0, None, None, None)
    vp = C.c_void_p
    L.nla_k_cobyla_batch_global.argtypes = [C.c_int] * 4 + [vp] * 6 + [C.POINTER(_Params), vp, vp]
    rc = L.nla_k_cobyla_batch_global(nlopt_amd.OBJECTIVES[obj], n, ld, count, bl.ptr, bu.ptr, bd.ptr if bd else None, bX.ptr, bw.ptr, bi.ptr, C.byref(P), bo.ptr, None)
    if expect_rc is None:
        return rc
    assert rc == 0, L.nla_dev_error_string(rc)
    assert L.nla_stream_sync(None) == 0
    raw = bo.to_array(np.uint8, C.sizeof(_Result) * count)
    res = (_Result * count).from_buffer_copy(raw.tobytes())
    return dict(x=bX.to_array(np.float64, count * ld).reshape(count, ld)[:, :n], f=np.array([r.f for r in res]), ret=[r.ret for r in res], nevals=[r.nevals for r in res])


def boxes(obj, n, count, kind, seed):
    """box, starts and step as tests/test_gpu_cobyla.py builds them"""
    rng = np.random.default_rng(seed)
    lo, hi = nlopt_amd.objective_box(obj)
    lb, ub = np.full(n, lo), np.full(n, hi)
    starts = rng.uniform(lo, hi, (count, n))
    dx = None
    if kind == "onbound":
        starts[0, : max(1, n // 3)] = hi
        starts[-1, -1] = lo
    if kind == "halfinf":
        ub[0] = np.inf; lb[1] = -np.inf; lb[2] = -np.inf; ub[2] = np.inf
    if kind == "steps":
        dx = np.linspace(0.3, 1.7, n) * 0.1 * (hi - lo)
    return lb, ub, starts, dx


def same(a, r):
    assert a["ret"] == r["ret"] and a["nevals"] == r["nevals"], (a["ret"], r["ret"], a["nevals"], r["nevals"])
    assert np.array_equal(a["f"], r["f"]) and np.array_equal(a["x"], r["x"])


# n = 52: the first dimension past the LDS kernel; 64 / 65: one and two trips of the lanes over a column; 130: n in three trips and
# the m + 2 = 262 rows of a vertex in five; 96 searches: more than one per slot of a compute unit's share
@pytest.mark.parametrize("obj,n,count,maxeval,kind", [("sphere", 52, 3, 0, "plain"), ("rosenbrock", 64, 2, 0, "onbound"), ("sphere", 65, 2, 0, "steps"),
                                                      ("rosenbrock", 70, 2, 0, "halfinf"), ("sphere", 130, 2, 0, "plain"), ("rosenbrock", 52, 96, 90, "plain")])
def test_global_memory_cobyla_kernel_is_the_references_search_evaluation_by_evaluation(obj, n, count, maxeval, kind):
    """the initial simplex and 150 iterations behind it (or the given budget): result code, evaluation count, f and the minimiser
    are the real reference's bit for bit"""
    maxeval = maxeval or n + 1 + 150
    lb, ub, starts, dx = boxes(obj, n, count, kind, 1000 + n + count)
    a = global_batch(obj, n, starts, lb, ub, maxeval=maxeval, dx=dx)
    same(a, reference_cobyla(obj, n, starts, lb, ub, maxeval=maxeval, dx=dx))


@pytest.mark.parametrize("obj,seed", [("sphere", 3000), ("rosenbrock", 3010)])
def test_global_memory_cobyla_search_that_stops_by_itself(obj, seed):
    """xtol_rel = 0.25 at n = 52: the trust region shrinks to its end (SHRINK / FINISH) within the budget — the seeds are chosen so
    that the reference's searches all end with XTOL_REACHED (after 1 800 - 3 100 evaluations), and the kernel's are those searches"""
    n = 52
    lb, ub, starts, _ = boxes(obj, n, 2, "plain", seed)
    r = reference_cobyla(obj, n, starts, lb, ub, xtol_rel=0.25, maxeval=4000)
    assert r["ret"] == [XTOL_REACHED] * 2, (r["ret"], r["nevals"])
    same(global_batch(obj, n, starts, lb, ub, xtol_rel=0.25, maxeval=4000), r)


@pytest.mark.parametrize("n", [5, 33, 51])
def test_global_memory_cobyla_kernel_takes_the_lds_kernels_steps_bit_for_bit(n):
    """the dimensions both kernels serve: one body, two storage layouts — same starts, same bits"""
    lb, ub, starts, _ = boxes("rosenbrock", n, 3, "onbound", 70 + n)
    same(global_batch("rosenbrock", n, starts, lb, ub, maxeval=n + 1 + 300), kernel_batch("rosenbrock", n, starts, lb, ub, maxeval=n + 1 + 300))


def test_global_memory_cobyla_launcher_contract():
    L = nlopt_amd.lib()
    assert L.nla_cobyla_global_fits(256) == 1 and L.nla_cobyla_global_fits(257) == 0 and L.nla_cobyla_global_fits(1) == 1 and L.nla_cobyla_global_fits(0) == 0
    assert L.nla_cobyla_fits(51) == 1 and L.nla_cobyla_fits(52) == 0                     # the LDS kernel's limit is where it was
    assert global_batch("sphere", 257, np.zeros((1, 257)) + 0.5, np.full(257, -1.0), np.full(257, 1.0), maxeval=10, expect_rc=None) != 0
    # a fixed coordinate is refused exactly as the LDS kernel refuses it: INVALID_ARGS, no evaluation, f = inf, the start untouched
    n = 60
    lb, ub, starts, _ = boxes("sphere", n, 4, "plain", n)
    for i in (0, 17, 59):
        lb[i] = ub[i] = starts[0, i]
        starts[:, i] = lb[i]
    a = global_batch("sphere", n, starts, lb, ub, maxeval=200)
    assert a["ret"] == [nlopt_amd.INVALID_ARGS] * 4 and a["nevals"] == [0] * 4, (a["ret"], a["nevals"])
    assert np.all(a["f"] == np.inf) and np.array_equal(a["x"], starts)


# population 24, xtol_rel = 0.25; the budgets are chosen on the CPU (the same runs through the host algorithm, which are the reference's)
# so that at least three local searches complete: sphere n = 52 starts its fourth search before 5 000 evaluations, Rosenbrock
# n = 64 — whose third search alone takes more than 6 000 — before 12 000
MLSL_CASES = [(T.GN_MLSL, "sphere", 52, 5000), (T.GN_MLSL_LDS, "sphere", 52, 5000),
              (T.GN_MLSL, "rosenbrock", 64, 12000), (T.GN_MLSL_LDS, "rosenbrock", 64, 12000)]
_mlsl_ref = {}


def mlsl_reference(alg, obj, n, maxeval):
    key = (alg, obj, n, maxeval)
    if key not in _mlsl_ref:
        _mlsl_ref[key] = run_gn_mlsl(T.more_bind(O.ref()), alg, obj, n, maxeval, xtol=0.25, population=24)
    return _mlsl_ref[key]


@pytest.mark.parametrize("alg,obj,n,maxeval", MLSL_CASES)
def test_gn_mlsl_beyond_the_lds_dimension_stays_on_the_device_and_is_the_references_run(alg, obj, n, maxeval):
    """GN_MLSL(_LDS) with its default local optimiser at n > 51, parity mode: the searches run in batched launches of the
    global-memory kernel (none on the host) and the run is the reference's bit for bit; with "amd_cobyla_host" = 1 the same run
    through the host algorithm, no launch"""
    r = mlsl_reference(alg, obj, n, maxeval)
    A = T.more_bind(C.CDLL(nlopt_amd.LIB_PATH))
    a = run_gn_mlsl(A, alg, obj, n, maxeval, params=[("amd_exact_dot", 1), ("amd_cobyla_min_batch", 1)], xtol=0.25, population=24, stats=True)
    assert (a["ret"], a["minf"], a["nevals"]) == (r["ret"], r["minf"], r["nevals"]) and np.array_equal(a["x"], r["x"]), (a, r)
    assert a["searches"] >= 3, a
    assert a["launches"] > 0 and a["host_searches"] == 0, a
    h = run_gn_mlsl(A, alg, obj, n, maxeval, params=[("amd_exact_dot", 1), ("amd_cobyla_min_batch", 1), ("amd_cobyla_host", 1)], xtol=0.25, population=24, stats=True)
    assert (h["ret"], h["minf"], h["nevals"]) == (r["ret"], r["minf"], r["nevals"]) and np.array_equal(h["x"], r["x"]), (h, r)
    assert h["launches"] == 0, h


def test_gn_mlsl_beyond_the_lds_dimension_default_mode():
    """the default (tree-sum) objective at n = 52: f differs from the host twin's by rounding, so single steps may differ — the
    reference's result code, batched launches and a minimum of the reference's size (the latitude
    test_gpu_cobyla.test_gn_mlsl_batched_device_cobyla_default_mode grants n <= 51)"""
    alg, obj, n, maxeval = MLSL_CASES[0]
    r = mlsl_reference(alg, obj, n, maxeval)
    a = run_gn_mlsl(T.more_bind(C.CDLL(nlopt_amd.LIB_PATH)), alg, obj, n, maxeval, params=[("amd_cobyla_min_batch", 1)], xtol=0.25, population=24, stats=True)
    assert a["ret"] == r["ret"], (a, r)
    assert a["launches"] > 0
    assert 0.0 <= a["minf"] <= 2.0 * max(r["minf"], 1.0), (a["minf"], r["minf"])
