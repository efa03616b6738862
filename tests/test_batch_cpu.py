"""CPU: nlopt_amd_optimize_batch (include/nlopt_amd.h, csrc/batch_driver.c), the row-data ABI (include/nlopt_amd_device.h ABI 3) and the
device-built waiting list (csrc/hip/local_list.hip) as far as a machine without a GPU can see them.

  - on the emulated device layer (oracle/libnlopt_amd_emu.so: the product's drivers over kernels restated in C): LD_LBFGS and LD_MMA with
    an ordinary host callback — search i of a batch is the lone nlopt_optimize from x_i, and the REAL reference's run from x_i, bit for
    bit; the callback is called in ascending search order within a step; the chunking changes nothing; the refusals leave x and the
    optimiser alone; binding and row-data calls fail loudly (no code object loads there);
  - tests/batch/fit_rows.hip cross-compiles for gfx950 and defines <name>_evalgrad_r, _abi and _form; the list kernel and the NP = 8
    row-data residual kernel use no scratch; libnlopt_amd.so exports the new entry points.
tests/test_gpu_batch.py runs the feature."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nlopt_amd
import _oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")
SRC = os.path.join(HERE, "batch", "fit_rows.hip")
LIST_SRC = os.path.join(ROOT, "nlopt_amd", "csrc", "hip", "local_list.hip")
HIPCC = "/opt/rocm/bin/hipcc"
FUNC = C.CFUNCTYPE(C.c_double, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
vp, dbl, dpp, ip = C.c_void_p, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_int)
LD_LBFGS, LD_MMA, LN_COBYLA, GN_CRS2_LM = 11, 24, 25, 19
INVALID_ARGS, FORCED_STOP, SUCCESS = -2, -5, 1
N = 4


def bind(L, batch):
    L.nlopt_create.restype = vp
    L.nlopt_create.argtypes = [C.c_int, C.c_uint]
    L.nlopt_destroy.argtypes = [vp]
    for nm in ("nlopt_set_lower_bounds", "nlopt_set_upper_bounds"):
        getattr(L, nm).argtypes = [vp, dpp]
    for nm in ("nlopt_set_ftol_rel", "nlopt_set_xtol_rel", "nlopt_set_stopval"):
        getattr(L, nm).argtypes = [vp, dbl]
    for nm in ("nlopt_get_ftol_rel", "nlopt_get_stopval"):
        getattr(L, nm).argtypes = [vp]
        getattr(L, nm).restype = dbl
    L.nlopt_set_min_objective.argtypes = [vp, vp, vp]
    L.nlopt_set_max_objective.argtypes = [vp, vp, vp]
    L.nlopt_set_maxeval.argtypes = [vp, C.c_int]
    L.nlopt_get_maxeval.argtypes = [vp]
    L.nlopt_optimize.argtypes = [vp, dpp, dpp]
    L.nlopt_get_numevals.argtypes = [vp]
    L.nlopt_force_stop.argtypes = [vp]
    L.nlopt_get_errmsg.argtypes = [vp]
    L.nlopt_get_errmsg.restype = C.c_char_p
    L.nlopt_add_inequality_constraint.argtypes = [vp, vp, vp, dbl]
    if batch:
        L.nlopt_set_param.argtypes = [vp, C.c_char_p, dbl]
        L.nlopt_amd_optimize_batch.argtypes = [vp, C.c_size_t, dpp, dpp, ip, ip]
        L.nlopt_amd_set_min_device_objective.argtypes = [vp, C.c_char_p, C.c_char_p, vp, vp]
        L.nlopt_amd_set_device_objective_row_data.argtypes = [vp, C.c_size_t, C.c_size_t, vp]
        L.nlopt_amd_set_comm.argtypes = [vp, vp]
        L.nlopt_amd_comm_create_host.restype = vp
        L.nlopt_amd_comm_create_host.argtypes = [C.c_int, C.c_int, vp, vp]
        L.nlopt_amd_comm_destroy.argtypes = [vp]
    return L


@pytest.fixture(scope="module")
def emu():
    assert os.path.exists(EMU), "oracle/libnlopt_amd_emu.so is not built (build() makes it)"
    return bind(C.CDLL(EMU), True)


# a smooth objective with two basins per coordinate and an analytic gradient; records (search-identifying x, gradient requested?)
CENTRE = np.array([0.7, -0.4, 1.3, 0.2])
WGT = 1 + 0.3 * np.arange(N)


def objective(calls=None, on_call=None, sign=1.0):
    def f(nn, xp, gp, d):
        x = np.array([xp[i] for i in range(nn)])
        if calls is not None:
            calls.append((x.tobytes(), bool(gp)))
        if on_call is not None:
            on_call(len(calls))
        if gp:
            g = sign * (2 * WGT * (x - CENTRE) - 1.5 * np.sin(3 * x))
            for i in range(nn):
                gp[i] = float(g[i])
        return sign * float(np.sum(WGT * (x - CENTRE) ** 2) + 0.5 * np.sum(np.cos(3 * x)))
    return FUNC(f)


STARTS = np.array([[-1.5, 2.0, 0.1, -0.7], [2.5, 2.5, -2.0, 1.0], [0.0, 0.0, 0.0, 0.0]])
LB, UB = np.full(N, -3.0), np.full(N, 4.0)
dp = lambda a: a.ctypes.data_as(dpp)


def make_opt(L, alg, fcb, maximise=False):
    o = L.nlopt_create(alg, N)
    L.nlopt_set_lower_bounds(o, dp(LB))
    L.nlopt_set_upper_bounds(o, dp(UB))
    (L.nlopt_set_max_objective if maximise else L.nlopt_set_min_objective)(o, C.cast(fcb, vp), None)
    L.nlopt_set_ftol_rel(o, 1e-10)
    L.nlopt_set_maxeval(o, 200)
    return o


def lone(L, alg, x0, maximise=False):
    calls = []
    fcb = objective(calls, sign=-1.0 if maximise else 1.0)
    o = make_opt(L, alg, fcb, maximise)
    x = np.array(x0, dtype=np.float64)
    minf = C.c_double(123.0)
    ret = L.nlopt_optimize(o, dp(x), C.byref(minf))
    out = dict(x=x, minf=minf.value, ret=ret, nev=L.nlopt_get_numevals(o), calls=calls)
    L.nlopt_destroy(o)
    return out


def batch(L, alg, X0, chunk=0, maximise=False):
    calls = []
    fcb = objective(calls, sign=-1.0 if maximise else 1.0)
    o = make_opt(L, alg, fcb, maximise)
    if chunk:
        assert L.nlopt_set_param(o, b"amd_batch_chunk", float(chunk)) > 0, L.nlopt_get_errmsg(o)
    X = np.array(X0, dtype=np.float64)
    count = len(X)
    minf, res, nev = np.full(count, np.nan), np.zeros(count, dtype=np.intc), np.zeros(count, dtype=np.intc)
    ret = L.nlopt_amd_optimize_batch(o, count, dp(X), dp(minf), res.ctypes.data_as(ip), nev.ctypes.data_as(ip))
    msg = L.nlopt_get_errmsg(o)
    out = dict(X=X, minf=minf, res=res, nev=nev, ret=ret, total=L.nlopt_get_numevals(o), calls=calls, msg=msg.decode() if msg else None)
    L.nlopt_destroy(o)
    return out


def same_search(b, i, one):
    assert b["res"][i] == one["ret"], (i, b["res"][i], one["ret"])
    assert b["nev"][i] == one["nev"], (i, b["nev"][i], one["nev"])
    assert np.array_equal(b["X"][i].view(np.uint64), one["x"].view(np.uint64)), (i, b["X"][i], one["x"])
    assert np.float64(b["minf"][i]).view(np.uint64) == np.float64(one["minf"]).view(np.uint64), (i, b["minf"][i], one["minf"])


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
@pytest.mark.parametrize("count", [1, 3])
def test_on_the_emulated_device_a_batch_equals_the_lone_runs(emu, alg, count):
    b = batch(emu, alg, STARTS[:count])
    assert b["ret"] == SUCCESS, b["msg"]
    ones = [lone(emu, alg, STARTS[i]) for i in range(count)]
    for i in range(count):
        same_search(b, i, ones[i])
        assert b["res"][i] > 0
    assert b["total"] == sum(o["nev"] for o in ones)
    # every search saw exactly the calls of its lone run, in their order (the batch interleaves the searches step by step)
    for i in range(count):
        mine = [c for c in b["calls"] if c in set(ones[i]["calls"])]
        assert mine == ones[i]["calls"], i


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_the_callback_is_called_in_ascending_search_order_within_a_step(emu, alg):
    """the first step of a batch evaluates every start: rows 0, 1, 2 in that order"""
    b = batch(emu, alg, STARTS)
    first = [np.frombuffer(c[0]) for c in b["calls"][:3]]
    assert all(np.array_equal(first[i], STARTS[i]) for i in range(3)), first


@pytest.mark.skipif(not O.have_ref(), reason="oracle/_ref is not built")
@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
@pytest.mark.parametrize("count", [1, 3])
def test_a_batch_with_a_host_callback_equals_the_real_reference(emu, alg, count):
    R = bind(O.ref(), False)
    b = batch(emu, alg, STARTS[:count])
    for i in range(count):
        same_search(b, i, lone(R, alg, STARTS[i]))


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_maximisation_of_a_host_callback(emu, alg):
    b = batch(emu, alg, STARTS, maximise=True)
    assert b["ret"] == SUCCESS, b["msg"]
    for i in range(3):
        same_search(b, i, lone(emu, alg, STARTS[i], maximise=True))


@pytest.mark.parametrize("alg", [LD_LBFGS, LD_MMA])
def test_chunking_is_invariant(emu, alg):
    X0 = np.concatenate([STARTS, STARTS[::-1] * 0.5, STARTS[:2] + 0.25])          # 8 searches
    a = batch(emu, alg, X0)
    for chunk in (1, 3, 8):
        c = batch(emu, alg, X0, chunk=chunk)
        assert c["ret"] == a["ret"] == SUCCESS
        assert np.array_equal(c["X"].view(np.uint64), a["X"].view(np.uint64)) and np.array_equal(c["minf"].view(np.uint64), a["minf"].view(np.uint64))
        assert np.array_equal(c["res"], a["res"]) and np.array_equal(c["nev"], a["nev"]) and c["total"] == a["total"]


def test_maxeval_applies_to_each_search_and_force_stop_to_the_call(emu):
    fcb = objective([])
    o = make_opt(emu, LD_LBFGS, fcb)
    emu.nlopt_set_maxeval(o, 5)
    X = STARTS.copy()
    minf, res, nev = np.zeros(3), np.zeros(3, dtype=np.intc), np.zeros(3, dtype=np.intc)
    assert emu.nlopt_amd_optimize_batch(o, 3, dp(X), dp(minf), res.ctypes.data_as(ip), nev.ctypes.data_as(ip)) == SUCCESS
    # NLOPT_MAXEVAL_REACHED = 5.  (The third start ends inside a line search that the reference lets finish: 6 calls, lone and batched alike.)
    assert list(res) == [5, 5, 5] and list(nev) == [5, 5, 6] and emu.nlopt_get_numevals(o) == 16
    for i in range(3):
        x, m = STARTS[i].copy(), C.c_double()
        assert emu.nlopt_optimize(o, dp(x), C.byref(m)) == 5 and emu.nlopt_get_numevals(o) == nev[i]
        assert np.array_equal(x, X[i]) and m.value == minf[i]
    emu.nlopt_destroy(o)

    calls = []
    holder = {}
    fcb = objective(calls, on_call=lambda k: emu.nlopt_force_stop(holder["o"]) if k == 7 else None)
    holder["o"] = o = make_opt(emu, LD_LBFGS, fcb)
    X = STARTS.copy()
    assert emu.nlopt_amd_optimize_batch(o, 3, dp(X), dp(minf), res.ctypes.data_as(ip), nev.ctypes.data_as(ip)) == FORCED_STOP
    assert all(r == FORCED_STOP for r in res), res
    emu.nlopt_destroy(o)


def test_the_refusals_leave_x_and_the_optimiser_unchanged(emu):
    fcb = objective([])
    X0 = STARTS.copy()
    minf, res, nev = np.zeros(3), np.zeros(3, dtype=np.intc), np.zeros(3, dtype=np.intc)
    args = lambda X, count=3: (count, dp(X), dp(minf), res.ctypes.data_as(ip), nev.ctypes.data_as(ip))

    def refused(o, X, *a, msg):
        before = (emu.nlopt_get_ftol_rel(o), emu.nlopt_get_maxeval(o), emu.nlopt_get_stopval(o))
        assert emu.nlopt_amd_optimize_batch(o, *a) == INVALID_ARGS
        assert msg in emu.nlopt_get_errmsg(o).decode(), emu.nlopt_get_errmsg(o)
        assert np.array_equal(X, X0) and before == (emu.nlopt_get_ftol_rel(o), emu.nlopt_get_maxeval(o), emu.nlopt_get_stopval(o))

    X = X0.copy()
    o = make_opt(emu, GN_CRS2_LM, fcb)                                           # any other algorithm
    refused(o, X, *args(X), msg="serves NLOPT_LD_LBFGS")
    emu.nlopt_destroy(o)
    o = make_opt(emu, LN_COBYLA, fcb)                                            # COBYLA: device objectives only
    refused(o, X, *args(X), msg="device objectives only")
    emu.nlopt_destroy(o)
    o = make_opt(emu, LD_MMA, fcb)                                               # nonlinear constraints
    assert emu.nlopt_add_inequality_constraint(o, C.cast(fcb, vp), None, 1e-8) > 0
    refused(o, X, *args(X), msg="nonlinear constraints")
    emu.nlopt_destroy(o)
    o = make_opt(emu, LD_LBFGS, fcb)
    refused(o, X, *args(X, 0), msg="count == 0")
    refused(o, X, 3, None, dp(minf), res.ctypes.data_as(ip), None, msg="NULL array")
    refused(o, X, 3, dp(X), None, res.ctypes.data_as(ip), None, msg="NULL array")
    refused(o, X, 3, dp(X), dp(minf), None, None, msg="NULL array")
    refused(o, X, 2 ** 31, dp(X), dp(minf), res.ctypes.data_as(ip), None, msg="INT_MAX")
    Xout = X0.copy()
    Xout[2, 1] = 9.0                                                             # a start outside the box
    assert emu.nlopt_amd_optimize_batch(o, *args(Xout)) == INVALID_ARGS and "search 2" in emu.nlopt_get_errmsg(o).decode()
    comm = emu.nlopt_amd_comm_create_host(0, 1, None, None)                      # a communicator
    if comm:
        assert emu.nlopt_amd_set_comm(o, comm) > 0
        refused(o, X, *args(X), msg="communicator")
        emu.nlopt_amd_set_comm(o, None)
        emu.nlopt_amd_comm_destroy(comm)
    fixed = LB.copy()
    fixed[1] = UB[1] = 4.0                                                       # lb == ub
    emu.nlopt_set_lower_bounds(o, dp(fixed))
    Xf = X0.copy()
    Xf[:, 1] = 4.0
    assert emu.nlopt_amd_optimize_batch(o, *args(Xf)) == INVALID_ARGS
    assert "fixed coordinates is out of scope" in emu.nlopt_get_errmsg(o).decode() and np.all(Xf[:, 1] == 4.0)
    emu.nlopt_destroy(o)
    assert emu.nlopt_amd_optimize_batch(None, *args(X)) == INVALID_ARGS


def test_on_the_emulated_device_binding_and_row_data_fail_loudly(emu):
    o = emu.nlopt_create(LD_LBFGS, 3)
    buf = (C.c_double * 8)()
    try:
        assert emu.nlopt_amd_set_min_device_objective(o, os.path.join(HERE, "batch", "fit_rows.hsaco").encode(), b"expfit_rows", None, None) == INVALID_ARGS
        assert "could not load code object" in emu.nlopt_get_errmsg(o).decode()
        assert emu.nlopt_amd_set_device_objective_row_data(o, 2, 32, buf) == INVALID_ARGS
        assert "no device objective is bound" in emu.nlopt_get_errmsg(o).decode()
    finally:
        emu.nlopt_destroy(o)
    assert emu.nlopt_amd_set_device_objective_row_data(None, 2, 32, buf) == INVALID_ARGS


# ---- what the cross-compiler shows ------------------------------------------------------------------------------------------------
def _genco(tmp, src, name):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = str(tmp / name)
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"), src, "-o", out],
                   check=True)
    return out


@pytest.fixture(scope="module")
def images(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("batch")
    return _genco(tmp, SRC, "fit_rows.hsaco"), _genco(tmp, LIST_SRC, "local_list.hsaco")


def test_the_samples_compile_for_gfx950_and_define_the_row_kernels(images):
    image = open(images[0], "rb").read()
    has = lambda sym: (sym.encode() + b"\0" in image) and (sym.encode() + b".kd\0" in image)
    for name in ("expfit_rows", "polyfit_rows", "shifted_rows"):
        for sym in ("_evalgrad_r", "_abi", "_form"):
            assert has(name + sym), name + sym
        assert (name + "_evalgrad_d.kd").encode() not in image and (name + "_evalgrad.kd").encode() not in image, name
    for name in ("expfit2", "polyfit2", "shifted2"):                             # the same structs under the ABI-2 macros
        assert has(name + "_evalgrad_d") and (name + "_evalgrad_r.kd").encode() not in image, name


def test_the_list_kernel_and_the_row_residual_kernel_use_no_scratch(images):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = {k["name"]: k for img in images for k in kernel_resources.code_object_kernels(img)}
    lst = [k for name, k in ks.items() if "local_waiting_list_kernel" in name]
    assert len(lst) == 1
    for k in lst + [ks["polyfit_rows_evalgrad_r"], ks["expfit_rows_evalgrad_r"]]:
        assert k["scratch"] == "0" and k["vgpr_spill"] == "0", k
    assert int(lst[0]["lds"]) == 16, lst[0]                                       # the four wavefront totals


def test_the_library_exports_the_new_entry_points():
    L = C.CDLL(nlopt_amd.LIB_PATH)
    for name in ("nlopt_amd_optimize_batch", "nlopt_amd_set_device_objective_row_data", "nla_k_local_waiting_list", "nlopt_amd_local_list_launches"):
        assert hasattr(L, name), name
    for name in ("optimize_batch", "set_device_objective_row_data"):
        assert hasattr(nlopt_amd.Opt, name), name
    o = nlopt_amd.Opt(LD_LBFGS, 2)
    assert o.stats()["local_list_launches"] == 0
