"""CPU: nlopt_amd_optimize_batch and nonlinear constraints (csrc/batch_driver.c) as far as a machine without a GPU can see them.

  - on the emulated device layer (oracle/libnlopt_amd_emu.so), which has neither code objects nor the constrained COBYLA launcher
    (hip/cobyla_con.hip is reached through weak references): every constrained batch is refused with NLOPT_INVALID_ARGS and its
    documented message, x and the optimiser untouched — never a call through a null symbol.  No device block can be bound on that
    layer, so the refusals that need one (a compiled-in objective beside bound blocks, an (n, mc) beyond the launcher, the missing
    launcher itself) are reached on the GPU only (tests/test_gpu_batch_constrained.py); here the layer's side of it is pinned: the
    symbols are absent, and the per-search memory with constraint values is the unconstrained one.
  - the product library exports the new entry points, and the new kernel uses no scratch.
tests/test_cobyla_con_emu.py runs the kernel on the CPU; tests/test_gpu_batch_constrained.py runs the feature."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

import nlopt_amd
from test_batch_cpu import EMU, INVALID_ARGS, LD_MMA, LN_COBYLA, STARTS, bind, dp, dpp, ip, make_opt, objective, vp
from test_api_differential import MFUNC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def emu():
    assert os.path.exists(EMU), "oracle/libnlopt_amd_emu.so is not built (build() makes it)"
    L = bind(C.CDLL(EMU), True)
    L.nlopt_add_equality_mconstraint.argtypes = [vp, C.c_uint, vp, vp, dpp]
    L.nlopt_amd_objective.restype = vp
    L.nlopt_amd_objective.argtypes = [C.c_int]
    L.nlopt_amd_batch_constraint_launches.restype = C.c_uint64
    L.nlopt_amd_batch_constraint_launches.argtypes = [vp]
    L.nlopt_amd_add_inequality_device_mconstraint.argtypes = [vp, C.c_uint, C.c_char_p, C.c_char_p, vp, vp, dpp]
    return L


def test_every_constrained_batch_is_refused_cleanly_on_the_emulated_layer(emu):
    fcb = objective([])
    con = objective([])
    mcb = MFUNC(lambda m, res, n, x, g, d: None)
    X0 = STARTS.copy()
    minf, res, nev = np.zeros(3), np.zeros(3, dtype=np.intc), np.zeros(3, dtype=np.intc)

    def refused(o, msg):
        X = X0.copy()
        before = (emu.nlopt_get_ftol_rel(o), emu.nlopt_get_maxeval(o), emu.nlopt_get_stopval(o))
        assert emu.nlopt_amd_optimize_batch(o, 3, dp(X), dp(minf), res.ctypes.data_as(ip), nev.ctypes.data_as(ip)) == INVALID_ARGS
        assert msg in emu.nlopt_get_errmsg(o).decode(), emu.nlopt_get_errmsg(o)
        assert np.array_equal(X, X0) and before == (emu.nlopt_get_ftol_rel(o), emu.nlopt_get_maxeval(o), emu.nlopt_get_stopval(o))
        assert emu.nlopt_amd_batch_constraint_launches(o) == 0

    o = make_opt(emu, LD_MMA, fcb)                                               # a derivative-based algorithm
    assert emu.nlopt_add_inequality_constraint(o, C.cast(con, vp), None, 1e-8) > 0
    refused(o, "nonlinear constraints are served for NLOPT_LN_COBYLA only")
    emu.nlopt_destroy(o)
    o = make_opt(emu, LN_COBYLA, fcb)                                            # a host callback as constraint (and as objective)
    assert emu.nlopt_add_inequality_constraint(o, C.cast(con, vp), None, 1e-8) > 0
    refused(o, "must be device blocks")
    refused(o, "inequality constraint 0 is a host callback")
    emu.nlopt_destroy(o)
    o = make_opt(emu, LN_COBYLA, fcb)                                            # ... beside a compiled-in objective, as an equality block
    emu.nlopt_set_min_objective(o, emu.nlopt_amd_objective(5), None)
    assert emu.nlopt_add_equality_mconstraint(o, 2, C.cast(mcb, vp), None, None) > 0
    refused(o, "equality constraint 0 is a host callback")
    # what would be served on the device cannot come to be here: no code object loads, so no block is bound
    r = emu.nlopt_amd_add_inequality_device_mconstraint(o, 1, os.path.join(ROOT, "tests", "batchcon", "con_models.hsaco").encode(), b"ball", None, None, None)
    assert r == INVALID_ARGS and "could not load code object" in emu.nlopt_get_errmsg(o).decode()
    emu.nlopt_destroy(o)
    assert emu.nlopt_amd_batch_constraint_launches(None) == 0


def test_the_emulated_layer_has_no_constrained_launcher_and_sizes_nothing_for_it(emu):
    for name in ("nla_k_cobyla_batch_ext_con", "nla_cobyla_con_serves", "nla_cobyla_con_work_doubles", "nla_cobyla_con_save_bytes"):
        assert not hasattr(emu, name), name

    class Evaluator(C.Structure):
        _fields_ = [("kind", C.c_int), ("obj", C.c_int), ("f", vp), ("f_data", vp), ("user", vp), ("sign", C.c_double)]
    emu.nla_local_ctx_bytes_per_search.restype = emu.nla_local_ctx_bytes_per_search_con.restype = C.c_size_t
    emu.nla_local_ctx_bytes_per_search.argtypes = [C.c_int, C.POINTER(Evaluator), C.c_int, C.c_int]
    emu.nla_local_ctx_bytes_per_search_con.argtypes = [C.c_int, C.POINTER(Evaluator), C.c_int, C.c_int, C.c_int, C.c_int]
    for kind in (0, 1, 2):
        ev = Evaluator(kind=kind, sign=1.0)
        for n in (1, 5, 64):
            plain = emu.nla_local_ctx_bytes_per_search(2, C.byref(ev), n, 0)
            assert emu.nla_local_ctx_bytes_per_search_con(2, C.byref(ev), n, 0, 0, 0) == plain
            assert emu.nla_local_ctx_bytes_per_search_con(2, C.byref(ev), n, 0, 4, 2) == plain      # (no launcher: nothing to size)


def test_the_library_exports_the_new_entry_points():
    L = C.CDLL(nlopt_amd.LIB_PATH)
    for name in ("nla_k_cobyla_batch_ext_con", "nla_cobyla_con_serves", "nla_cobyla_con_work_doubles", "nla_cobyla_con_save_bytes",
                 "nlopt_amd_batch_constraint_launches"):
        assert hasattr(L, name), name
    assert hasattr(nlopt_amd.Opt, "batch_constraint_launches")
    L.nla_cobyla_con_serves.argtypes = [C.c_int, C.c_int]
    assert [L.nla_cobyla_con_serves(n, mc) for n, mc in ((0, 1), (5, 0), (5, 8), (256, 175), (256, 176), (257, 1))] == [0, 0, 1, 1, 0, 0]


def test_the_constrained_cobyla_kernel_uses_no_scratch():
    """as tests/test_abi.py checks the hot kernels: the code object's own metadata"""
    if not os.path.isdir(os.path.join(ROOT, "nlopt_amd", "lib", "obj")) or not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no object files / no llvm-readelf here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.kernels() if "cobyla_batch_ext_con_kernel" in k["name"]]
    assert len(ks) == 1
    assert ks[0]["scratch"] == "0" and ks[0]["vgpr_spill"] == "0", ks[0]
    assert int(ks[0]["lds"]) <= 64, ks[0]                                        # (static LDS: the reduction buffers; the state is dynamic)
