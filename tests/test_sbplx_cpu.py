"""No GPU needed: what can be said about device LN_SBPLX (hip/sbplx_kernels.hip over hip/nm_search.h, nldrmd_driver.c) without running it.
  - the kernel cross-compiles for gfx950 and none of its instances uses scratch memory or spills a VGPR;
  - libnlopt_amd.so exports the launcher and its three size helpers, the Python package the constant;
  - over the EMULATED device layer (oracle/libnlopt_amd_emu.so, which has no such launcher — the drivers reach it through weak
    references) nlopt_optimize(LN_SBPLX) answers "not provided" as it always did and nlopt_amd_optimize_batch refuses, leaving x alone;
    nlopt_algorithm_name is unchanged.
tests/test_sbplx_emu.py runs the kernel's logic on the CPU, tests/test_gpu_sbplx.py the feature."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import nlopt_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")
SRC = os.path.join(ROOT, "nlopt_amd", "csrc", "hip", "sbplx_kernels.hip")
HIPCC = "/opt/rocm/bin/hipcc"
FUNC = C.CFUNCTYPE(C.c_double, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
vp, dpp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
LN_SBPLX, INVALID_ARGS = 29, -2


def test_every_kernel_of_the_code_object_uses_no_scratch_and_spills_no_vgpr(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf here")
    out = str(tmp_path / "sbplx_kernels.hsaco")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"), SRC, "-o", out],
                   check=True)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    ks = kernel_resources.code_object_kernels(out)
    names = [k["name"] for k in ks]
    assert sum("sbplx_batch_ext_kernel" in nm for nm in names) == 1 and sum("sbplx_batch_kernel" in nm for nm in names) == 6, names
    for k in ks:
        assert k["scratch"] == "0" and k["vgpr_spill"] == "0", k


def test_the_library_exports_the_launcher_and_its_helpers():
    L = C.CDLL(nlopt_amd.LIB_PATH)
    for sym in ("nla_k_sbplx_batch", "nla_sbplx_serves", "nla_sbplx_work_doubles", "nla_sbplx_save_bytes"):
        assert hasattr(L, sym), sym
    L.nla_sbplx_serves.argtypes = [C.c_int]
    assert [L.nla_sbplx_serves(n) for n in (0, 1, 256, 257)] == [0, 1, 1, 0]
    assert nlopt_amd.LN_SBPLX == LN_SBPLX


@pytest.fixture(scope="module")
def emu():
    if not os.path.exists(EMU):
        pytest.skip("oracle/libnlopt_amd_emu.so is not built here")
    L = C.CDLL(EMU)
    L.nlopt_create.restype = vp
    L.nlopt_create.argtypes = [C.c_int, C.c_uint]
    L.nlopt_destroy.argtypes = [vp]
    for nm in ("nlopt_set_lower_bounds", "nlopt_set_upper_bounds"):
        getattr(L, nm).argtypes = [vp, dpp]
    L.nlopt_set_min_objective.argtypes = [vp, vp, vp]
    L.nlopt_set_maxeval.argtypes = [vp, C.c_int]
    L.nlopt_optimize.argtypes = [vp, dpp, dpp]
    L.nlopt_get_errmsg.argtypes = [vp]
    L.nlopt_get_errmsg.restype = C.c_char_p
    L.nlopt_algorithm_name.argtypes = [C.c_int]
    L.nlopt_algorithm_name.restype = C.c_char_p
    L.nlopt_amd_optimize_batch.argtypes = [vp, C.c_size_t, dpp, dpp, ip, ip]
    return L


def _opt(L, calls):
    def f(nn, xp, gp, d):
        calls.append(1)
        return sum(xp[i] * xp[i] for i in range(nn))
    fcb = FUNC(f)
    o = L.nlopt_create(LN_SBPLX, 3)
    lb, ub = np.full(3, -2.0), np.full(3, 2.0)
    L.nlopt_set_lower_bounds(o, lb.ctypes.data_as(dpp)); L.nlopt_set_upper_bounds(o, ub.ctypes.data_as(dpp))
    L.nlopt_set_min_objective(o, C.cast(fcb, vp), None)
    L.nlopt_set_maxeval(o, 50)
    return o, fcb


def test_on_the_emulated_device_a_lone_run_is_not_provided_as_before(emu):
    calls = []
    o, keep = _opt(emu, calls)
    x, minf = np.array([0.5, -0.5, 1.0]), C.c_double(123.0)
    x0 = x.copy()
    try:
        assert emu.nlopt_optimize(o, x.ctypes.data_as(dpp), C.byref(minf)) == INVALID_ARGS
        assert emu.nlopt_get_errmsg(o).decode() == "algorithm LN_SBPLX is not provided by libnlopt_amd (stochastic-global hot path only)"
        assert np.array_equal(x, x0) and not calls
    finally:
        emu.nlopt_destroy(o)


def test_on_the_emulated_device_a_batch_is_refused_and_x_is_left_alone(emu):
    calls = []
    o, keep = _opt(emu, calls)
    X = np.array([[0.5, -0.5, 1.0], [1.0, 1.0, 1.0]])
    X0, minf, res, nev = X.copy(), np.full(2, 123.0), np.full(2, 77, dtype=np.intc), np.full(2, 77, dtype=np.intc)
    try:
        assert emu.nlopt_amd_optimize_batch(o, 2, X.ctypes.data_as(dpp), minf.ctypes.data_as(dpp), res.ctypes.data_as(ip), nev.ctypes.data_as(ip)) == INVALID_ARGS
        assert emu.nlopt_get_errmsg(o).decode() == "nlopt_amd_optimize_batch: this device layer has no LN_SBPLX launcher"
        assert np.array_equal(X, X0) and np.all(minf == 123.0) and np.all(res == 77) and np.all(nev == 77) and not calls
    finally:
        emu.nlopt_destroy(o)


def test_the_algorithm_name_is_unchanged(emu):
    assert emu.nlopt_algorithm_name(LN_SBPLX) == b"Sbplx variant of Nelder-Mead (re-implementation of Rowan's Subplex) (local, no-derivative)"
    L = C.CDLL(nlopt_amd.LIB_PATH)
    L.nlopt_algorithm_name.argtypes = [C.c_int]
    L.nlopt_algorithm_name.restype = C.c_char_p
    assert L.nlopt_algorithm_name(LN_SBPLX) == emu.nlopt_algorithm_name(LN_SBPLX)
