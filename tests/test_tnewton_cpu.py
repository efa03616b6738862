"""No GPU needed: what can be said about device LD_TNEWTON / _RESTART / _PRECOND / _PRECOND_RESTART (hip/tnewton_kernels.hip,
tnewton_driver.c) without running it.
  - the kernel is cross-compiled for gfx950, one instance per compiled-in objective and the coroutine;
  - no instance uses more scratch than the lbfgs_batch_kernel instance of the same objective did in the commit before this kernel
    (PARENT_SCRATCH: tools/kernel_resources.py on that commit's hip/lbfgs_kernels.hip), and today's lbfgs_batch_kernel still has those
    figures;
  - libnlopt_amd.so exports the launcher and its size helpers, the Python package the four constants;
  - over the EMULATED device layer (oracle/libnlopt_amd_emu.so, which has no such launcher — the drivers reach it through weak
    references) nlopt_optimize with each of the four ids answers "not provided" as it always did and nlopt_amd_optimize_batch refuses,
    leaving x alone.
tests/test_tnewton_emu.py runs the kernel's logic on the CPU, tests/test_gpu_tnewton.py the feature."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import nlopt_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")
HIP = os.path.join(ROOT, "nlopt_amd", "csrc", "hip")
OBJDIR = os.path.join(ROOT, "nlopt_amd", "lib", "obj")
HIPCC = "/opt/rocm/bin/hipcc"
FUNC = C.CFUNCTYPE(C.c_double, C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
vp, dpp, ip = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int)
IDS, INVALID_ARGS = (15, 16, 17, 18), -2
NAMES = {15: "LD_TNEWTON", 16: "LD_TNEWTON_RESTART", 17: "LD_TNEWTON_PRECOND", 18: "LD_TNEWTON_PRECOND_RESTART"}
# bytes of scratch per lane of lbfgs_batch_kernel<OBJ> in the commit before this kernel (OBJ: -1 the coroutine, 0 .. 5 rastrigin, ackley,
# griewank, rosenbrock, levy, sphere), with its VGPR count and LDS bytes
PARENT_LBFGS = {-1: (1588, 256, 51392), 0: (788, 252, 45312), 1: (788, 252, 45312), 2: (884, 252, 45312), 3: (724, 254, 45312), 4: (756, 252, 45312),
                5: (708, 254, 45312)}


def _resources():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kernel_resources
    finally:
        sys.path.remove(os.path.join(ROOT, "tools"))
    return kernel_resources


def _kernels(tmp_path, src, stem):
    """the code object's kernels: from the library's own object where the build left it, cross-compiled here otherwise"""
    K = _resources()
    if os.path.exists(os.path.join(OBJDIR, src.replace(".hip", ".o"))):
        return [k for k in K.kernels(OBJDIR) if k["file"] == src.replace(".hip", ".o") and stem in k["name"]]
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = str(tmp_path / src.replace(".hip", ".hsaco"))
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--genco", os.path.join(HIP, src), "-o", out], check=True)
    return [k for k in K.code_object_kernels(out) if stem in k["name"]]


def _obj_of(name):
    """the OBJ template argument from the mangled name: ILi3EE -> 3, ILin1EE -> -1"""
    m = re.search(r"_kernelILi(n?)(\d+)EE", name)
    return -int(m.group(2)) if m.group(1) else int(m.group(2))


def test_the_kernel_is_built_for_gfx950_within_the_l_bfgs_kernels_scratch(tmp_path):
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf here")
    tn = {_obj_of(k["name"]): k for k in _kernels(tmp_path, "tnewton_kernels.hip", "tnewton_batch_kernel")}
    lb = {_obj_of(k["name"]): k for k in _kernels(tmp_path, "lbfgs_kernels.hip", "lbfgs_batch_kernel")}
    assert sorted(tn) == sorted(lb) == sorted(PARENT_LBFGS), (sorted(tn), sorted(lb))
    for obj, (scratch, vgpr, lds) in PARENT_LBFGS.items():
        assert (int(lb[obj]["scratch"]), int(lb[obj]["vgpr"]), int(lb[obj]["lds"])) == (scratch, vgpr, lds), (obj, lb[obj])      # LD_LBFGS: unchanged
        assert int(tn[obj]["scratch"]) <= scratch, (obj, tn[obj])
        if obj >= 0:
            assert int(tn[obj]["scratch"]) == 0 and int(tn[obj]["vgpr"]) <= 256, (obj, tn[obj])          # two workgroups per CU, no spill


def test_the_library_exports_the_launcher_and_its_helpers():
    L = C.CDLL(nlopt_amd.LIB_PATH)
    for sym in ("nla_k_tnewton_batch", "nla_tnewton_work_doubles", "nla_tnewton_hist_doubles", "nla_tnewton_save_bytes"):
        assert hasattr(L, sym), sym
    L.nla_tnewton_hist_doubles.restype = C.c_size_t
    L.nla_tnewton_hist_doubles.argtypes = [C.c_int] * 3
    assert L.nla_tnewton_hist_doubles(10, 0, 4) == 0 and L.nla_tnewton_hist_doubles(10, 3, 4) == 240
    assert (nlopt_amd.LD_TNEWTON, nlopt_amd.LD_TNEWTON_RESTART, nlopt_amd.LD_TNEWTON_PRECOND, nlopt_amd.LD_TNEWTON_PRECOND_RESTART) == IDS


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
    L.nlopt_amd_optimize_batch.argtypes = [vp, C.c_size_t, dpp, dpp, ip, ip]
    return L


def _opt(L, alg, calls):
    def f(nn, xp, gp, d):
        calls.append(1)
        if gp:
            for i in range(nn):
                gp[i] = 2 * xp[i]
        return sum(xp[i] * xp[i] for i in range(nn))
    fcb = FUNC(f)
    o = L.nlopt_create(alg, 3)
    lb, ub = np.full(3, -2.0), np.full(3, 2.0)
    L.nlopt_set_lower_bounds(o, lb.ctypes.data_as(dpp)); L.nlopt_set_upper_bounds(o, ub.ctypes.data_as(dpp))
    L.nlopt_set_min_objective(o, C.cast(fcb, vp), None)
    L.nlopt_set_maxeval(o, 50)
    return o, fcb


@pytest.mark.parametrize("alg", IDS)
def test_on_the_emulated_device_a_lone_run_is_not_provided_as_before(emu, alg):
    calls = []
    o, keep = _opt(emu, alg, calls)
    x, minf = np.array([0.5, -0.5, 1.0]), C.c_double(123.0)
    x0 = x.copy()
    try:
        assert emu.nlopt_optimize(o, x.ctypes.data_as(dpp), C.byref(minf)) == INVALID_ARGS
        assert emu.nlopt_get_errmsg(o).decode() == "algorithm %s is not provided by libnlopt_amd (stochastic-global hot path only)" % NAMES[alg]
        assert np.array_equal(x, x0) and not calls
    finally:
        emu.nlopt_destroy(o)


@pytest.mark.parametrize("alg", IDS)
def test_on_the_emulated_device_a_batch_is_refused_and_x_is_left_alone(emu, alg):
    calls = []
    o, keep = _opt(emu, alg, calls)
    X = np.array([[0.5, -0.5, 1.0], [1.0, 1.0, 1.0]])
    X0, minf, res, nev = X.copy(), np.full(2, 123.0), np.full(2, 77, dtype=np.intc), np.full(2, 77, dtype=np.intc)
    try:
        assert emu.nlopt_amd_optimize_batch(o, 2, X.ctypes.data_as(dpp), minf.ctypes.data_as(dpp), res.ctypes.data_as(ip), nev.ctypes.data_as(ip)) == INVALID_ARGS
        assert emu.nlopt_get_errmsg(o).decode().startswith("nlopt_amd_optimize_batch serves ") and NAMES[alg] in emu.nlopt_get_errmsg(o).decode()
        assert np.array_equal(X, X0) and np.all(minf == 123.0) and np.all(res == 77) and np.all(nev == 77) and not calls
    finally:
        emu.nlopt_destroy(o)
