"""CPU: device objectives and constraints that read the caller's data (include/nlopt_amd_device.h ABI 2: NLOPT_AMD_DEVICE_RESIDUALS,
NLOPT_AMD_DEVICE_OBJECTIVE_DATA, NLOPT_AMD_DEVICE_CONSTRAINTS_DATA; include/nlopt_amd.h: nlopt_amd_set_device_objective_data,
nlopt_amd_add_*_device_mconstraint_data, nlopt_amd_eval_device_objective) as far as a machine without a GPU can see them: the samples
cross-compile for gfx950 with the header alone and define the kernels the library looks up, the residual kernel at NP = 32 keeps its
per-thread sums in registers, libnlopt_amd.so exports the entry points, and on the emulated device layer (where no code object can be
loaded) the setters fail loudly and change nothing.  tests/test_gpu_userdata.py runs the feature."""
import ctypes as C
import os
import subprocess
import sys

import pytest

import nlopt_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "userdata", "fit_models.hip")
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")
HIPCC = "/opt/rocm/bin/hipcc"
GN_CRS2_LM, GN_ISRES, INVALID_ARGS = 19, 35, -2
vp = C.c_void_p


@pytest.fixture(scope="module")
def image_path(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc here")
    out = str(tmp_path_factory.mktemp("userdata") / "fit_models.hsaco")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"), SRC, "-o", out],
                   check=True)
    return out


def test_the_samples_compile_for_gfx950_and_define_the_kernels(image_path):
    image = open(image_path, "rb").read()
    has = lambda sym: (sym.encode() + b"\0" in image) and (sym.encode() + b".kd\0" in image)     # the symbol's string and its kernel descriptor's
    for name in ("polyfit", "polyfit32", "expfit", "shifted"):
        for sym in ("_evalgrad_d", "_abi", "_form"):
            assert has(name + sym), name + sym
        assert (name + "_evalgrad.kd").encode() not in image, name              # an ABI-2 name brings no ABI-1 kernel
    assert has("lincons_coneval_d") and has("lincons_conabi") and b"lincons_coneval.kd" not in image
    assert has("sphere1_evalgrad") and has("sphere1_abi") and b"sphere1_evalgrad_d" not in image    # the ABI-1 macro beside them is unchanged


def test_the_residual_kernel_at_np_32_keeps_its_sums_in_registers(image_path):
    """x, the f partial and 32 gradient partials per thread are compile-time indexed: no scratch memory, no spilled VGPRs"""
    if not os.path.exists("/opt/rocm/lib/llvm/bin/llvm-readelf"):
        pytest.skip("no llvm-readelf here")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = {k["name"]: k for k in kernel_resources.code_object_kernels(image_path)}
    for name in ("polyfit32_evalgrad_d", "polyfit_evalgrad_d", "expfit_evalgrad_d"):
        k = ks[name]
        assert k["scratch"] == "0" and k["vgpr_spill"] == "0", k
        assert int(k["vgpr"]) + int(k["agpr"]) <= 256, k                       # a workgroup of 256 threads can be resident


def test_the_library_exports_the_new_entry_points():
    L = C.CDLL(nlopt_amd.LIB_PATH)
    for name in ("nlopt_amd_set_device_objective_data", "nlopt_amd_add_inequality_device_mconstraint_data",
                 "nlopt_amd_add_equality_device_mconstraint_data", "nlopt_amd_eval_device_objective"):
        assert hasattr(L, name), name
    for name in ("set_device_objective_data", "eval_device_objective", "copy"):
        assert hasattr(nlopt_amd.Opt, name), name


@pytest.fixture(scope="module")
def emu():
    assert os.path.exists(EMU), "oracle/libnlopt_amd_emu.so is not built (build() makes it)"
    L = C.CDLL(EMU)
    L.nlopt_create.restype = vp
    L.nlopt_create.argtypes = [C.c_int, C.c_uint]
    L.nlopt_destroy.argtypes = [vp]
    L.nlopt_get_errmsg.argtypes = [vp]
    L.nlopt_get_errmsg.restype = C.c_char_p
    L.nlopt_amd_set_min_device_objective.argtypes = [vp, C.c_char_p, C.c_char_p, vp, vp]
    L.nlopt_amd_has_device_objective.argtypes = [vp]
    L.nlopt_amd_set_device_objective_data.argtypes = [vp, vp, C.c_size_t]
    L.nlopt_amd_eval_device_objective.argtypes = [vp, C.c_size_t, vp, vp, vp]
    for nm in ("nlopt_amd_add_inequality_device_mconstraint_data", "nlopt_amd_add_equality_device_mconstraint_data"):
        getattr(L, nm).argtypes = [vp, C.c_uint, C.c_char_p, C.c_char_p, vp, vp, vp, vp, C.c_size_t]
    L.nlopt_amd_device_constraint_count.argtypes = [vp]
    return L


NOT_LOADABLE = os.path.join(HERE, "userdata", "fit_models.hsaco")        # (built or not: the emulated layer loads no code object)


def test_on_the_emulated_device_the_objective_setters_fail_loudly_and_change_nothing(emu):
    image_path = NOT_LOADABLE
    o = emu.nlopt_create(GN_CRS2_LM, 3)
    buf = (C.c_double * 4)(1, 2, 3, 4)
    f = (C.c_double * 1)(-7.0)
    try:
        assert emu.nlopt_amd_set_min_device_objective(o, image_path.encode(), b"polyfit", None, None) == INVALID_ARGS
        assert "could not load code object" in emu.nlopt_get_errmsg(o).decode()
        assert emu.nlopt_amd_has_device_objective(o) == 0
        assert emu.nlopt_amd_set_device_objective_data(o, buf, 32) == INVALID_ARGS
        assert "no device objective is bound" in emu.nlopt_get_errmsg(o).decode()
        assert emu.nlopt_amd_eval_device_objective(o, 1, buf, f, None) == INVALID_ARGS
        assert "no device objective is bound" in emu.nlopt_get_errmsg(o).decode() and f[0] == -7.0
        assert emu.nlopt_amd_has_device_objective(o) == 0
    finally:
        emu.nlopt_destroy(o)
    assert emu.nlopt_amd_set_device_objective_data(None, buf, 32) == INVALID_ARGS


@pytest.mark.parametrize("adder", ["nlopt_amd_add_inequality_device_mconstraint_data", "nlopt_amd_add_equality_device_mconstraint_data"])
def test_on_the_emulated_device_the_constraint_adders_fail_loudly_and_add_nothing(emu, adder):
    image_path = NOT_LOADABLE
    add = getattr(emu, adder)
    o = emu.nlopt_create(GN_ISRES, 3)
    buf = (C.c_double * 12)()
    try:
        for m, path, name, data, nbytes, msg in ((3, None, b"lincons", buf, 96, "need a code object path"), (0, image_path.encode(), b"lincons", buf, 96, "m > 0"),
                                                 (3, image_path.encode(), b"lincons", None, 96, "NULL with bytes > 0"),
                                                 (3, image_path.encode(), b"lincons", buf, 96, "could not load code object")):
            assert add(o, m, path, name, None, None, None, data, nbytes) == INVALID_ARGS
            assert msg in emu.nlopt_get_errmsg(o).decode()
            assert emu.nlopt_amd_device_constraint_count(o) == 0
    finally:
        emu.nlopt_destroy(o)
