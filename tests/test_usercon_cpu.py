"""CPU: user-supplied device constraints (include/nlopt_amd_device.h: NLOPT_AMD_DEVICE_CONSTRAINTS; include/nlopt_amd.h:
nlopt_amd_add_*_device_mconstraint) as far as a machine without a GPU can see them: the sample block cross-compiles for gfx950 and
defines the two kernels the library looks up, libnlopt_amd.so exports the new entry points, and on the emulated device layer (where no
code object can be loaded) the adders fail loudly and add nothing.  tests/test_gpu_usercon.py runs the feature."""
import ctypes as C
import os
import subprocess

import pytest

import nlopt_amd

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "usercon", "cons_extra.hip")
EMU = os.path.join(ROOT, "oracle", "libnlopt_amd_emu.so")
HIPCC = "/opt/rocm/bin/hipcc"
GN_ISRES, INVALID_ARGS = 35, -2
vp = C.c_void_p


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc here")
def test_the_sample_block_compiles_for_gfx950_and_defines_the_kernels(tmp_path):
    out = str(tmp_path / "cons_extra.hsaco")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--genco", "-I", os.path.join(ROOT, "include"), SRC, "-o", out],
                   check=True)
    image = open(out, "rb").read()
    for name in ("cons", "pair", "eqh", "many"):
        for sym in ("_coneval", "_conabi"):
            assert (name + sym).encode() + b"\0" in image, name + sym          # the symbol table's string
            assert (name + sym).encode() + b".kd\0" in image, name + sym       # ... and the kernel descriptor's
    assert b"cons_evalgrad.kd\0" in image and b"cons_abi.kd\0" in image       # the objective of the same name lives beside the block
    assert b"pair_evalgrad" not in image                                       # ... and a constraint block alone brings no objective kernel


def test_the_library_exports_the_new_entry_points():
    L = C.CDLL(nlopt_amd.LIB_PATH)
    for name in ("nlopt_amd_add_inequality_device_mconstraint", "nlopt_amd_add_equality_device_mconstraint",
                 "nlopt_amd_device_constraint_count", "nla_k_isres_eval_cv"):
        assert hasattr(L, name), name


def test_the_stats_mirror_matches_the_library():
    """nlopt_amd_stats is append-only; the ctypes mirror carries the new counter at its end and has the library's size"""
    L = nlopt_amd.lib()
    o = nlopt_amd.Opt(GN_ISRES, 2)
    L.nlopt_amd_get_stats_sized.restype = C.c_size_t
    L.nlopt_amd_get_stats_sized.argtypes = [vp, vp, C.c_size_t]
    s = nlopt_amd.Stats()
    assert L.nlopt_amd_get_stats_sized(o._h, C.byref(s), C.sizeof(s)) == C.sizeof(s)
    assert nlopt_amd.Stats._fields_[-1][0] == "isres_usercon_launches" and o.stats()["isres_usercon_launches"] == 0


@pytest.fixture(scope="module")
def emu():
    assert os.path.exists(EMU), "oracle/libnlopt_amd_emu.so is not built (build() makes it)"
    L = C.CDLL(EMU)
    L.nlopt_create.restype = vp
    L.nlopt_create.argtypes = [C.c_int, C.c_uint]
    L.nlopt_destroy.argtypes = [vp]
    L.nlopt_get_errmsg.argtypes = [vp]
    L.nlopt_get_errmsg.restype = C.c_char_p
    for nm in ("nlopt_amd_add_inequality_device_mconstraint", "nlopt_amd_add_equality_device_mconstraint"):
        getattr(L, nm).argtypes = [vp, C.c_uint, C.c_char_p, C.c_char_p, vp, vp, vp]
    L.nlopt_amd_device_constraint_count.argtypes = [vp]
    return L


@pytest.mark.parametrize("adder", ["nlopt_amd_add_inequality_device_mconstraint", "nlopt_amd_add_equality_device_mconstraint"])
def test_on_the_emulated_device_the_adders_fail_loudly_and_add_nothing(emu, adder):
    add = getattr(emu, adder)
    o = emu.nlopt_create(GN_ISRES, 3)
    try:
        for m, path, name, msg in ((2, None, b"cons", "need a code object path"), (2, SRC.encode(), None, "need a code object path"),
                                   (2, SRC.encode(), b"x" * 201, "need a code object path"), (0, SRC.encode(), b"cons", "m > 0"),
                                   (2, SRC.encode(), b"cons", "could not load code object"),
                                   (2, os.path.join(HERE, "usercon", "cons_extra.hsaco").encode(), b"cons", "could not load code object")):
            assert add(o, m, path, name, None, None, None) == INVALID_ARGS
            assert msg in emu.nlopt_get_errmsg(o).decode()
            assert emu.nlopt_amd_device_constraint_count(o) == 0
    finally:
        emu.nlopt_destroy(o)
    assert emu.nlopt_amd_device_constraint_count(None) == 0
